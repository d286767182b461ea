"""Semantic evaluation on the GPU (csrc/semeval.hip through snerf_amd.eval.utils.semantic): the kernel's statistics against the
fp64 restatement (tests/semeval_ref.py) at every class count, car index, label dtype and a range of ray and sample counts,
streaming over chunks, bit reproducibility, the refusal of out-of-range labels, the reference-made fixtures through the
kernel path, eval_semantic_images end to end against lean_inference, the peak memory of a 1M-ray frame, and two
data-parallel ranks."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import semeval_ref as R
from tests.test_semeval_cpu import LOOPS, METRIC_CASES, _load, compare_results

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def _S():
    from snerf_amd.eval.utils import semantic
    return semantic


def _case(g, n, C, S, car, dtype, corrupt=0.2):
    """labels mostly right, some wrong, some cars; weights and beta like a composite's"""
    gt = torch.randint(0, C, (n,), generator=g)
    pred = torch.where(torch.rand(n, generator=g) < corrupt, torch.randint(0, C, (n,), generator=g), gt)
    nocar = torch.where(gt == car, (gt + 1) % C, gt) if car >= 0 else gt.clone()
    nc = torch.where(torch.rand(n, generator=g) < 0.1, torch.randint(0, C, (n,), generator=g), gt)
    w = torch.softmax(torch.randn(n, S, generator=g) * 2, 1) * torch.rand(n, 1, generator=g)
    b = torch.rand(n, S, 1, generator=g) + 0.05
    return {"pred": pred, "gt": gt.to(dtype)[:, None], "nocar": nocar.to(dtype)[:, None], "nc": nc.to(dtype)[:, None],
            "w": w.float(), "b": b.float()}


def _dev(c):
    return {k: v.to(DEV) for k, v in c.items()}


def _host_stats(acc):
    return acc._read()


def _check(acc, c, C, car, with_nocar=True, with_nc=True, with_beta=True):
    want = R.stats(c["pred"], c["gt"], C, car, gt_no_cars=c["nocar"] if with_nocar else None,
                   gt_non_corrupted=c["nc"] if with_nc else None, weights=c["w"] if with_beta else None,
                   beta=c["b"] if with_beta else None)
    h = _host_stats(acc)
    assert np.array_equal(h["conf"], want["conf"])
    assert h["rays"] == want["rays"] and h["car_rays"] == want["car_rays"] and h["out_of_range"] == 0
    for i in range(4):
        if want["errors"][i] is not None:
            assert h["errors"][i] == want["errors"][i], i
        else:
            assert h["errors"][i] == 0, i
    if with_beta:
        ref = want["beta_car_sum"]
        assert abs(h["beta_car_sum"] - ref) <= 1e-12 * abs(ref), (h["beta_car_sum"], ref)
    else:
        assert h["beta_car_sum"] == 0.0


@pytest.mark.parametrize("dtype", (torch.uint8, torch.int64))
def test_kernel_matches_restatement_every_class_count(dtype):
    S_ = _S()
    g = torch.Generator().manual_seed(7 if dtype == torch.uint8 else 8)
    shapes = ((1, 1), (37, 7), (1000, 64), (4099, 130), (70001, 7), (300, 64))
    k = 0
    for C in range(1, 17):
        for car in sorted({-1, 0, C - 1}):
            n, S = shapes[k % len(shapes)]
            k += 1
            c = _case(g, n, C, S, car, dtype)
            d = _dev(c)
            opt = k % 3            # 0: every target; 1: no gt_no_cars / non_corrupted; 2: no beta
            acc = S_.SemanticEvalAccumulator(C, None if car < 0 else car, DEV)
            acc.add(d["pred"], d["gt"], None if opt == 1 else d["nocar"], None if opt == 1 else d["nc"],
                    weights=None if opt == 2 else d["w"], beta=None if opt == 2 else d["b"])
            _check(acc, c, C, car, opt != 1, opt != 1, opt != 2)


@pytest.mark.parametrize("S", (1, 7, 64, 130))
def test_kernel_sample_counts_and_ragged_rays(S):
    S_ = _S()
    g = torch.Generator().manual_seed(100 + S)
    for n in (1, 255, 257, 1023, 65537 + 13, 600_001):
        if n * S > 40_000_000:
            continue
        c = _case(g, n, 5, S, 4, torch.uint8)
        acc = S_.SemanticEvalAccumulator(5, 4, DEV)
        d = _dev(c)
        acc.add(d["pred"], d["gt"], d["nocar"], d["nc"], weights=d["w"], beta=d["b"])
        _check(acc, c, 5, 4)


def test_streaming_chunks_equal_one_call_and_runs_are_bit_identical():
    S_ = _S()
    g = torch.Generator().manual_seed(3)
    n, S, C, car = 300_007, 64, 9, 3
    d = _dev(_case(g, n, C, S, car, torch.uint8))

    def run(cuts):
        acc = S_.SemanticEvalAccumulator(C, car, DEV)
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            acc.add(d["pred"][lo:hi], d["gt"][lo:hi], d["nocar"][lo:hi], d["nc"][lo:hi], weights=d["w"][lo:hi],
                    beta=d["b"][lo:hi])
        return acc.buf.clone()

    one = run([0, n])
    chunked = run([0, 1000, 77_777, 200_000, 200_001, n])
    assert torch.equal(one[:-1], chunked[:-1])                       # every integer count
    b1, b2 = one[-1:].view(torch.float64).item(), chunked[-1:].view(torch.float64).item()
    assert abs(b1 - b2) <= 1e-12 * abs(b1)
    assert torch.equal(run([0, n]), one)                             # bit for bit, the fp64 sum included
    assert torch.equal(run([0, 1000, 77_777, 200_000, 200_001, n]), chunked)


def _order_case(n, S, seed):
    """three classes, car = 1 on about a third of the rays and on none of rays [200, 560) (a whole tile of 256 without a car);
    weights and beta of either sign with magnitudes spread over 2^-20 ... 2^20, so that the order shows in the low bits"""
    rng = np.random.default_rng(seed)
    gt = rng.integers(0, 3, n)
    gt[200:560] = np.where(gt[200:560] == 1, 0, gt[200:560])
    draw = lambda: (rng.uniform(1.0, 2.0, (n, S)) * 2.0 ** rng.integers(-20, 21, (n, S)) *                # noqa: E731
                    rng.choice((-1.0, 1.0), (n, S))).astype(np.float32)
    return gt, draw(), draw()


def test_beta_sum_is_the_restated_summation_order_bit_for_bit():
    """beta_car_sum against tests/semeval_ref.py beta_car_sum_in_kernel_order as int64 bits: n = 600 (three tiles, the last
    ragged; fewer partials than threads), 257 * 256 + 17 (258 partials: the strided part of the reduce launch) and
    2048 * 256 + 256 + 40 (more tiles than the grid cap: a workgroup walks two tiles).  A plain np.sum of the same products
    must differ from the restated value in at least one case, or the inputs could not tell one order from another."""
    S_ = _S()
    told_apart = False
    for k, (n, S) in enumerate(((600, 5), (257 * 256 + 17, 2), (2048 * 256 + 256 + 40, 1))):
        gt, w, b = _order_case(n, S, 40 + k)
        assert not (gt[200:560] == 1).any() and (gt[:200] == 1).any() and (gt[560:] == 1).any()
        want = R.beta_car_sum_in_kernel_order(gt, 1, w, b)
        plain = float(np.sum((w.astype(np.float64) * b.astype(np.float64))[gt == 1]))
        told_apart |= plain != want
        acc = S_.SemanticEvalAccumulator(3, 1, DEV)
        acc.add(torch.zeros(n, dtype=torch.int64, device=DEV), torch.from_numpy(gt).to(DEV),
                weights=torch.from_numpy(w).to(DEV), beta=torch.from_numpy(b).to(DEV)[..., None])
        got = acc._read()["beta_car_sum"]
        print(f"n = {n}, S = {S}: kernel {got!r}, restated {want!r}, np.sum {plain!r}")
        assert np.float64(got).view(np.int64) == np.float64(want).view(np.int64), (n, S, got, want)
    assert told_apart


def test_out_of_range_labels_are_refused():
    S_ = _S()
    pred = torch.zeros(100, dtype=torch.int64, device=DEV)
    for bad in (5, 200):
        gt = torch.zeros(100, 1, dtype=torch.uint8, device=DEV)
        gt[17] = bad
        acc = S_.SemanticEvalAccumulator(5, 4, DEV).add(pred, gt)
        assert acc._read()["out_of_range"] == 1
        with pytest.raises(ValueError, match="outside"):
            acc.image_entry()
    gt = torch.zeros(100, dtype=torch.int64, device=DEV)
    gt[3] = -1
    acc = S_.SemanticEvalAccumulator(5, None, DEV).add(pred, gt)
    with pytest.raises(ValueError, match="outside"):
        acc.image_entry()
    with pytest.raises(ValueError):                                       # weights without beta
        S_.SemanticEvalAccumulator(5, 4, DEV).add(pred, gt, weights=torch.zeros(100, 4, device=DEV))


@pytest.mark.parametrize("name", METRIC_CASES)
def test_metric_fixtures_through_the_kernel(name):
    S_ = _S()
    z = _load(name)
    C, car = int(z["n_classes"]), int(z["car_idx"])
    t = {k: torch.from_numpy(z[k]).to(DEV) for k in ("pred", "gt", "gt_no_cars", "weights", "beta")}
    acc = S_.SemanticEvalAccumulator(C, car, DEV)
    acc.add(t["pred"], t["gt"], t["gt_no_cars"], t["gt"], weights=t["weights"], beta=t["beta"])
    e = acc.image_entry()
    assert e["semantic_accuracy"] == float(z["acc"]) and e["semantic_accuracy_wo_cars"] == float(z["acc_no_cars"])
    assert e["semantic_accuracy_comparison_non_corrupted_wo_cars"] == float(z["acc_filter"])
    assert np.array_equal(np.array(e["confusion_matrix"], np.float32).view(np.uint32), z["cm"].view(np.uint32))
    m = float(z["miou"])
    assert (math.isnan(m) and math.isnan(e["mIoU"])) or e["mIoU"] == m
    u = float(z["unc"])
    if math.isnan(u):
        assert math.isnan(e["uncertainty_at_transient"])
    else:
        assert abs(e["uncertainty_at_transient"] - u) <= 1e-5 * abs(u)
        c = {"w": z["weights"], "b": z["beta"], "gt": z["gt"]}
        st = R.stats(z["pred"], c["gt"], C, car, weights=c["w"], beta=c["b"])
        assert abs(acc._read()["beta_car_sum"] - st["beta_car_sum"]) <= 1e-12 * st["beta_car_sum"]


@pytest.mark.parametrize("typ", LOOPS)
def test_reference_results_json_through_the_kernel(typ):
    S_ = _S()
    from snerf_amd.eval.eval_semantic import semantic_results
    z = _load(f"semeval_loop_{typ}")
    with open(os.path.join(ROOT, "tests", "golden", f"semeval_loop_{typ}.json")) as f:
        want = json.load(f)
    C, car = int(z["n_classes"]), int(z["car_idx"])
    nc = "gt_non_corrupted_0" in z.files
    entries, split = {}, np.zeros((C, C), np.int64)
    for i, name in list(enumerate(str(s) for s in z["names"]))[1:]:
        t = lambda k: torch.from_numpy(z[f"{k}_{i}"]).to(DEV)           # noqa: E731
        acc = S_.SemanticEvalAccumulator(C, car, DEV)
        half = z[f"pred_{i}"].shape[0] // 2                              # two chunks
        for lo, hi in ((0, half), (half, None)):
            acc.add(t("pred")[lo:hi], t("gt")[lo:hi], t("gt_no_cars")[lo:hi], t("gt_non_corrupted")[lo:hi] if nc else None,
                    weights=t("weights")[lo:hi], beta=t("beta")[lo:hi])
        entries[name] = acc.image_entry()
        split += acc.counts()
    compare_results(semantic_results(entries, split), want)


# ---- end to end -----------------------------------------------------------------------------------------------------------
def _setup(chunk=1000):
    from oracle import snerf_oracle as O
    from tests.test_gpu_pipeline import _pipeline_for
    cfg = O.OracleCfg(fc_units=32, n_samples=16, first_beta_epoch=0, render_chunk_size=chunk)
    pipe, _ = _pipeline_for(cfg, 256, 3)
    return O, pipe


def _image(O, n, seed, name, nc=False):
    bank = O.batch_to_torch(O.synthetic_batch(n, 16, seed=seed))
    sem = bank["semantic"].to(torch.uint8).reshape(-1, 1)
    img = {"name": name, "rays": bank["rays"].to(DEV), "extras": bank["extras"].to(DEV), "semantic": sem.to(DEV),
           "semantic_no_cars": torch.where(sem == 4, torch.zeros_like(sem), sem).to(DEV)}
    if nc:
        g = torch.Generator().manual_seed(seed)
        img["semantic_non_corrupted"] = torch.where(torch.rand(n, 1, generator=g) < 0.1, (sem + 1) % 5, sem).to(DEV)
    return img


def test_eval_semantic_images_equals_lean_inference(tmp_path):
    from snerf_amd.eval.eval_semantic import eval_semantic_images, semantic_results
    from snerf_amd.eval.utils.util import lean_inference
    S_ = _S()
    O, pipe = _setup(chunk=1000)
    for nc in (False, True):
        images = [_image(O, n, 60 + i, f"img_{i}", nc) for i, n in enumerate((4096, 3000, 2500))]
        assert any(int((img["semantic"] == 4).sum()) for img in images)
        torch.manual_seed(11)                   # the renderer's default jitter, drawn per chunk, image by image
        out = eval_semantic_images(pipe.cfgs, pipe.renderer, pipe.models, images, 5, 4, output_dp=str(tmp_path / str(nc)))
        with open(tmp_path / str(nc) / "results.json") as f:
            on_disk = json.load(f)
        assert list(on_disk) == list(out)
        assert list(out)[:2] == ["img_1", "img_2"]                       # item 0 skipped on the test split
        torch.manual_seed(11)
        entries, split = {}, np.zeros((5, 5), np.int64)
        for img in images[1:]:
            res = lean_inference(pipe.cfgs, pipe.renderer, pipe.models, img["rays"], img["extras"],
                                 keys=("semantic_label_coarse", "weights_coarse", "beta_coarse"))
            st = R.stats(res["semantic_label_coarse"].cpu(), img["semantic"].cpu(), 5, 4,
                         gt_no_cars=img["semantic_no_cars"].cpu(),
                         gt_non_corrupted=img["semantic_non_corrupted"].cpu() if nc else None,
                         weights=res["weights_coarse"].cpu(), beta=res["beta_coarse"].cpu())
            assert st["out_of_range"] == 0
            entries[img["name"]] = S_.entry_from_stats(st["conf"], st["errors"], st["rays"], st["car_rays"],
                                                       st["beta_car_sum"], True, nc, True)
            split += st["conf"]
            e = out[img["name"]]
            assert abs(e["semantic_accuracy"] - R.accuracy(st["errors"][0], st["rays"])) <= 1e-7
        want = semantic_results(entries, split)
        assert list(out) == list(want)
        for k, w in want.items():
            if isinstance(w, dict):
                for m, wv in w.items():
                    if m == "uncertainty_at_transient":
                        assert (math.isnan(wv) and math.isnan(out[k][m])) or abs(out[k][m] - wv) <= 1e-12 * abs(wv)
                    elif m == "mIoU":
                        assert out[k][m] == wv or (math.isnan(wv) and math.isnan(out[k][m]))
                    else:
                        assert out[k][m] == wv, (k, m)
            elif k == "Uncertainty at transient (Mean)":
                assert out[k] == w or abs(float(out[k]) - float(w)) <= 1e-4 + 1e-12
            else:
                assert out[k] == w, k
    # the train split keeps item 0; a model without a semantic head is refused
    tr = eval_semantic_images(pipe.cfgs, pipe.renderer, pipe.models, images, 5, 4, split="train")
    assert [k for k in tr if k.startswith("img_")] == ["img_0", "img_1", "img_2"]


def test_the_three_lean_evaluators_render_the_same_chunks():
    """a frame of 2 * chunk + 3 rays (a ragged last chunk) with the jitter pinned for the whole frame: lean_inference,
    lean_frame_maps and lean_semantic_eval go through util.render_chunks and give bit-identical rgb, depth and labels"""
    from snerf_amd.eval.utils.util import lean_inference
    from snerf_amd.eval.utils.vismaps import lean_frame_maps
    S_ = _S()
    chunk = 500
    O, pipe = _setup(chunk=chunk)
    n = 2 * chunk + 3
    img = _image(O, n, 70, "x")
    opts = {"perturb_rand": torch.rand(n, 16, generator=torch.Generator().manual_seed(5)).to(DEV)}
    args = (pipe.cfgs, pipe.renderer, pipe.models, img["rays"], img["extras"])
    res = lean_inference(*args, render_options=opts)
    maps = lean_frame_maps(*args, products=("rgb", "depth"), render_options=opts)
    assert torch.equal(maps["rgb"], res["rgb_coarse"]) and torch.equal(maps["depth"], res["depth_coarse"])

    class Recording(S_.SemanticEvalAccumulator):
        def add(self, pred, *a, **kw):
            self.labels = getattr(self, "labels", []) + [pred.clone()]
            return super().add(pred, *a, **kw)

    acc = S_.lean_semantic_eval(*args, img["semantic"], car_cls_idx=4, render_options=opts, acc=Recording(5, 4, DEV))
    assert [t.numel() for t in acc.labels] == [chunk, chunk, 3]
    assert torch.equal(torch.cat(acc.labels), res["semantic_label_coarse"])
    st = R.stats(res["semantic_label_coarse"].cpu(), img["semantic"].cpu(), 5, 4)
    assert np.array_equal(acc.counts(), st["conf"]) and acc._read()["rays"] == n


def test_model_without_semantic_head_is_refused():
    from oracle import snerf_oracle as O
    from tests.test_gpu_pipeline import _pipeline_for
    from snerf_amd.eval.utils.semantic import lean_semantic_eval
    cfg = O.OracleCfg(model="satnerf", fc_units=32, n_samples=16)
    pipe, _ = _pipeline_for(cfg, 256, 3)
    img = _image(O, 512, 5, "x")
    with pytest.raises(ValueError, match="no semantic head"):
        lean_semantic_eval(pipe.cfgs, pipe.renderer, pipe.models, img["rays"], img["extras"], img["semantic"])


def test_peak_memory_stays_far_below_whole_frame_tensors():
    """on a 1M-ray frame, lean_semantic_eval's peak allocation stays below that of lean_inference of the same results by at
    least 90 % of the whole-frame (N, S) weights and beta: both hold the same chunk workspace, only lean_inference the frame"""
    from snerf_amd.eval.utils.semantic import lean_semantic_eval
    from snerf_amd.eval.utils.util import lean_inference
    O, pipe = _setup(chunk=1 << 15)
    n, S = 1 << 20, 16
    small = _image(O, 4096, 9, "x")
    reps = n // 4096
    rays = small["rays"].repeat(reps, 1)
    extras = small["extras"].repeat(reps, 1)
    sem = small["semantic"].repeat(reps, 1)

    def peak(fn):
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        r = fn()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base, r

    keys = ("semantic_label_coarse", "weights_coarse", "beta_coarse")
    g_inf, res = peak(lambda: lean_inference(pipe.cfgs, pipe.renderer, pipe.models, rays, extras, keys=keys))
    del res
    g_sem, acc = peak(lambda: lean_semantic_eval(pipe.cfgs, pipe.renderer, pipe.models, rays, extras, sem, car_cls_idx=4))
    e = acc.image_entry()
    whole = 2 * n * S * 4
    print(f"peak growth: lean_semantic_eval {g_sem / 2**20:.1f} MiB, lean_inference {g_inf / 2**20:.1f} MiB, "
          f"whole-frame weights + beta {whole / 2**20:.1f} MiB")
    assert g_inf - g_sem >= 0.9 * whole, (g_sem, g_inf, whole)
    assert acc._read()["rays"] == n and 0.0 < e["semantic_accuracy"] <= 1.0


_DDP_WORKER = r"""
import os, sys, json
sys.path.insert(0, {root!r})
import numpy as np, torch, torch.distributed as dist
from snerf_amd import parallel
rank, world, dev = parallel.init_distributed(backend="gloo")
from tests.test_gpu_semeval import _setup, _image
from snerf_amd.eval.eval_semantic import eval_semantic_images
O, pipe = _setup(chunk=700)
images = [_image(O, n, 80 + i, f"img_{{i}}", True) for i, n in enumerate((4096, 3001, 5))]
out = eval_semantic_images(pipe.cfgs, pipe.renderer, pipe.models, images, 5, 4, output_dp={out!r} + f".{{rank}}", sharded=True,
                           render_options={{"perturb": 0}})
with open({out!r} + f".{{rank}}.ret.json", "w") as f:
    json.dump(out, f)
dist.barrier()
"""


def test_data_parallel_equals_single_process(tmp_path):
    """2 ranks (gloo, both on this GPU), each streaming its frame_shard slice of every image (the third image has 5 rays:
    ragged shards): counts, accuracies and matrices equal the single-process values bit for bit, the uncertainty within 1e-12
    relative; only rank 0 writes results.json"""
    from snerf_amd.eval.eval_semantic import eval_semantic_images
    O, pipe = _setup(chunk=700)
    images = [_image(O, n, 80 + i, f"img_{i}", True) for i, n in enumerate((4096, 3001, 5))]
    single = eval_semantic_images(pipe.cfgs, pipe.renderer, pipe.models, images, 5, 4, render_options={"perturb": 0})
    script = tmp_path / "worker.py"
    out = str(tmp_path / "sem")
    script.write_text(_DDP_WORKER.format(root=ROOT, out=out))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29653", WORLD_SIZE="2", HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r), LOCAL_RANK="0"), cwd=ROOT)
             for r in range(2)]
    for p in procs:
        assert p.wait(timeout=300) == 0
    assert os.path.exists(out + ".0/results.json") and not os.path.exists(out + ".1/results.json")
    single = json.loads(json.dumps(single))
    for r in range(2):
        with open(out + f".{r}.ret.json") as f:
            got = json.load(f)
        assert list(got) == list(single)
        for k, w in single.items():
            if isinstance(w, dict):
                for m, wv in w.items():
                    if m == "uncertainty_at_transient":
                        assert (math.isnan(wv) and math.isnan(got[k][m])) or abs(got[k][m] - wv) <= 1e-12 * abs(wv)
                    else:
                        assert got[k][m] == wv or (isinstance(wv, float) and math.isnan(wv) and math.isnan(got[k][m])), (k, m)
            elif k != "Uncertainty at transient (Mean)":
                assert got[k] == w, (r, k)
