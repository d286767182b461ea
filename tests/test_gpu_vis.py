"""Visualisation maps on the GPU (csrc/vismaps.hip through snerf_amd.eval.utils.vismaps and framework/visualize.py): the fold
against the reference-made fixtures and against the fp64 restatement at every sample-count regime and ragged ray counts, chunk
invariance and bit reproducibility, null inputs and absent heads, the colormap's indices and bounds, lean_frame_maps and
run_visualizer end to end on tests/golden/scene_small, peak memory, and two data-parallel ranks.

The bound of a weighted sum: |ours - ref| <= S * 2^-23 * sum_s |fl32(w_s f_s)| (tests/vis_ref.py sum_bound)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import vis_ref as R
from tests.test_vis_cpu import CASES, CMAPS, SUMS, check_maps_against_fixture, load

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
OUTS = {"albedo": "albedo_map", "sun": "sun_map", "sky": "sky_map", "beta": "beta_map", "beta_semantic": "beta_semantic_map",
        "depth": "depth_map", "rgb_diff": "rgb_diff", "rgb_diff_distance": "rgb_diff_distance", "sem_color": "sem_color",
        "sem_shaded": "sem_shaded", "sem_error": "sem_error"}


def _V():
    from snerf_amd.eval.utils import vismaps
    return vismaps


def _planes(n, which=tuple(OUTS)):
    out = {}
    for p in which:
        bands = 3 if p in ("albedo", "sky", "rgb_diff", "sem_color", "sem_shaded") else 1
        dt = torch.uint8 if p in ("sem_color", "sem_shaded") else torch.float32
        out[OUTS[p]] = torch.full((bands, n) if bands > 1 else (n,), 77, dtype=dt, device=DEV)
    return out


def _fold(c, chunk=None, which=tuple(OUTS)):
    """fold the case `c` (numpy arrays by SnerfVisIn name + palette) in chunks of `chunk` rays -> ({product: numpy}, stats)"""
    V = _V()
    n, S = c["weights"].shape
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in c.items()}
    planes, stats = _planes(n, which), V.new_stats(DEV)
    chunk = n if chunk is None else chunk
    for i in range(0, n, chunk):
        k = min(chunk, n - i)
        V.fold_chunk(planes, stats, i, n, k, S, **{key: (v if key == "palette" else v[i:i + k]) for key, v in d.items()})
    return {p: planes[OUTS[p]].cpu().numpy() for p in which}, stats


def _inputs(z):
    return {"weights": z["weights"], "albedo": z["albedo"], "sun": z["sun"], "sky": z["sky"], "beta": z["beta"],
            "beta_semantic": z["beta_semantic"], "depth": z["depth"], "rgb": z["rgb"], "rgbs_gt": z["rgbs"], "label": z["label"],
            "semantic_gt": z["semantic"].reshape(-1), "palette": z["palette"]}


def _want_bounds(got):
    return {k: R.minmax(got[k]) for k in ("depth", "sun", "beta", "beta_semantic", "rgb_diff_distance", "sem_error")}


@pytest.mark.parametrize("name", CASES)
def test_fold_against_reference_fixtures(name):
    z = load(name)
    got, stats = _fold(_inputs(z))
    report = {}
    check_maps_against_fixture(z, got, report)
    print(name, "max |ours - ref| / bound:", report)
    assert np.array_equal(got["depth"], z["depth"])
    st = _V().decode_stats(stats.cpu().numpy())
    assert st["bad_labels"] == 0
    for k, w in _want_bounds(got).items():
        assert st["bounds"][k] == w, k
    assert st["bounds"]["user"] is None


def _synth(g, n, S, C=5):
    f = lambda *s: torch.rand(*s, generator=g)                               # noqa: E731
    w = torch.softmax(torch.randn(n, S, generator=g) * 2, 1) * f(n, 1)
    lab = torch.randint(0, C, (n,), generator=g)
    c = {"weights": w, "albedo": f(n, S, 3), "sun": f(n, S, 1), "sky": f(n, S, 3) - 0.5, "beta": f(n, S, 1) + 0.05,
         "beta_semantic": f(n, S, 1), "depth": f(n) + 0.3, "rgb": f(n, 3), "rgbs_gt": f(n, 3), "label": lab,
         "semantic_gt": torch.where(f(n) < 0.7, lab, torch.randint(0, C, (n,), generator=g)),
         "palette": torch.randint(0, 256, (C, 3), generator=g).to(torch.uint8)}
    return {k: v.numpy() for k, v in c.items()}


def _check_against_restatement(c, got):
    w = c["weights"]
    for k in SUMS:
        ref, bound = R.weighted_sum(w, c[k]).astype(np.float64), R.sum_bound(w, c[k])
        assert (np.abs(got[k].astype(np.float64) - ref) <= bound).all(), k
        assert np.array_equal(got[k], R.weighted_sum(w, c[k])), k             # the spec itself: fp64 sum of fp32 products, one rounding
    assert np.array_equal(got["rgb_diff"], R.rgb_diff(c["rgb"], c["rgbs_gt"]))
    ref = R.rgb_diff_distance(c["rgb"], c["rgbs_gt"])
    assert (np.abs(got["rgb_diff_distance"].astype(np.float64) - ref) <= 2 * np.spacing(ref)).all()
    col, bad = R.sem_color(c["label"], c["palette"])
    assert np.array_equal(got["sem_color"], col)
    assert np.array_equal(got["sem_shaded"], R.sem_shaded(c["label"], c["palette"], got["sun"]))
    assert np.array_equal(got["sem_error"], R.sem_error(c["label"], c["semantic_gt"]))
    return bad


@pytest.mark.parametrize("S", (1, 3, 63, 64, 65, 130))
def test_sample_counts_and_ragged_rays(S):
    g = torch.Generator().manual_seed(500 + S)
    for n in (1, 255, 257, 1000):
        c = _synth(g, n, S)
        if n == 257:
            c["semantic_gt"] = c["semantic_gt"].astype(np.uint8)              # both label dtypes
        got, stats = _fold(c)
        assert _check_against_restatement(c, got) == 0
        st = _V().decode_stats(stats.cpu().numpy())
        for k, want in _want_bounds(got).items():
            assert st["bounds"][k] == want, (n, k)


def test_chunk_invariance_and_bit_reproducibility():
    g = torch.Generator().manual_seed(9)
    n = 1000
    c = _synth(g, n, 65)
    one, s1 = _fold(c)
    for chunk in (1, 7, 256, n):
        got, st = _fold(c, chunk)
        for k, v in one.items():
            assert np.array_equal(v.view(np.uint8), got[k].view(np.uint8)), (chunk, k)
        assert torch.equal(st, s1), chunk
    again, s2 = _fold(c)
    assert all(np.array_equal(one[k].view(np.uint8), again[k].view(np.uint8)) for k in one) and torch.equal(s1, s2)


def test_null_inputs_bad_labels_and_nan_stats():
    V = _V()
    z = load("vis_badlabel")
    c = _inputs(z)
    got, stats = _fold(c)
    assert _check_against_restatement(c, got) == 3
    assert V.decode_stats(stats.cpu().numpy())["bad_labels"] == 3 and (got["sem_color"][:, [3, 10, 17]] == 0).all()
    # only some inputs: the other planes are not touched, their slots stay empty
    some = {k: c[k] for k in ("weights", "sun", "depth")}
    got, stats = _fold(some, which=("sun", "depth"))
    assert np.array_equal(got["sun"], R.weighted_sum(c["weights"], c["sun"]))
    st = V.decode_stats(stats.cpu().numpy())["bounds"]
    assert st["beta"] is None and st["sem_error"] is None and st["sun"] == R.minmax(got["sun"])
    with pytest.raises(ValueError, match="without the input"):
        _fold(some, which=("sun", "beta"))
    with pytest.raises(ValueError, match="need weights"):
        V.fold_chunk({}, V.new_stats(DEV), 0, 24, 24, 5, sun=torch.from_numpy(c["sun"]).to(DEV))
    # NaN and inf enter the bounds as nan_to_num makes them
    d = c["depth"].copy()
    d[1], d[2], d[5] = np.nan, np.inf, -np.inf
    _, stats = _fold({"depth": d, "weights": c["weights"]}, which=("depth",))
    fmax = float(np.finfo(np.float32).max)
    assert V.decode_stats(stats.cpu().numpy())["bounds"]["depth"] == (-fmax, fmax)


def _identity():
    from snerf_amd.framework.util.colormaps import IDENTITY
    return torch.from_numpy(IDENTITY).to(DEV)


def test_colormap_indices_and_stats():
    V = _V()
    tab = _identity()
    planes = []
    for name in CASES:
        z = load(name)
        planes += [(f"{name}:{k}", z[f"cmap_{k}"], z[f"idx_{k}"], z[f"bounds_{k}"], z[f"idxb_{k}"]) for k in CMAPS]
    z = load("vis_nan_const")
    for dt in ("float32", "float64"):
        planes += [(f"nan_{dt}", z[f"cmap_nan_{dt}"], z[f"idx_nan_{dt}"], None, None),
                   (f"zero_{dt}", z[f"cmap_zero_{dt}"], z[f"idx_zero_{dt}"], None, None),
                   (f"const_{dt}", z[f"cmap_const_{dt}"], z[f"idx_const_{dt}"], z[f"bounds_const_{dt}"], z[f"idxb_const_{dt}"])]
    for what, plane, idx, bounds, idxb in planes:
        p = torch.from_numpy(plane).to(DEV)
        stats = V.plane_minmax(p, V.new_stats(DEV), "user")
        out = V.colormap(p, tab, stats=stats, slot="user").cpu().numpy()
        assert out.shape == (3,) + plane.shape and (out[0] == out[1]).all() and (out[0] == out[2]).all()
        assert np.array_equal(out[0], idx), what
        assert np.array_equal(V.colormap(p, tab).cpu().numpy()[0], idx), what
        if bounds is not None:
            assert np.array_equal(V.colormap(p, tab, cmap_bounds=tuple(bounds)).cpu().numpy()[0], idxb), what
        n2n = torch.nan_to_num(p)
        lo, hi = V.decode_stats(stats.cpu().numpy())["bounds"]["user"]
        assert lo == float(torch.amin(n2n)) and hi == float(torch.amax(n2n)), what
    # a real table: out = table[index]
    from snerf_amd.framework.util import colormaps as cm
    z = load(CASES[0])
    p = torch.from_numpy(z["cmap_sun"]).to(DEV)
    jet = V.colormap(p, cm.table(cm.COLORMAP_JET, DEV)).cpu().numpy()
    assert np.array_equal(jet, cm.TABLES[cm.COLORMAP_JET][z["idx_sun"]].transpose(2, 0, 1))


# ---- end to end ---------------------------------------------------------------------------------------------------------------
def _scene_pipeline(tmp_path, chunk=300, semantic=True):
    from snerf_amd.framework.configs import MainConfig
    from snerf_amd.framework.pipelines import load_pipeline
    scene = os.path.join(ROOT, "tests", "golden", "scene_small")
    name = "snerf_amd.semantic.pipelines.rs_semantic.RSSemanticPipeline" if semantic else "snerf_amd.baseline.pipelines.satnerf.SatNeRFPipeline"
    torch.manual_seed(0)
    c = MainConfig(run={"max_train_steps": 4, "dataset_dp": scene, "cache_dp": str(tmp_path), "dataset_name": "scene_small",
                        "run_dp": str(tmp_path / "run")},
                   pipeline={"pipeline": name, "fc_units": 64, "n_samples": 32, "batch_size": 128, "depth_enabled": False,
                             "first_beta_epoch": 0, "sparsity_n_images": 2, "render_chunk_size": chunk})
    return load_pipeline(c).to(DEV)


ALL = ("rgb", "depth", "albedo", "sun", "sky", "beta", "rgb_diff", "rgb_diff_distance", "sem_color", "sem_shaded", "sem_error")


def test_lean_frame_maps_equals_lean_inference_and_run_visualizer_writes_pngs(tmp_path):
    from PIL import Image
    from snerf_amd.eval.utils.util import lean_inference
    from snerf_amd.framework.util import colormaps as cm
    from snerf_amd.framework.visualize import run_visualizer
    from snerf_amd.baseline.components.visualize import AltsVisualization
    V = _V()
    pipe = _scene_pipeline(tmp_path)
    images = pipe.datasets["rgb_test"].scene_images()
    img = images[1]
    pal = torch.from_numpy(cm.DEFAULT_PALETTE)
    opts = {"perturb": 0}
    maps = V.lean_frame_maps(pipe.cfgs, pipe.renderer, pipe.models, img["rays"], img["extras"], rgbs=img["rgbs"],
                             semantic=img["semantic"], palette=pal, products=ALL, render_options=opts)
    keys = ("rgb", "depth", "weights", "albedo", "sun", "sky", "beta", "semantic_label")
    res = lean_inference(pipe.cfgs, pipe.renderer, pipe.models, img["rays"], img["extras"], keys=[k + "_coarse" for k in keys],
                         render_options=opts)
    c = {k: res[k + "_coarse"].cpu().numpy() for k in keys}
    c.update(label=c.pop("semantic_label"), rgbs_gt=img["rgbs"].cpu().numpy(), semantic_gt=img["semantic"].cpu().numpy().reshape(-1),
             palette=cm.DEFAULT_PALETTE, beta_semantic=c["beta"])
    got = {k: maps[k].cpu().numpy() for k in ALL}
    got["beta_semantic"] = got["beta"]
    assert _check_against_restatement(c, got) == 0
    assert np.array_equal(got["rgb"], c["rgb"]) and np.array_equal(got["depth"], c["depth"])
    assert maps.decode()["bounds"]["sun"] == R.minmax(got["sun"])
    vis = type(pipe).create_visualizers(pipe.cfgs) + [AltsVisualization(pipe.cfgs, False, False)]
    written = run_visualizer(pipe, split="test", epoch=3, create_visualizers_fn=lambda cfgs: vis,
                             render_options_fn=lambda p, s: {"perturb": 0})
    assert len(written) == len(vis) * len(images) == 10 * 3
    for k, im in enumerate(images):
        for v in vis:
            fp = tmp_path / "run" / "visualization" / ("train" if k == 0 else "test") / v._name() / f"{im['name']}_3.png"
            assert str(fp) in written
            with Image.open(fp) as png:
                assert png.size == (im["w"], im["h"]) and png.mode == "RGB"
    # the sun PNG of image 1 is the BONE table at the restated index of the folded plane
    with Image.open(tmp_path / "run" / "visualization" / "test" / "sun" / f"{img['name']}_3.png") as png:
        want = cm.TABLES[cm.COLORMAP_BONE][R.colormap_index(got["sun"])].reshape(img["h"], img["w"], 3)
        assert np.array_equal(np.asarray(png), want)


def test_model_without_semantic_head(tmp_path):
    V = _V()
    pipe = _scene_pipeline(tmp_path, semantic=False)
    img = pipe.datasets["rgb_test"].scene_images()[2]
    maps = V.lean_frame_maps(pipe.cfgs, pipe.renderer, pipe.models, img["rays"], img["extras"], rgbs=img["rgbs"],
                             products=V.BASELINE_PRODUCTS, render_options={"perturb": 0})
    assert set(maps.planes) == set(V.BASELINE_PRODUCTS) and torch.isfinite(maps["albedo"]).all()
    assert [v._name() for v in type(pipe).create_visualizers(pipe.cfgs)] == ["rgb", "depth", "albedo", "sun", "beta", "RGB_Diff_Distance"]
    with pytest.raises(ValueError, match="semantic head"):
        V.lean_frame_maps(pipe.cfgs, pipe.renderer, pipe.models, img["rays"], img["extras"], products=("sem_color",),
                          palette=torch.zeros(5, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="`rgbs`"):
        V.lean_frame_maps(pipe.cfgs, pipe.renderer, pipe.models, img["rays"], img["extras"], products=("rgb_diff",))


def test_peak_memory_stays_within_chunk_buffers_and_planes():
    """a 2^19-ray frame at S = 16 whose weights, albedo, sun, sky and beta would take 302 MB as whole-frame tensors: the fold's
    peak stays below lean_inference's of the same results by at least 90 % of them"""
    from tests.test_gpu_semeval import _image, _setup
    from snerf_amd.eval.utils.util import lean_inference
    V = _V()
    O, pipe = _setup(chunk=1 << 15)
    n, S = 1 << 19, 16
    small = _image(O, 4096, 9, "x")
    rays, extras = small["rays"].repeat(n // 4096, 1), small["extras"].repeat(n // 4096, 1)

    def peak(fn):
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        r = fn()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base, r

    keys = [k + "_coarse" for k in ("weights", "albedo", "sun", "sky", "beta")]
    g_inf, res = peak(lambda: lean_inference(pipe.cfgs, pipe.renderer, pipe.models, rays, extras, keys=keys))
    del res
    g_vis, maps = peak(lambda: V.lean_frame_maps(pipe.cfgs, pipe.renderer, pipe.models, rays, extras,
                                                 products=("albedo", "sun", "sky", "beta")))
    whole = n * S * 9 * 4
    planes = n * 8 * 4
    print(f"peak growth: lean_frame_maps {g_vis / 2**20:.1f} MiB, lean_inference {g_inf / 2**20:.1f} MiB, whole-frame per-sample "
          f"tensors {whole / 2**20:.1f} MiB, planes {planes / 2**20:.1f} MiB")
    assert whole > 300e6 and g_inf - g_vis >= 0.9 * whole - planes, (g_vis, g_inf, whole)
    assert maps["sun"].shape == (n,) and torch.isfinite(maps["albedo"]).all()


_DDP_WORKER = r"""
import os, sys
sys.path.insert(0, {root!r})
import torch, torch.distributed as dist
from snerf_amd import parallel
rank, world, dev = parallel.init_distributed(backend="gloo")
from tests.test_gpu_vis import _ddp_case
maps = _ddp_case(sharded=True)
torch.save({{"planes": {{k: v.cpu() for k, v in maps.planes.items()}}, "stats": maps.stats.cpu()}}, {out!r} + f".{{rank}}.pt")
dist.barrier()
"""


def _ddp_case(sharded):
    from tests.test_gpu_semeval import _image, _setup
    V = _V()
    O, pipe = _setup(chunk=700)
    img = _image(O, 3001, 81, "x")
    bank = O.batch_to_torch(O.synthetic_batch(3001, 16, seed=81))
    fn = V.sharded_lean_frame_maps if sharded else V.lean_frame_maps
    return fn(pipe.cfgs, pipe.renderer, pipe.models, img["rays"], img["extras"], rgbs=bank["rgbs"].to(DEV), semantic=img["semantic"],
              palette=torch.arange(15, dtype=torch.uint8).reshape(5, 3) * 17, products=ALL, render_options={"perturb": 0})


def test_two_ranks_equal_single_process(tmp_path):
    single = _ddp_case(sharded=False)
    script, out = tmp_path / "worker.py", str(tmp_path / "vis")
    script.write_text(_DDP_WORKER.format(root=ROOT, out=out))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29657", WORLD_SIZE="2", HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r), LOCAL_RANK="0"), cwd=ROOT) for r in range(2)]
    for p in procs:
        assert p.wait(timeout=300) == 0
    for r in range(2):
        got = torch.load(out + f".{r}.pt")
        assert torch.equal(got["stats"], single.stats.cpu()), r
        for k, v in single.planes.items():
            assert torch.equal(got["planes"][k].view(torch.uint8), v.cpu().view(torch.uint8)), (r, k)
