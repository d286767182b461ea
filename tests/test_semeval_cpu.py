"""Semantic evaluation without a GPU: the fp64 restatement (tests/semeval_ref.py) and the host arithmetic of
snerf_amd.eval.utils.semantic against the reference-made fixtures (tests/golden/semeval_*, tools/gen_golden_semeval.py), the
render-free results.json of snerf_amd.eval.eval_semantic against the file the reference's own loop wrote, the ctypes mirror
of SnerfSemevalAcc, the refusals of the C-ABI entries and of the Python functions (all before any device work), and the
build checks on the generated code of csrc/semeval.hip."""
import ctypes as C
import json
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import semeval_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CSRC = os.path.join(ROOT, "semantic-nerf-for-satellite-data_amd", "csrc")
METRIC_CASES = ("semeval_metrics_c2", "semeval_metrics_c5", "semeval_metrics_c9", "semeval_metrics_c16")
LOOPS = ("own", "own_corrupted")


def _S():
    from snerf_amd.eval.utils import semantic
    return semantic


def _load(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def _same_float(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


@pytest.mark.parametrize("name", METRIC_CASES)
def test_restatement_agrees_with_reference_metrics(name):
    z = _load(name)
    C_, car = int(z["n_classes"]), int(z["car_idx"])
    st = R.stats(z["pred"], z["gt"], C_, car, gt_no_cars=z["gt_no_cars"], gt_non_corrupted=z["gt"], weights=z["weights"],
                 beta=z["beta"])
    n = st["rays"]
    assert st["out_of_range"] == 0 and n == z["pred"].shape[0]
    # fp64 restatement within the reference's fp32 rounding
    assert abs(R.accuracy(st["errors"][0], n) - float(z["acc"])) <= 1e-7
    assert abs(R.accuracy(st["errors"][1], n) - float(z["acc_no_cars"])) <= 1e-7
    assert abs(R.accuracy(st["errors"][3], n) - float(z["acc_filter"])) <= 1e-7      # gt with filter_idx = car
    assert np.abs(R.normalized(st["conf"]) - z["cm"]).max() <= 1e-7
    assert abs(R.miou(z["cm"]) - float(z["miou"])) <= 1e-6
    unc = float(z["unc"])
    if st["car_rays"] == 0:
        assert math.isnan(unc) and name == "semeval_metrics_c9"
    else:
        assert abs(st["beta_car_sum"] / st["car_rays"] - unc) <= 1e-5 * abs(unc)
    # the product's host arithmetic: bit for bit
    S = _S()
    assert S.accuracy_from_errors(st["errors"][0], n) == float(z["acc"])
    assert S.accuracy_from_errors(st["errors"][1], n) == float(z["acc_no_cars"])
    assert S.accuracy_from_errors(st["errors"][3], n) == float(z["acc_filter"])
    cm = S.normalized_confusion(st["conf"])
    assert cm.dtype == np.float32 and np.array_equal(cm.view(np.uint32), z["cm"].view(np.uint32))
    assert _same_float(S.semantic_miou(cm), float(z["miou"]))


def test_metric_fixtures_cover_the_edge_cases():
    c2, c5, c9, c16 = (_load(n) for n in METRIC_CASES)
    assert float(c2["acc"]) == 1.0                                            # all correct
    g5 = set(c5["gt"].ravel().tolist())
    assert 3 not in g5 and 3 in set(c5["pred"].tolist())                     # predicted but absent from the ground truth
    assert int(c9["car_idx"]) not in set(c9["gt"].ravel().tolist()) and math.isnan(float(c9["unc"]))
    both = set(c16["gt"].ravel().tolist()) | set(c16["pred"].tolist())
    assert {4, 11}.isdisjoint(both)                                           # absent from both: NaN IoU, skipped
    assert all(z["gt"].dtype == np.uint8 and z["gt"].ndim == 2 for z in (c2, c5, c9, c16))


def _loop_entries(typ):
    """per-image entries of the fixture images from the restated statistics, through the product's host arithmetic"""
    S = _S()
    z = _load(f"semeval_loop_{typ}")
    C_, car = int(z["n_classes"]), int(z["car_idx"])
    names = [str(s) for s in z["names"]]
    nc = "gt_non_corrupted_0" in z.files
    entries, split = {}, np.zeros((C_, C_), np.int64)
    for i, name in list(enumerate(names))[1:]:               # the test split skips item 0
        st = R.stats(z[f"pred_{i}"], z[f"gt_{i}"], C_, car, gt_no_cars=z[f"gt_no_cars_{i}"],
                     gt_non_corrupted=z[f"gt_non_corrupted_{i}"] if nc else None, weights=z[f"weights_{i}"],
                     beta=z[f"beta_{i}"])
        entries[name] = S.entry_from_stats(st["conf"], st["errors"], st["rays"], st["car_rays"], st["beta_car_sum"],
                                           True, nc, True)
        split += st["conf"]
    return entries, split


def compare_results(got, want):
    """got (the product's dict) against want (the reference's results.json): keys and their order, per-image accuracies and
    matrices exactly, mIoU and uncertainty within 1e-6 relative, the means' strings equal or one unit of the last digit apart"""
    assert list(got) == list(want)
    for k, w in want.items():
        g = got[k]
        if isinstance(w, dict):
            assert list(g) == list(w), k
            for m, wv in w.items():
                if m in ("mIoU", "uncertainty_at_transient"):
                    assert (math.isnan(wv) and math.isnan(g[m])) or abs(g[m] - wv) <= 1e-6 * abs(wv), (k, m, g[m], wv)
                else:
                    assert g[m] == wv, (k, m)
        elif isinstance(w, str):
            assert re.fullmatch(r"-?\d+\.\d{4}|nan", g), (k, g)
            assert g == w or (w != "nan" and abs(float(g) - float(w)) <= 1e-4 + 1e-12), (k, g, w)
        else:
            assert g == w, k


@pytest.mark.parametrize("typ", LOOPS)
def test_semantic_results_reproduce_reference_results_json(typ):
    from snerf_amd.eval.eval_semantic import semantic_results
    with open(os.path.join(GOLDEN, f"semeval_loop_{typ}.json")) as f:
        want = json.load(f)
    entries, split = _loop_entries(typ)
    got = semantic_results(entries, split)
    compare_results(got, want)
    # the file form: the reference's json.dump(indent=4) of the same dict
    assert json.loads(json.dumps(got, indent=4)).keys() == want.keys()
    if typ == "own":
        assert want["Uncertainty at transient (Mean)"] == "nan"                          # an image without a car ray
        assert want["Semantic Accuracy comparison to GT (Mean)"] == "0.0000"             # a metric no image has
        assert "semantic_accuracy_comparison_non_corrupted" not in want["img_1"]
    else:
        assert want["Uncertainty at transient (Mean)"] != "nan"
        assert "semantic_accuracy_comparison_non_corrupted_wo_cars" in want["img_1"]
    # without the split counts: the per-image writes (no top-level matrix)
    assert "confusion_matrix" not in semantic_results(entries)


def test_results_catch_mutations():
    """what the fixture comparison is there to catch: a transposed matrix, a car filter on the wrong accuracy, NaN left in
    empty rows, mIoU over counts instead of the normalised matrix"""
    S = _S()
    from snerf_amd.eval.eval_semantic import semantic_results
    with open(os.path.join(GOLDEN, "semeval_loop_own_corrupted.json")) as f:
        want = json.load(f)
    entries, split = _loop_entries("own_corrupted")
    bad = {k: dict(v, confusion_matrix=np.array(v["confusion_matrix"]).T.tolist()) for k, v in entries.items()}
    with pytest.raises(AssertionError):
        compare_results(semantic_results(bad, split), want)
    bad = {k: dict(v, semantic_accuracy_comparison_non_corrupted=v["semantic_accuracy_comparison_non_corrupted_wo_cars"])
           for k, v in entries.items()}
    with pytest.raises(AssertionError):
        compare_results(semantic_results(bad, split), want)
    z = _load("semeval_loop_own_corrupted")
    conf = R.stats(z["pred_3"], z["gt_3"], 6, 4)["conf"]
    assert conf[1].sum() == 0                                  # class 1 is absent from image 3: an empty row
    assert not np.isnan(S.normalized_confusion(conf)).any()
    m_counts = S.semantic_miou(conf.astype(np.float32))
    assert abs(m_counts - want["img_3"]["mIoU"]) > 1e-3


def test_struct_mirror_matches_header():
    from snerf_amd import _lib
    A = _lib.SnerfSemevalAcc
    assert C.sizeof(A) == 8 * (16 * 16 + 4 + 3 + 1)
    assert A.errors.offset == 8 * 256 and A.rays.offset == 8 * 260 and A.out_of_range.offset == 8 * 262
    assert A.beta_car_sum.offset == 8 * 263
    hdr = open(os.path.join(ROOT, "include", "snerf_hip.h")).read()
    assert "#define SNERF_SEMEVAL_MAX_CLASSES 16" in hdr and _lib.SEMEVAL_MAX_CLASSES == 16
    assert "#define SNERF_SEMEVAL_U8 0" in hdr and "#define SNERF_SEMEVAL_I64 1" in hdr
    assert _lib.SEMEVAL_U8 == 0 and _lib.SEMEVAL_I64 == 1


def test_abi_refusals_before_device_work():
    from snerf_amd import _lib
    L = _lib.lib()
    assert L.snerf_semeval_workspace_bytes(-1, 8) == 0 and L.snerf_semeval_workspace_bytes(10, 0) == 0
    assert L.snerf_semeval_workspace_bytes(0, 1) == 8
    assert L.snerf_semeval_workspace_bytes(1000, 64) == 8 * 4
    assert L.snerf_semeval_workspace_bytes(1 << 30, 64) == 8 * 2048
    P = C.c_void_p(16)          # never dereferenced: every call below is refused on the host
    acc = C.c_void_p(4096)

    def call(pred=P, gt=P, dtype=0, n=100, ncls=5, car=1, w=None, b=None, S=8, a=acc, ws=None, wsb=0):
        return L.snerf_semeval_accumulate(pred, gt, None, None, dtype, n, ncls, car, w, b, S, a, ws, wsb, None)

    cases = [(dict(pred=None), "null pointer"), (dict(a=None), "null pointer"), (dict(n=-1), "n = -1"),
             (dict(ncls=0), "n_classes = 0"), (dict(ncls=17), "n_classes = 17"), (dict(car=-2), "car_idx = -2"),
             (dict(car=5), "car_idx = 5"), (dict(dtype=2), "label dtype"), (dict(w=P), "together"),
             (dict(w=P, b=P, S=0), "n_samples = 0"), (dict(w=P, b=P), "null workspace"),
             (dict(w=P, b=P, ws=P, wsb=7), "workspace of 7 bytes")]
    for kw, msg in cases:
        rc = call(**kw)
        assert rc != 0, kw
        assert msg in L.snerf_last_error().decode(), (kw, L.snerf_last_error())


def test_python_refusals_before_device_work():
    S = _S()
    from snerf_amd.eval.eval_semantic import eval_semantic_images, semantic_results
    for ncls, car in ((0, None), (17, None), (5, 5), (5, -2)):
        with pytest.raises(ValueError):
            S.SemanticEvalAccumulator(ncls, car, "cpu")
    with pytest.raises(ValueError, match="no test image"):
        eval_semantic_images(None, None, None, [{"name": "a"}], 5, 1)
    imgs = [{"name": f"i{k}", "semantic": 0, "semantic_no_cars": (0 if k != 2 else None)} for k in range(3)]
    with pytest.raises(ValueError, match="semantic_no_cars"):
        eval_semantic_images(None, None, None, imgs, 5, 1, split="train")
    imgs = [{"name": f"i{k}", "semantic": 0, "semantic_non_corrupted": (0 if k == 2 else None)} for k in range(3)]
    with pytest.raises(ValueError, match="semantic_non_corrupted"):
        eval_semantic_images(None, None, None, imgs, 5, 1)
    with pytest.raises(ValueError):
        semantic_results({})


def test_semeval_kernel_builds_clean():
    """csrc/semeval.hip's gfx950 code: no scratch, no spills, no float atomics, no scalar memory writes, and none of the
    register hazards tools/check_vgpr_hazards.py scans for"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not installed")
    import importlib.util
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "semeval.s")
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-function",
                            "-Wno-pass-failed", "-I" + CSRC, "--cuda-device-only", "-S", os.path.join(CSRC, "semeval.hip"),
                            "-o", out], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        lines = open(out).read().splitlines()
    text = "\n".join(lines)
    kernels = re.findall(r"^(_Z\w*semeval\w*):", text, re.M)
    assert len(kernels) == 3, kernels
    for key in (".private_segment_fixed_size", ".sgpr_spill_count", ".vgpr_spill_count"):
        vals = [int(v) for v in re.findall(re.escape(key) + r":\s+(\d+)", text)]
        assert len(vals) == 3 and not any(vals), (key, vals)
    assert not re.search(r"global_atomic_(add|pk_add)_f|cmpswap", text)
    mnemonics = {ln.split()[0].lower() for ln in lines if ln.strip() and not ln.lstrip().startswith((".", ";", "_"))}
    assert not [m for m in mnemonics if m.startswith("s_") and ("store" in m or "atomic" in m or "dcache" in m)]
    assert len(re.findall(r"global_atomic_add_x2", text)) >= 2
    spec = importlib.util.spec_from_file_location("check_vgpr_hazards", os.path.join(ROOT, "tools", "check_vgpr_hazards.py"))
    chk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(chk)
    assert not chk.scan_store(lines) and not chk.scan_lds(lines) and not chk.scan_trans(lines)
