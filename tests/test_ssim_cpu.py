"""SSIM without a GPU: the fp64 restatement (tests/ssim_ref.py) against the reference-made fixtures (tests/golden/ssim_*.npz,
tools/gen_golden_ssim.py), the windows bit for bit, the reference callers' (H*W, 3) -> (1, 3, H, W) view, PSNR, and the
refusals of the C-ABI entries and of the Python functions (all before any device work)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import ssim_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
INRIA = sorted(f[:-4] for f in os.listdir(GOLDEN) if f.startswith("ssim_inria_"))
WINDOWS = (3, 7, 11)


def _load(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def test_fixture_set_is_complete():
    assert INRIA == ["ssim_inria_11", "ssim_inria_37x53", "ssim_inria_5x200", "ssim_inria_64", "ssim_inria_batch2",
                     "ssim_inria_const"]


@pytest.mark.parametrize("ws", WINDOWS)
@pytest.mark.parametrize("name", INRIA)
def test_restatement_reproduces_reference_ssim_inria(name, ws):
    z = _load(name)
    x, y = torch.from_numpy(z["x"]), torch.from_numpy(z["y"])
    got = R.inria(x, y, ws, bool(z["size_average"])).numpy()
    f64, f32 = z[f"f64_ws{ws}"], z[f"f32_ws{ws}"].astype(np.float64)
    assert got.shape == f64.shape
    assert np.abs(got - f64).max() <= 1e-12
    gap = np.abs(f32 - f64)                      # the reference's own fp32 / fp64 difference in this case
    assert np.all(np.abs(got - f32) <= gap + 1e-12)


@pytest.mark.parametrize("ws", WINDOWS)
def test_create_window_and_gaussian_bit_equal_reference(ws):
    from snerf_amd.eval.utils import metrics as M
    want = _load("ssim_misc")[f"window_{ws}"]
    got = M.create_window(ws, 3)
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, 1, ws, ws)
    assert np.array_equal(got.numpy().view(np.uint32), want.view(np.uint32))
    g = M.gaussian(ws, 1.5)
    assert g.dtype == torch.float32 and g.shape == (ws,)
    assert np.array_equal(g.unsqueeze(1).mm(g.unsqueeze(0)).numpy().view(np.uint32), want[0, 0].view(np.uint32))


@pytest.mark.parametrize("ws", (1, 3, 5, 11, 31))
def test_kornia_window_matches_restatement(ws):
    from snerf_amd.eval.utils import metrics as M
    got, want = M.kornia_window(ws), R.kornia_window(ws)
    assert got.dtype == torch.float32 and np.array_equal(got.numpy().view(np.uint32), want.numpy().view(np.uint32))
    assert abs(float(got.double().sum()) - 1.0) <= 1e-6


def test_reference_ssim_call_is_the_flat_view_with_window_3():
    """what the reference's metrics.ssim hands to kornia for an (H*W, 3) frame: the frame's flat buffer as (1, 3, H, W) -- its
    "channels" are the three thirds of the interleaved buffer -- and window 3"""
    z = _load("ssim_kornia_call")
    h, w = int(z["H"]), int(z["W"])
    assert int(z["window_size"]) == 3
    for frame, img in (("frame_pred", "image_pred"), ("frame_gt", "image_gt")):
        got = R.frame_view(torch.from_numpy(z[frame]), h, w).numpy()
        assert np.array_equal(got.view(np.uint32), z[img].view(np.uint32))
        assert not np.array_equal(got, np.ascontiguousarray(z[frame].T.reshape(1, 3, h, w)))   # not an R, G, B split


def test_psnr_matches_reference():
    from snerf_amd.eval.utils import metrics as M
    z = _load("ssim_misc")
    got = float(M.psnr(torch.from_numpy(z["psnr_pred"]), torch.from_numpy(z["psnr_gt"])))
    assert abs(got - float(z["psnr"])) <= 1e-5


def test_python_functions_refuse_cpu_tensors():
    from snerf_amd.eval.utils import metrics as M
    a = torch.rand(1, 3, 8, 8)
    with pytest.raises(ValueError, match="CUDA"):
        M.ssim(a, a)
    with pytest.raises(ValueError, match="CUDA"):
        M.ssim_inria(a, a, 3)


# ---- C-ABI refusals (host-side checks; nothing reaches the device) --------------------------------------------------------
def _lib():
    from snerf_amd import _lib
    return _lib, _lib.lib()


@pytest.mark.parametrize("args,msg", [
    ((1, 3, 8, 8, 4), b"odd"), ((1, 3, 8, 8, 0), b"odd"), ((1, 3, 8, 8, -3), b"odd"), ((1, 3, 8, 8, 33), b"odd"),
    ((0, 3, 8, 8, 3), b"> 0"), ((1, 0, 8, 8, 3), b"> 0"), ((1, 3, 0, 8, 3), b"> 0"), ((1, 3, 8, -1, 3), b"> 0"),
    ((2 ** 30, 3, 64, 64, 3), b"too large"), ((1, 1, 2 ** 30, 2 ** 30, 3), b"too large"),
])
def test_workspace_bytes_refusals(args, msg):
    _, L = _lib()
    assert L.snerf_ssim_workspace_bytes(*args) == 0
    assert msg in L.snerf_last_error()


def test_workspace_bytes_counts_tiles():
    _, L = _lib()
    assert L.snerf_ssim_workspace_bytes(1, 1, 1, 1, 1) == 8
    assert L.snerf_ssim_workspace_bytes(2, 3, 37, 53, 11) == 2 * 3 * 3 * 4 * 8      # 16 x 16 tiles: 3 rows x 4 columns


def _call(L, *, x=8, y=8, b=1, c=3, h=8, w=8, ws=3, border=0, weights=8, c1=1e-4, c2=9e-4, eps=1e-12, out=8, work=8,
          nbytes=1 << 20):
    """snerf_ssim with fake non-null device pointers: every case below is refused on the host before any launch"""
    p = lambda v: C.c_void_p(v)   # noqa: E731
    return L.snerf_ssim(p(x), p(y), b, c, h, w, ws, border, p(weights), c1, c2, eps, None, p(out), p(work), nbytes, None)


@pytest.mark.parametrize("kw,code,msg", [
    (dict(x=0), 3, b"null"), (dict(y=0), 3, b"null"), (dict(weights=0), 3, b"null"), (dict(out=0), 3, b"null"),
    (dict(work=0), 3, b"null"),
    (dict(ws=4), 1, b"odd"), (dict(ws=0), 1, b"odd"), (dict(ws=33), 1, b"odd"),
    (dict(b=0), 1, b"> 0"), (dict(h=0), 1, b"> 0"), (dict(w=-5), 1, b"> 0"),
    (dict(b=2 ** 30, h=64, w=64), 1, b"too large"),
    (dict(border=2), 1, b"border"),
    (dict(h=2, w=8, ws=5), 1, b"reflect"), (dict(h=8, w=1, ws=3), 1, b"reflect"), (dict(h=5, w=200, ws=11), 1, b"reflect"),
    (dict(c1=float("nan")), 1, b"finite"), (dict(eps=float("inf")), 1, b"finite"),
    (dict(nbytes=8), 2, b"workspace"),
])
def test_ssim_entry_refusals(kw, code, msg):
    _, L = _lib()
    assert _call(L, **kw) == code
    assert msg in L.snerf_last_error()


def test_zero_border_takes_windows_larger_than_the_image():
    """ssim_inria pads with zeros: a 5 x 200 image with window 11 is legal there (and only the workspace is refused here)"""
    _lib_mod, L = _lib()
    assert _call(L, h=5, w=200, ws=11, border=_lib_mod.SSIM_ZERO, nbytes=8) == 2
    assert b"workspace" in L.snerf_last_error()
