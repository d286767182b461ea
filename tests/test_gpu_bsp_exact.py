"""The plane GEMMs (csrc/bsp_gemm.hip, bsp_kc.hip, epilogues of bsp_kc_epi.h) element by element against an OPERAND-EXACT reference.

tests/test_gpu_bsp.py compares these kernels with the fp64 product of the fp32 inputs, so its bars have to swallow the operand
rounding of the format (2^-11 with one plane) and can only be norms.  Here the operands are quantised by a numpy restatement
of the format (tests/bsp_numpy.py; parts a and b hold it to the library bit for bit), the reference is the fp64 sum of exactly
the products the matrix cores are given, and what is left for the kernel is fp32 accumulation and ONE rounding of the output:
  * fp32 outputs (narrow variant, dW):  |got - exact| <= acc_bound(n, mag) = (n + 2) 2^-23 sum |terms|, element-wise;
  * plane outputs:  bsp_numpy.on_grid_near -- on the block's grid, within half a grid spacing + acc_bound of the exact value.
Both hold for either plane count.  No bar here was read off a GPU run: each is derived where it is used, or names the existing
test it is taken from.  Every comparison appends its worst error / bound to RATIOS (printed with -s)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import bsp_numpy as N

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ACT_NONE, ACT_SIN, ACT_RELU = 0, 1, 2
AUX_NONE, AUX_RELU_MASK, AUX_SINREC = 0, 2, 3
RATIOS = []     # (case, worst error / bound)
# Relative error of the derivative epilogue's fp32 rebuild of w0 |cos| and its application (bsp_kc.hip, AUX_SINREC), in order:
#   s = hi + lo                       one mixed-precision FMA, exact (bsp.h: sum8 / cvt8f)
#   om = fma(-s, s, 2^2eH)            ONE rounding of the exact 2^2eH (1 - h^2): 2^-24; halved by the root: 2^-25
#   root = v_sqrt_f32(|om|)           the guides give no accuracy for it; taken as 2 ulp = 2^-22 (the ISA manual states 1 ulp)
#   v = raw accumulator * root        one rounding: 2^-24
#   v * (2^eC 2^-e_in |w0| 2^-eH)     the plane split's FMA forms the product in fp32 before it rounds to fp16: 2^-24 (|w0| is
#                                     no power of two; the other factors are)
# sum 13 * 2^-25, taken as 2^-21 (second-order terms).  The bound is relative to the result; nothing is divided by |cos|.
SINREC_REL = 2.0 ** -21
SIN_BAR = 4e-6     # the sine epilogue's own bar, times max(1, w0 / 8): tests/test_gpu_bsp.py, test_kc_siren_forward_then_derivative_epilogue


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _lib():
    from snerf_amd import _lib
    return _lib.lib(), _lib


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


def _record(case, ratio):
    RATIOS.append((case, float(ratio)))
    print(f"error / bound {float(ratio):9.3e}  {case}")


def _randn(g, *shape):
    return torch.randn(*shape, generator=g).numpy()


@pytest.fixture(params=[0, 3, 2], ids=["grid_default", "grid_3_workgroups", "grid_2_workgroups"])
def kc_grid(request):
    """the default persistent grid (one tile per workgroup at these sizes) and forced grids of 3 / 2 workgroups, where every
    workgroup walks several tiles drawn from the tile counters (snerf_test_set_kc_grid)"""
    L, _ = _lib()
    L.snerf_test_set_kc_grid(request.param)
    yield request.param
    L.snerf_test_set_kc_grid(0)


def _kc(A, W, bias=None, A2=None, act=ACT_NONE, w0=1.0, aux=AUX_NONE, Hact=None, Hsign=None, a_col0=0, c_col0=0,
        want_sign=False, want_colsum=False, narrow=False, planes=2, nd_w=None, nd_rows=None):
    """one launch through snerf_test_bsp_kc; numpy fp32 in, torch tensors out: (C, sign words, colsum or nd_out)"""
    L, lib = _lib()
    A, W, bias, A2, nd_w = _dev(A), _dev(W), _dev(bias), _dev(A2), _dev(nd_w)
    Hact = _dev(Hact) if isinstance(Hact, np.ndarray) else Hact
    I, Ka = A.shape
    K = Ka + (A2.shape[1] if A2 is not None else 0)
    J = W.shape[0]
    Cm = torch.full((I, 32 if narrow else J), float("nan"), device=DEV)
    ldc = c_col0 + (J + 15) // 16 * 16
    sign = torch.zeros(((I + 127) // 128 * 128 // 32) * ((ldc + 63) // 64) * 64, dtype=torch.int32, device=DEV) if want_sign else None
    cs = torch.zeros(((I + 127) // 128, J), device=DEV) if want_colsum else None
    nd_out = torch.full((((J + 255) // 256) * 4 * (5 if nd_rows else 1), I), float("nan"), device=DEV) if nd_w is not None else None
    rows_c = (C.c_int * len(nd_rows))(*nd_rows) if nd_rows else None
    lib.check(L.snerf_test_bsp_kc(_p(A), _p(A2), Ka, _p(W), _p(bias), I, J, K, a_col0, c_col0, act, w0, aux, _p(Hact), _p(Hsign),
                                  _p(Cm), _p(sign), _p(cs), _p(nd_w), _p(nd_out), rows_c, int(narrow), planes, _st()), "test_bsp_kc")
    return Cm, sign, (nd_out if nd_w is not None else cs)


def _roundtrip(x, ld, col0, planes):
    L, lib = _lib()
    x = _dev(x) if isinstance(x, np.ndarray) else x
    rows, cols = x.shape
    y = torch.empty_like(x)
    E = torch.full((((rows + 127) // 128) * ((ld + 127) // 128),), -7, dtype=torch.int32, device=DEV)
    lib.check(L.snerf_test_bsp_roundtrip(_p(x), rows, cols, ld, col0, _p(y), _p(E), planes, _st()), "roundtrip")
    return y, E


def _qa(A, planes):
    """dequantised activation planes of an fp32 matrix (blocks anchored at its column 0, wherever the hook places it)"""
    hi, lo, e = N.to_planes(A, planes)
    return N.deq(hi, lo, N.expand(e, *A.shape))


def _exact_kc(A, W, planes, A2=None):
    """exact product and mag of a K-contiguous launch: A [I][Ka] (| A2, quantised on its own), W [J][K]"""
    ah, al = _qa(A, planes)
    if A2 is not None:
        a2h, a2l = _qa(A2, planes)
        ah, al = np.concatenate([ah, a2h], 1), np.concatenate([al, a2l], 1)
    wh, wl, ew = N.weight_planes(W, planes)
    wh, wl = N.deq(wh, wl, ew)
    return N.exact_product(ah, al, wh.T.copy(), wl.T.copy(), planes)


# ---------------------------------------------------------------------------------------------------------------------------------
# a. storage round trip, bit for bit
# ---------------------------------------------------------------------------------------------------------------------------------
def _roundtrip_input():
    """300 x 200: blocks (row block, column block) of 128 x 128 / 128 x 72 / 44 x 128 / 44 x 72
      (0,0) quiet (x 1e-6), a -0          (0,1) all zero, a -0
      (1,0) loud (x 3e3), |max| = 2^14 exactly
      (1,1) a value that rounds up to 2^14 on the hi plane; rounding ties of the hi plane, of the lo plane and in the fp16
            subnormal range of the block; values that flush to zero; the subnormal / normal boundary
      (2,0) beyond the quiet clamp (|max| < 2^-47: exponent 60, bits lost)      (2,1) beyond the loud clamp (|max| >= 2^114)"""
    x = _randn(torch.Generator().manual_seed(0), 300, 200).copy()
    x[:128, :128] *= np.float32(1e-6)
    x[5, 7] = -0.0
    x[:128, 128:] = 0.0
    x[3, 130] = -0.0
    x[128:256, :128] *= np.float32(3e3)
    assert np.abs(x[128:256, :128]).max() < 2.0 ** 14
    x[200, 64] = 2.0 ** 14
    b = x[128:256, 128:]
    b *= np.float32(0.3)
    assert np.abs(b).max() < 1.9
    b[0, 0] = 2.0 - 2.0 ** -18                                          # 2^14 - 2^-5 under the block's exponent 13
    b[1, 1], b[1, 2] = 1025.5 * 2.0 ** -13, 1026.5 * 2.0 ** -13          # hi-plane ties, one to each side
    b[1, 3] = -(2048.5 + 2.0 ** -11 + 2.0 ** -12) * 2.0 ** -13           # a lo-plane tie (24 bits: exact in fp32)
    b[2, 1], b[2, 2], b[2, 3] = 5.5 * 2.0 ** -37, 2.0 ** -39, -6.5 * 2.0 ** -37   # subnormal tie, flush to zero, subnormal tie
    b[2, 4] = 1023.75 * 2.0 ** -37                                      # rounds up to the smallest fp16 normal
    b[2, 5] = 3.2 * 2.0 ** -37                                          # an odd subnormal
    x[256:, :128] *= np.float32(2.0 ** -50)
    x[256, 1] = 1.3 * 2.0 ** -80
    x[256:, 128:] *= np.float32(2.0 ** 113)
    x[257, 129] = 1.5 * 2.0 ** 115
    return x.astype(np.float32)


@pytest.mark.parametrize("planes", [2, 1])
def test_round_trip_bit_for_bit(planes):
    x = _roundtrip_input()
    rows, cols, ld, col0 = 300, 200, 384, 128
    hi, lo, e = N.to_planes(x, planes)
    # the inputs reach the edges they are meant to reach (on the restatement)
    assert e[0, 1] == 0 and e[1, 0] == -1 and e[1, 1] == 13 and e[2, 0] == N.E_QUIET and e[2, 1] == -N.E_MAX, e
    assert hi[200, 64] == 2.0 ** 13 and hi[128, 128] == 2.0 ** 14 and hi[129, 129] == 1026.0 and hi[129, 130] == 1026.0
    assert hi[130, 129] == 6 * 2.0 ** -24 and hi[130, 130] == 0.0 and hi[130, 132] == 2.0 ** -14
    assert planes == 1 or lo[129, 131] in (-(0.5 + 2.0 ** -10), -(0.5 + 2.0 ** -11))
    assert np.abs(hi[256:, 128:]).max() == 1.5 * 2.0 ** 15 and np.isfinite(hi).all()
    want = N.from_planes(hi, lo, N.expand(e, rows, cols))
    assert np.isfinite(want).all() and (np.abs(want[want != 0]) >= 2.0 ** -126).all()     # inside the fp32 normal range
    y, E = _roundtrip(x, ld, col0, planes)
    E = _np(E).reshape(3, 3)
    want_E = np.zeros((3, 3), np.int64)
    want_E[:, 1:] = e                                       # blocks anchored at the source's column 0, placed at column block 1
    assert np.array_equal(E, want_E), (E, want_E)
    got = _np(y)
    diff = got.view(np.int32) != want.view(np.int32)
    assert not diff.any(), (int(diff.sum()), np.argwhere(diff)[:8].tolist())


# ---------------------------------------------------------------------------------------------------------------------------------
# b. weight pack, bit for bit: one-hot rows read the packed matrix out through the narrow (fp32 output) launch
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("planes", [2, 1])
@pytest.mark.parametrize("J,K", [(32, 16), (9, 64), (20, 528)])
def test_weight_pack_bit_for_bit(J, K, planes):
    """A = identity (K x K): 1.0 is exact in the format (2^13 under exponent 13; the all-zero blocks beside the diagonal carry
    exponent 0 and the accumulators are rescaled across them, exactly), every output is one product, and C[i][j] is the packed
    W[j][i]: fp32 (hi + lo) 2^-e.  W has a heavy tail, so most of it lies deep below the matrix's one exponent (fp16 subnormals)."""
    g = torch.Generator().manual_seed(100 + K)
    W = (_randn(g, J, K) * 10.0 ** (1.5 * _randn(g, J, K))).astype(np.float32)
    m = np.abs(W).max()
    W[0, :4] = 0.0, m * 2.0 ** -30, -m * 2.0 ** -45, m * 2.0 ** -26     # zero, fp16 subnormal, flushed, subnormal
    hi, lo, e = N.weight_planes(W, planes)
    assert (hi == 0).sum() > 1 and (np.abs(hi[hi != 0]) < 2.0 ** -14).any()      # flushed and subnormal entries exist
    want = N.from_planes(hi, lo, e) + np.float32(0.0)     # (a flushed negative entry is -0 on the planes; the accumulators start at +0)
    Cm, _, _ = _kc(np.eye(K, dtype=np.float32), W, None, narrow=True, planes=planes)
    got = _np(Cm)[:, :J].T.copy()
    diff = got.view(np.int32) != want.view(np.int32)
    assert not diff.any(), (int(diff.sum()), np.argwhere(diff)[:8].tolist())


# ---------------------------------------------------------------------------------------------------------------------------------
# c. K-contiguous GEMM, fp32 output
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("planes", [2, 1])
@pytest.mark.parametrize("I,K", [(129, 32), (300, 512), (257, 528)])
def test_kc_narrow_fp32_output_elementwise(I, K, planes):
    """|got - exact| <= acc_bound(K, mag); with the bias one more term (the epilogue adds it in fp32: K + 1, mag + |b|).  The quiet
    rows (x 1e-5) have their own exponents, so the bound is as tight for them as for the loud ones."""
    g = torch.Generator().manual_seed(I)
    A = _randn(g, I, K).copy()
    A[:100] *= np.float32(1e-5)
    W = (_randn(g, 9, K) * np.float32(0.1)).astype(np.float32)
    b = _randn(g, 9)
    ex, mag = _exact_kc(A, W, planes)
    C0 = _np(_kc(A, W, None, narrow=True, planes=planes)[0])[:, :9].astype(np.float64)
    r0 = np.abs(C0 - ex) / N.acc_bound(K, mag)
    _record(f"narrow I{I} K{K} planes{planes}", r0.max())
    Cb = _np(_kc(A, W, b, narrow=True, planes=planes)[0])[:, :9].astype(np.float64)
    rb = np.abs(Cb - (ex + b)) / N.acc_bound(K + 1, mag + np.abs(b))
    _record(f"narrow+bias I{I} K{K} planes{planes}", rb.max())
    assert r0.max() <= 1.0 and rb.max() <= 1.0, (float(r0.max()), float(rb.max()))


# ---------------------------------------------------------------------------------------------------------------------------------
# d. K-contiguous GEMM, plane output
# ---------------------------------------------------------------------------------------------------------------------------------
def _check_planes(case, got, exact, delta, planes, **kw):
    res = N.on_grid_near(_np(got), exact, delta, planes, **kw)
    _record(case, res["ratio"])
    assert res["ok"], (case, res)


def _check_colsum(case, cs, exact, bound, I):
    """per 128-row tile: |cs - sum_rows exact| <= sum_rows acc_bound + 128 u sum_rows |exact| (the sums run over the kernel's
    fp32 values, which lie within acc_bound of exact; 128 fp32 adds in any order)"""
    cs = _np(cs).astype(np.float64)
    worst = 0.0
    for t, r in enumerate(range(0, I, 128)):
        bar = bound[r:r + 128].sum(0) + 128 * N.U * np.abs(exact[r:r + 128]).sum(0)
        worst = max(worst, float((np.abs(cs[t] - exact[r:r + 128].sum(0)) / bar).max()))
    _record(case, worst)
    assert worst <= 1.0, (case, worst)


@functools.lru_cache(maxsize=None)
def _plain_case(I, J, K, planes):
    g = torch.Generator().manual_seed(I + J + K)
    A = _randn(g, I, K)
    W = (_randn(g, J, K) * np.float32(0.05)).astype(np.float32)
    b = _randn(g, J)
    return (A, W, b) + _exact_kc(A, W, planes)


@pytest.mark.parametrize("planes", [2, 1])
@pytest.mark.parametrize("I,J,K", [(128, 256, 16), (300, 512, 512), (257, 48, 64), (1000, 544, 528), (300, 256, 32)])
def test_kc_plane_output_plain_bias_colsum(I, J, K, planes, kc_grid):
    A, W, b, ex, mag = _plain_case(I, J, K, planes)
    case = f"kc I{I} J{J} K{K} planes{planes} grid{kc_grid}"
    Cb, _, _ = _kc(A, W, b, planes=planes)                             # forward launches carry the bias ...
    _check_planes(case + " bias", Cb, ex + b, N.acc_bound(K + 1, mag + np.abs(b)), planes)
    C0, _, cs = _kc(A, W, None, want_colsum=True, planes=planes)       # ... backward launches the column sums
    _check_planes(case + " plain", C0, ex, N.acc_bound(K, mag), planes)
    _check_colsum(case + " colsum", cs, ex, N.acc_bound(K, mag), I)


@functools.lru_cache(maxsize=None)
def _two_segment_case(planes):
    """the inputs of test_kc_two_segments_offsets_and_exponent_changes (tests/test_gpu_bsp.py; its one-plane sibling takes Kb = 288):
    A blocks 2^-20 / 2^9 apart along k and down the rows, a second segment quantised on its own"""
    g = torch.Generator().manual_seed(7)
    I, Ka, Kb, J = 384, 256, 272 if planes == 2 else 288, 512
    A = _randn(g, I, Ka).copy()
    A[:, 128:] *= np.float32(2.0 ** -20)
    A[128:256] *= np.float32(2.0 ** 9)
    A2 = (_randn(g, I, Kb) * np.float32(37.0)).astype(np.float32)
    W = _randn(g, J, Ka + Kb)
    Wz = W.copy()
    Wz[:, :128] = 0
    Wz[:, Ka:] = 0
    W1 = W[:, :Ka].copy()
    return {"A": A, "A2": A2, "W": W, "Wz": Wz, "W1": W1, "K": Ka + Kb, "Ka": Ka,
            "both": _exact_kc(A, W, planes, A2), "first": _exact_kc(A, W1, planes), "zero": _exact_kc(A, Wz, planes, A2)}


@pytest.mark.parametrize("planes", [2, 1])
def test_kc_plane_output_two_segments_offsets_exponent_changes(planes, kc_grid):
    c = _two_segment_case(planes)
    case = f"kc two segments planes{planes} grid{kc_grid}"
    for name, A2, W, K, kw in (("both", c["A2"], c["W"], c["K"], dict(a_col0=128, c_col0=256)),        # loud, quiet, loud: two rescales
                               ("first", None, c["W1"], c["Ka"], dict(a_col0=128)),                  # ends on the quiet block
                               ("zero", c["A2"], c["Wz"], c["K"], dict(a_col0=128, c_col0=128))):    # the quiet block alone decides
        ex, mag = c[name]
        Cm, _, _ = _kc(c["A"], W, None, A2=A2, planes=planes, **kw)
        _check_planes(f"{case} {name}", Cm, ex, N.acc_bound(K, mag), planes)
    assert float(np.abs(c["zero"][0]).max()) < 2.0 ** -10 * float(np.abs(c["both"][0]).max())          # (it IS the quiet block's scale)


# ---------------------------------------------------------------------------------------------------------------------------------
# e. SIREN forward and its folded projections;  f. derivative epilogues
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _siren_case(I, J, K, w0, planes):
    g = torch.Generator().manual_seed(I + K)
    X = (torch.rand(I, K, generator=g) * 2 - 1).numpy()
    W = (_randn(g, J, K) * np.float32(0.3 / K ** 0.5)).astype(np.float32)
    b = (_randn(g, J) * np.float32(0.1)).astype(np.float32)
    ex, mag = _exact_kc(X, W, planes)
    z = w0 * (ex + b)
    h = np.sin(z)
    # the argument's error times w0, plus the sine epilogue's own bar (SIN_BAR: from the existing two-plane test)
    dh = w0 * N.acc_bound(K + 1, mag + np.abs(b)) + SIN_BAR * max(1.0, w0 / 8)
    Kg = 256
    G = _randn(g, I, Kg).copy()
    G[:128] *= np.float32(1e-7)                                          # a quiet block of gradient rows
    W2 = (_randn(g, J, Kg) * np.float32(0.05)).astype(np.float32)
    nd_w = _randn(g, 9, J)
    return {"X": X, "W": W, "b": b, "z": z, "h": h, "dh": dh, "G": G, "W2": W2, "gw": _exact_kc(G, W2, planes), "Kg": Kg, "nd_w": nd_w}


def _cos_sign(sign, I, J, ldc, c_col0):
    """+1 / -1 from the sign words (bsp.h: sign_words; bsp_kc.hip: the sine epilogue): word (32-row block, 64-column group, lane =
    row % 32 + 32 ((col >> 3) & 1)), bit 8 ((col >> 4) & 3) + (col & 7) set where cos < 0"""
    w = _np(sign).astype(np.uint32).reshape(-1, (ldc + 63) // 64, 64)
    rows, cols = np.arange(I)[:, None], np.arange(J)[None, :]
    lane = rows % 32 + 32 * ((cols >> 3) & 1)
    bit = (8 * ((cols >> 4) & 3) + (cols & 7)).astype(np.uint32)
    return 1.0 - 2.0 * ((w[rows // 32, (c_col0 + cols) // 64, lane] >> bit) & 1).astype(np.float64)


@pytest.mark.parametrize("planes", [2, 1])
@pytest.mark.parametrize("I,J,K,w0", [(300, 512, 64, 30.0), (300, 512, 512, 1.0)])
def test_siren_forward_then_derivative_epilogue(I, J, K, w0, planes, kc_grid):
    """Forward: H on the grid of the constant exponent 13 (the sine epilogue writes no block maximum), near sin(w0 (exact + b)).
    Backward: (G W2^T) w0 cos rebuilt from the STORED H and the sign words, against (exact product) w0 s sqrt(1 - H^2) with the H and
    s the forward launch returned.  H is on its grid, so the hook's re-quantisation of it is the identity (asserted through the
    round-trip hook).  Bound: w0 |cos| acc_bound + SINREC_REL |ref| (derived at SINREC_REL).  Elements with |cos(w0 z)| < 2^-10, z from
    the reference alone, are left out of the nearness check: at most 1 % of a case (uniform phases: ~0.06 %)."""
    c = _siren_case(I, J, K, w0, planes)
    case = f"siren I{I} J{J} K{K} w0 {w0:g} planes{planes} grid{kc_grid}"
    H, sign, _ = _kc(c["X"], c["W"], c["b"], act=ACT_SIN, w0=w0, want_sign=True, c_col0=128, planes=planes)
    _check_planes(case + " H", H, c["h"], c["dh"], planes, e_fixed=13)
    ldc = 128 + J
    Hrt, _ = _roundtrip(H, ldc, 128, planes)
    assert torch.equal(Hrt, H), "the stored activation is not a fixed point of the plane conversion"
    Hn = _np(H).astype(np.float64)
    s = _cos_sign(sign, I, J, ldc, 128)
    clear = np.abs(np.cos(c["z"])) > 2.0 * c["dh"]            # a phase error of dh cannot move cos across zero there
    assert clear.mean() > 0.99 and np.array_equal(s[clear], np.sign(np.cos(c["z"]))[clear])
    D, _, cs = _kc(c["G"], c["W2"], None, aux=AUX_SINREC, Hact=H, Hsign=sign, w0=w0, want_colsum=True, c_col0=128, planes=planes)
    gw, gmag = c["gw"]
    cosr = np.sqrt(np.clip(1.0 - Hn * Hn, 0.0, None))
    ref = gw * (w0 * s * cosr)
    delta = w0 * cosr * N.acc_bound(c["Kg"], gmag) + SINREC_REL * np.abs(ref)
    skip = np.abs(np.cos(c["z"])) < 2.0 ** -10                # from the reference alone (tests/test_bsp_exact_cpu.py bounds the share)
    assert float(skip.mean()) <= 0.01, float(skip.mean())
    _check_planes(case + " D", D, ref, delta, planes, skip=skip)
    # column sums of the values before they are rounded to planes (one more rounding: the uniform factor is applied to the sum)
    _check_colsum(case + " D colsum", cs, ref, delta + N.U * np.abs(ref), I)


@pytest.mark.parametrize("planes", [2, 1])
def test_siren_forward_with_folded_projections(planes, kc_grid):
    """The projections ride on the fp32 sine values BEFORE they are rounded to planes: per wave (64 columns) and point,
    |part - sum_j h_ij w_j| <= sum_j dh_ij |w_j| + acc_bound(64, sum_j |h_ij w_j|) -- an fp32-class bar for both plane counts.  The
    single-row form at J = 512, the nd_rows = (3, 5, 1, 0) form at K = 528; the layer's own output is unchanged by them."""
    for (I, J, K, w0), rows in (((300, 512, 512, 1.0), None), ((300, 1024, 528, 1.0), (3, 5, 1, 0))):
        c = _siren_case(I, J, K, w0, planes)
        case = f"projections J{J} K{K} planes{planes} grid{kc_grid}"
        nw = c["nd_w"][:1].reshape(J).copy() if rows is None else c["nd_w"][:sum(rows)].copy()
        H0, s0, _ = _kc(c["X"], c["W"], c["b"], act=ACT_SIN, w0=w0, want_sign=True, planes=planes)
        H1, s1, parts = _kc(c["X"], c["W"], c["b"], act=ACT_SIN, w0=w0, want_sign=True, planes=planes, nd_w=nw, nd_rows=rows)
        assert torch.equal(H0, H1) and torch.equal(s0, s1)
        _check_planes(case + " H", H1, c["h"], c["dh"], planes, e_fixed=13)
        parts = _np(parts).astype(np.float64)
        h, dh, worst = c["h"], np.broadcast_to(c["dh"], c["h"].shape), 0.0
        if rows is None:
            assert parts.shape == ((J // 256) * 4, I)
            jobs = [(q, nw, 64 * q) for q in range(parts.shape[0])]
            get = lambda q: parts[q]
        else:
            parts = parts.reshape(len(rows), 4, 5, I)
            jobs, r0 = [], 0
            for tj, n in enumerate(rows):
                assert np.isnan(parts[tj, :, n:]).all(), "a slot beyond the tile's projections was written"
                jobs += [((tj, w, o), nw[r0 + o], 256 * tj + 64 * w) for o in range(n) for w in range(4)]
                r0 += n
            get = lambda q: parts[q[0], q[1], q[2]]
        for q, wrow, c0 in jobs:
            wv = wrow[c0:c0 + 64].astype(np.float64)
            want = h[:, c0:c0 + 64] @ wv
            bar = dh[:, c0:c0 + 64] @ np.abs(wv) + N.acc_bound(64, np.abs(h[:, c0:c0 + 64]) @ np.abs(wv))
            worst = max(worst, float((np.abs(get(q) - want) / bar).max()))
        _record(case + " partials", worst)
        assert worst <= 1.0, (case, worst)


@pytest.mark.parametrize("planes", [2, 1])
def test_relu_forward_and_mask(planes, kc_grid):
    """The mask is taken from the STORED activation (h > 0 <=> its hi plane > 0), so with the H the forward launch returned it is
    exact everywhere: D near (exact product of G and W2) [H > 0].  H itself is positive exactly where the exact pre-activation is,
    wherever that exceeds its acc_bound (+ 2^-36 of the block's maximum: what rounds to zero on the plane grid)."""
    I, J, K = 520, 256, 96
    g = torch.Generator().manual_seed(11)
    X, W = _randn(g, I, K), _randn(g, J, K)
    G = _randn(g, I, 64).copy()
    G[:128] *= np.float32(1e-7)
    W2 = _randn(g, J, 64)
    case = f"relu planes{planes} grid{kc_grid}"
    ex, mag = _exact_kc(X, W, planes)
    H, _, _ = _kc(X, W, None, act=ACT_RELU, planes=planes)
    _check_planes(case + " H", H, np.maximum(ex, 0.0), N.acc_bound(K, mag), planes)
    assert torch.equal(_roundtrip(H, J, 0, planes)[0], H)
    on = _np(H) > 0
    sure = np.abs(ex) > N.acc_bound(K, mag) + 2.0 ** -36 * np.abs(ex).max()
    assert sure.mean() > 0.99 and np.array_equal(on[sure], (ex > 0)[sure])
    gw, gmag = _exact_kc(G, W2, planes)
    D, _, _ = _kc(G, W2, None, aux=AUX_RELU_MASK, Hact=H, planes=planes)
    _check_planes(case + " D", D, gw * on, N.acc_bound(64, gmag) * on, planes)


# ---------------------------------------------------------------------------------------------------------------------------------
# g. weight-gradient GEMM
# ---------------------------------------------------------------------------------------------------------------------------------
def _dw(A, B, I, J, a_col0=0, b_col0=0, k_split=1024, narrow=False, planes=2):
    L, lib = _lib()
    A, B = _dev(A), _dev(B)
    Cm = torch.full((I, J), float("nan"), device=DEV)
    lib.check(L.snerf_test_bsp_dw(_p(A), A.shape[1], _p(B), B.shape[1], A.shape[0], I, J, a_col0, b_col0, k_split, int(narrow), _p(Cm), planes, _st()),
              "test_bsp_dw")
    return _np(Cm).astype(np.float64)


def _check_dw(case, A, B, I, J, planes, a_col0=0, b_col0=0, k_split=1024, narrow=False):
    """|got - exact| <= acc_bound(P + n_slabs, mag) (+ what the dropped-chunk rule can remove: bsp_numpy.dw_drop_bound): the
    slabs are fp32 sums over the points and are then added in fp32.  The source matrices are quantised whole, blocks anchored at
    their column 0, and THEN sliced (b_col0 = 192 is no block boundary)."""
    P = A.shape[0]
    ha, la, ea = N.to_planes(A, planes)
    hb, lb, eb = N.to_planes(B, planes)
    ah, al = N.deq(ha, la, N.expand(ea, *A.shape))
    bh, bl = N.deq(hb, lb, N.expand(eb, *B.shape))
    sa, sb = slice(a_col0, a_col0 + I), slice(b_col0, b_col0 + J)
    ex, mag = N.exact_product(ah[:, sa].T.copy(), al[:, sa].T.copy(), bh[:, sb], bl[:, sb], planes)
    n_slabs = (P + k_split - 1) // k_split
    bound = N.acc_bound(P + n_slabs, mag)
    for i0 in range(0, I, 128):
        for j0 in range(0, J, 64):
            ca, cb = (a_col0 + i0) >> 7, (b_col0 + j0) >> 7
            lost = sum(N.dw_drop_bound((ea[:, ca] + eb[:, cb])[k >> 7: (min(P, k + k_split) + 127) >> 7]) for k in range(0, P, k_split))
            bound[i0:i0 + 128, j0:j0 + 64] += lost
    got = _dw(A, B, I, J, a_col0, b_col0, k_split, narrow, planes)
    ratio = float((np.abs(got - ex) / bound).max())
    _record(case, ratio)
    assert ratio <= 1.0, (case, ratio)


@pytest.mark.parametrize("planes", [2, 1])
@pytest.mark.parametrize("P,I,J,ks", [(650, 256, 64, 128), (2048, 256, 256, 1024), (1000, 256, 256, 1024), (5000, 512, 544, 1024)])
def test_dw_elementwise(P, I, J, ks, planes):
    g = torch.Generator().manual_seed(P + I)
    A, B = _randn(g, P, I), _randn(g, P, J)
    scale = np.ones(P, np.float32)          # heavy tail along the contraction axis: blocks of points 2^18 / 2^24 apart
    scale[: P // 3] = 2.0 ** -18
    scale[P // 3: P // 2] = 2.0 ** 6
    _check_dw(f"dw P{P} I{I} J{J} ks{ks} planes{planes}", A * scale[:, None], B, I, J, planes, k_split=ks)


@pytest.mark.parametrize("planes", [2, 1])
def test_dw_column_offsets_and_narrow_elementwise(planes):
    g = torch.Generator().manual_seed(3)
    P = 3000
    A, B = _randn(g, P, 384), _randn(g, P, 448)
    _check_dw(f"dw offsets planes{planes}", A, B, 256, 320, planes, a_col0=128, b_col0=128)
    An = _randn(g, P, 32).copy()
    An[:1000] *= np.float32(1e-6)
    _check_dw(f"dw narrow I32 J448 planes{planes}", An, B, 32, 448, planes, narrow=True)
    _check_dw(f"dw narrow I9 J200 b_col0 192 planes{planes}", An, B, 9, 200, planes, b_col0=192, narrow=True)
