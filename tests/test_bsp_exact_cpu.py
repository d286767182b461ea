"""The restatement of the plane format (tests/bsp_numpy.py) and the element-wise bars of tests/test_gpu_bsp_exact.py, on the CPU.

Two questions are answered without a GPU: is the restatement the format the headers describe (properties below; the GPU module
then holds it to the library bit for bit), and do the bars see what they are meant to see.  For the second a stand-in "kernel" --
the restatement with fp32 accumulation in 16-wide k-steps -- must meet every bar, and the same stand-in with one planted defect
must fail them.  VERDICTS records, without asserting it, which of the defects the norm yardsticks of tests/test_gpu_bsp.py accept
(formulas copied from there); it is the source of the table in DESIGN.md (printed with -s)."""
import numpy as np
import pytest
import torch

from tests import bsp_numpy as N
from tests.test_gpu_bsp_exact import SINREC_REL, _qa, _roundtrip_input, _siren_case     # recipes and constants: no GPU at import

VERDICTS = []     # (case, defect, today's normwise error, today's bar, today's verdict, worst error / new bound)


def _blocks(R, Cn):
    return [(rb, cb, (slice(128 * rb, 128 * rb + 128), slice(128 * cb, 128 * cb + 128))) for rb in range((R + 127) // 128) for cb in range((Cn + 127) // 128)]


def _heavy(seed=0):
    x = torch.randn(300, 200, generator=torch.Generator().manual_seed(seed)).numpy().copy()
    x[:128] *= np.float32(1e-6)
    x[128:256, :128] *= np.float32(3e3)
    return x


# ---- the format -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("planes", [1, 2])
def test_reconstruction_and_block_exponents(planes):
    x = _heavy()
    hi, lo, e = N.to_planes(x, planes)
    y = N.from_planes(hi, lo, N.expand(e, *x.shape)).astype(np.float64)
    for rb, cb, sl in _blocks(*x.shape):
        m = float(np.abs(x[sl]).max())
        assert 2.0 ** 13 <= m * 2.0 ** int(e[rb, cb]) < 2.0 ** 14
        assert np.abs(y[sl] - x[sl]).max() <= m * (2.0 ** -11 if planes == 1 else 2.0 ** -22)
    if planes == 1:
        assert not lo.any()


@pytest.mark.parametrize("planes", [1, 2])
def test_requantising_is_the_identity(planes):
    x = _heavy(1)
    hi, lo, e = N.to_planes(x, planes)
    assert np.abs(hi).max() < 2.0 ** 14                    # (no block maximum rounds up to the next binade: see the edge test)
    y = N.from_planes(hi, lo, N.expand(e, *x.shape))
    hi2, lo2, e2 = N.to_planes(y, planes)
    y2 = N.from_planes(hi2, lo2, N.expand(e2, *x.shape))
    assert np.array_equal(e, e2) and np.array_equal(hi + lo, hi2 + lo2) and np.array_equal(y.view(np.int32), y2.view(np.int32))
    # a SIREN output is written under the constant exponent 13; the conversion picks 14 where the block's |max| < 1: the same values
    h = np.sin(np.linspace(-0.7, 0.7, 128 * 128)).reshape(128, 128)
    hh, hl = N.split(np.ldexp(h, 13), planes)
    stored = N.from_planes(hh, hl, 13)
    h2, l2, e14 = N.to_planes(stored, planes)
    assert e14[0, 0] == 14 and np.array_equal(N.from_planes(h2, l2, 14), stored)


@pytest.mark.parametrize("planes", [1, 2])
def test_clamps_and_edge_values(planes):
    x = _roundtrip_input()
    hi, lo, e = N.to_planes(x, planes)
    assert e[0].tolist() == [N.exp_of_max(np.abs(x[:128, :128]).max()), 0] and e[1:].tolist() == [[-1, 13], [N.E_QUIET, -N.E_MAX]]
    assert N.exp_of_max(0.0) == 0 and N.exp_of_max(-0.0) == 0 and N.exp_of_max(np.inf) == 0 and N.exp_of_max(np.nan) == 0
    assert N.exp_of_max(2.0 ** -47) == 60 and N.exp_of_max(2.0 ** -46) == 59 and N.exp_of_max(2.0 ** 113) == -100 and N.exp_of_max(2.0 ** 120) == -100
    assert not hi[:128, 128:].any() and not lo[:128, 128:].any()                       # the all-zero block (with its -0)
    assert np.signbit(hi[5, 7]) and np.signbit(hi[3, 130])                             # -0 keeps its sign on the plane ...
    y = N.from_planes(hi, lo, N.expand(e, *x.shape))
    assert y[5, 7] == 0 and not np.signbit(y[5, 7])                                    # ... and loses it in the fp32 sum hi + lo
    assert hi[200, 64] == 2.0 ** 13 and y[200, 64] == 2.0 ** 14                        # |max| an exact power of two
    assert hi[128, 128] == 2.0 ** 14 and (planes == 1 or lo[128, 128] == -2.0 ** -5)   # rounds up to 2^14; lo takes it back
    assert hi[129, 129] == 1026 and hi[129, 130] == 1026                               # ties to even, either side
    assert hi[130, 129] == 6 * 2.0 ** -24 and hi[130, 130] == 0 and hi[130, 131] == -6 * 2.0 ** -24 and hi[130, 132] == 2.0 ** -14   # fp16 subnormals
    assert hi[130, 133] == 3 * 2.0 ** -24
    assert np.isfinite(hi).all() and np.abs(hi[256:, 128:]).max() == 1.5 * 2.0 ** 15     # beyond the loud clamp: above 2^14, still fp16
    q = np.abs(hi[256:, :128])
    assert q.max() < 2.0 ** 13 and (q[q > 0] < 2.0 ** -14).any()                         # beyond the quiet clamp: bits lost, subnormals
    # re-quantising the block whose maximum rounded up moves its exponent to 12; every value stays within half a grid spacing
    blk = (slice(128, 256), slice(128, 200))
    h2, l2, e2 = N.to_planes(y[blk], planes)
    # (one plane; with two, lo takes the round-up back, the exponent stays and the conversion is the identity)
    assert int(e2[0, 0]) == (12 if planes == 1 else 13)
    y2 = N.from_planes(h2, l2, int(e2[0, 0])).astype(np.float64)
    sp = np.ldexp(N.grid_spacing(np.ldexp(np.abs(y[blk].astype(np.float64)), 12), planes), -12)
    assert (np.abs(y2 - y[blk]) <= 0.5 * sp).all() and (planes == 1) == bool((y2 != y[blk]).any())


def test_weight_planes_have_one_exponent():
    g = torch.Generator().manual_seed(2)
    w = (torch.randn(40, 300, generator=g) * 0.05).numpy()
    w[17, 250] = 3.0
    hi, lo, e = N.weight_planes(w, 2)
    assert e == 12 and np.abs(N.from_planes(hi, lo, e).astype(np.float64) - w).max() <= 3.0 * 2.0 ** -22
    h1, l1, e1 = N.weight_planes(w, 1)
    assert e1 == 12 and not l1.any() and np.array_equal(h1, hi)


def test_grid_helpers():
    assert N.ulp16(1.0) == 2.0 ** -10 and N.ulp16(2.0 ** -14) == 2.0 ** -24 and N.ulp16(2.0 ** -20) == 2.0 ** -24 and N.ulp16(8191.0) == 4.0
    assert N.grid_spacing(8192.0, 1) == 8.0 and N.grid_spacing(8192.0, 2) == 2.0 ** -8
    assert N.dw_drop_bound([10, 74, 10]) == 0.0                                          # 64 above the frame is kept
    lost = N.dw_drop_bound([10, 80, 12, 77, 200])                                         # 80 dropped, frame 12, 77 and 200 dropped
    assert lost == 128.0 * (2.0 ** (29 - 80) + 2.0 ** (29 - 77) + 2.0 ** (29 - 200))
    x = np.zeros((128, 128))
    x[0, 0], x[1, 1] = 1.0, 0.3
    g = N.from_planes(*N.split(np.ldexp(x, 13), 1), 13).astype(np.float64)
    assert N.on_grid_near(g, x, 0.0, 1)["ok"]
    g[1, 1] += 2.0 ** -12                                  # one grid point further: still on the grid, no longer nearest
    r = N.on_grid_near(g, x, 0.0, 1)
    assert r["bad_grid"] == 0 and r["bad_near"] == 1
    g[1, 1] += 2.0 ** -20                                  # off the grid
    assert N.on_grid_near(g, x, 1.0, 1)["bad_grid"] == 1


# ---- the bars' reach: a stand-in kernel, honest and with planted defects ------------------------------------------------------------
def _acc32(ah, al, bh, bl, planes, step=16):
    """fp32 accumulation of [M][K] x [K][N] in 16-wide k-steps, the products in the kernels' order (hi lo, lo hi, hi hi)"""
    ah, al, bh, bl = (np.ascontiguousarray(v, np.float32) for v in (ah, al, bh, bl))
    acc = np.zeros((ah.shape[0], bh.shape[1]), np.float32)
    for s in range(0, ah.shape[1], step):
        k = slice(s, s + step)
        if planes == 2:
            acc += ah[:, k] @ bl[k]
            acc += al[:, k] @ bh[k]
        acc += ah[:, k] @ bh[k]
    return acc


def _as_planes(v, planes):
    hi, lo, e = N.to_planes(v.astype(np.float32), planes)
    return N.from_planes(hi, lo, N.expand(e, *v.shape)).astype(np.float64)


def _relerr(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _kc_operands(I, J, K, planes, coherent=False):
    """random operands (the recipe of the GPU cases); coherent: A > 0 and every W entry (8192 + 8 r + 3.9) 2^-13 / 16, r a random
    integer -- lo = 3.9 under the matrix's exponent for every entry, so the hi lo products of a sum all have one sign"""
    g = torch.Generator().manual_seed(I + J + K)
    A = torch.randn(I, K, generator=g).numpy().copy()
    if K > 512:
        A[:, 512:] *= np.float32(0.25)           # the ragged last k-block gets an exponent of its own
    W = (torch.randn(J, K, generator=g) * 0.05).numpy()
    if coherent:
        A = np.abs(A)
        W = ((8192.0 + 8.0 * torch.randint(0, 1000, (J, K), generator=g).numpy() + 3.9) * 2.0 ** -17).astype(np.float32)
    ha, la, ea = N.to_planes(A, planes)
    ah, al = N.deq(ha, la, N.expand(ea, I, K))
    hw, lw, ew = N.weight_planes(W, planes)
    wh, wl = N.deq(hw, lw, ew)
    return A, W, ea, ah, al, wh.T.copy(), wl.T.copy()


KC_DEFECTS = ["none", "edge row x (1 + 2^-9)", "one k index dropped in a 32 x 32 block", "one 16-wide k-step dropped in a 32 x 32 block",
              "hi lo term left out in a 128 x 128 tile", "neighbour's exponent on the ragged last k-block"]


def _kc_standin(op, planes, defect):
    A, W, ea, ah, al, bh, bl = op
    I, K = ah.shape
    if defect == KC_DEFECTS[5]:
        if K <= 512:
            return None
        assert (ea[:, 4] != ea[:, 3]).all()
        f = np.ldexp(1.0, N.expand(ea, I, K)[:, 512:] - N.expand(ea, I, K)[:, 511:512])     # dequantised under block 3's exponent
        ah, al = ah.copy(), al.copy()
        ah[:, 512:] *= f
        al[:, 512:] *= f
    v = _acc32(ah, al, bh, bl, planes).astype(np.float64)
    a, b = ah + al, bh + bl
    blk = (slice(160, 192), slice(64, 96))
    if defect == KC_DEFECTS[1]:
        v[127] *= 1.0 + 2.0 ** -9
    elif defect == KC_DEFECTS[2]:
        v[blk] -= np.outer(a[blk[0], 37], b[37, blk[1]])
    elif defect == KC_DEFECTS[3]:
        v[blk] -= a[blk[0], 32:48] @ b[32:48, blk[1]]
    elif defect == KC_DEFECTS[4]:
        if planes == 1:
            return None
        v[128:256, 128:256] -= (ah @ bl)[128:256, 128:256]
    return v.astype(np.float32).astype(np.float64)


@pytest.mark.parametrize("planes", [1, 2])
@pytest.mark.parametrize("I,J,K", [(300, 512, 512), (1000, 544, 528)])
def test_standin_meets_the_bars_and_every_defect_fails_them(I, J, K, planes):
    op = _kc_operands(I, J, K, planes)
    A, W = op[0].astype(np.float64), op[1].astype(np.float64)
    ex, mag = N.exact_product(*op[3:], planes)
    bound = N.acc_bound(K, mag)
    # today's yardsticks (tests/test_gpu_bsp.py: test_kc_plain_and_bias / test_one_plane_kc_plain_bias_colsum), against the unrounded product
    ref = A @ W.T
    if planes == 2:
        today_bar = max(2.0 * _relerr((op[0] @ op[1].T).astype(np.float64), ref), 2e-7)
    else:
        today_bar = 2.0 * _relerr(op[0].astype(np.float16).astype(np.float64) @ op[1].astype(np.float16).astype(np.float64).T, ref) + 2.0 ** -11
    for defect in KC_DEFECTS:
        v = _kc_standin(op, planes, defect)
        if v is None:
            continue
        r32 = float((np.abs(v - ex) / bound).max())                    # fp32 output
        got = _as_planes(v, planes)                                    # plane output
        rp = N.on_grid_near(got, ex, bound, planes)
        today = _relerr(got, ref)
        VERDICTS.append((f"kc {I}x{J}x{K} planes {planes}", defect, today, today_bar, "pass" if today <= today_bar else "fail", r32, rp["ratio"]))
        print("%-24s %-50s today %.2e / %.2e %s   new: fp32 out %.3g, plane out %.3g" % VERDICTS[-1])
        if defect == "none":
            assert r32 <= 1.0 and rp["ok"], (r32, rp)
        elif defect != KC_DEFECTS[4]:
            assert r32 > 1.0 and not rp["ok"] and rp["bad_grid"] == 0, (defect, r32, rp)
    if planes == 2:
        # The lost hi lo term on RANDOM operands is recorded above, not asserted: it grows as sqrt(K) 2^-12, the worst-case bound as
        # K^2 2^-23 (mag ~ K), and at these K the two meet -- 1.0 ... 1.2 of the bound at K = 512, 0.93 at K = 528; the bars reach it
        # below K ~ 300 only.  It is asserted where the low planes are coherent and the lost term grows as K: lo / hi between 2^-12 and
        # 2^-11 for every entry, so 2^11 / (K + 2) ... 2^12 / (K + 2) = 4 ... 8 times the bound (5.3 here).
        opc = _kc_operands(I, J, K, planes, coherent=True)
        exc, magc = N.exact_product(*opc[3:], planes)
        for defect in (KC_DEFECTS[0], KC_DEFECTS[4]):
            v = _kc_standin(opc, planes, defect)
            r32 = float((np.abs(v - exc) / N.acc_bound(K, magc)).max())
            rp = N.on_grid_near(_as_planes(v, planes), exc, N.acc_bound(K, magc), planes)
            VERDICTS.append((f"kc {I}x{J}x{K} planes {planes}", defect + ", coherent lo", float("nan"), float("nan"), "-", r32, rp["ratio"]))
            print("%-24s %-50s today %.2e / %.2e %s   new: fp32 out %.3g, plane out %.3g" % VERDICTS[-1])
            assert (r32 <= 1.0 and rp["ok"]) if defect == "none" else (r32 > 1.0 and not rp["ok"] and rp["bad_grid"] == 0), (defect, r32, rp)


@pytest.mark.parametrize("planes", [1, 2])
def test_standin_with_bias_and_an_off_grid_output(planes):
    I, J, K = 300, 512, 512
    op = _kc_operands(I, J, K, planes)
    ex, mag = N.exact_product(*op[3:], planes)
    b = torch.randn(J, generator=torch.Generator().manual_seed(5)).numpy()
    v = (_acc32(*op[3:], planes) + b).astype(np.float64)
    bound = N.acc_bound(K + 1, mag + np.abs(b))
    assert (np.abs(v - (ex + b)) <= bound).all()
    got = _as_planes(v, planes)
    assert N.on_grid_near(got, ex + b, bound, planes)["ok"]
    e = N.exp_of_max(np.abs((ex + b)[:128, 256:384]).max())
    v73 = np.ldexp(got[7, 300], e)
    r = v73 - float(np.float16(v73))
    got[7, 300] += np.ldexp(0.25 * N.ulp16(v73 if planes == 1 else r), -e)       # a quarter step of the finest plane: no plane pair holds it
    r = N.on_grid_near(got, ex + b, bound, planes)
    assert not r["ok"] and r["bad_grid"] == 1


@pytest.mark.parametrize("planes", [1, 2])
def test_dw_standin_meets_the_bar_and_a_lost_chunk_fails_it(planes):
    """split-K slabs of 1024 points, fp32 inside a slab and across slabs; the planted defect leaves one 128-point chunk (points 768 ..
    895, in the loud third of the contraction) out of slab 0 for one 256 x 256 tile"""
    P, I, J, ks = 2048, 256, 256, 1024
    g = torch.Generator().manual_seed(P + I)
    A, B = torch.randn(P, I, generator=g).numpy(), torch.randn(P, J, generator=g).numpy()
    scale = np.ones(P, np.float32)
    scale[: P // 3] = 2.0 ** -18
    scale[P // 3: P // 2] = 2.0 ** 6
    A = A * scale[:, None]
    ha, la, ea = N.to_planes(A, planes)
    hb, lb, eb = N.to_planes(B, planes)
    ah, al = N.deq(ha, la, N.expand(ea, P, I))
    bh, bl = N.deq(hb, lb, N.expand(eb, P, J))
    ex, mag = N.exact_product(ah.T.copy(), al.T.copy(), bh, bl, planes)
    bound = N.acc_bound(P + 2, mag)
    assert all(N.dw_drop_bound(ea[k >> 7: (k + ks) >> 7, ca] + eb[k >> 7: (k + ks) >> 7, cb]) == 0.0 for k in (0, ks) for ca in range(2) for cb in range(2))
    ref = A.astype(np.float64).T @ B.astype(np.float64)
    if planes == 2:
        today_bar = max(2.0 * _relerr((A.T @ B).astype(np.float64), ref), 3e-7)
    else:
        today_bar = 2.0 * _relerr(A.astype(np.float16).astype(np.float64).T @ B.astype(np.float16).astype(np.float64), ref) + 1e-6
    for defect in ("none", "one 128-point chunk of a slab left out"):
        slabs = []
        for k in range(0, P, ks):
            keep = np.ones(P, bool)
            if defect != "none" and k == 0:
                keep[768:896] = False
            s = np.arange(k, k + ks)[keep[k:k + ks]]
            slabs.append(_acc32(ah[s].T, al[s].T, bh[s], bl[s], planes))
        got = (slabs[0] + slabs[1]).astype(np.float64)
        ratio = float((np.abs(got - ex) / bound).max())
        today = _relerr(got, ref)
        VERDICTS.append((f"dW {P}x{I}x{J} planes {planes}", defect, today, today_bar, "pass" if today <= today_bar else "fail", ratio, float("nan")))
        print("%-24s %-50s today %.2e / %.2e %s   new: fp32 out %.3g, plane out %.3g" % VERDICTS[-1])
        assert (ratio <= 1.0) == (defect == "none"), (defect, ratio)


@pytest.mark.parametrize("planes", [1, 2])
@pytest.mark.parametrize("I,J,K,w0", [(300, 512, 64, 30.0), (300, 512, 512, 1.0)])
def test_derivative_cases_leave_out_less_than_one_percent(I, J, K, w0, planes):
    """the derivative-epilogue cases of the GPU module leave out elements with |cos(w0 z)| < 2^-10, z from the reference alone:
    at most 1 % of a case (uniform phases: 2 / pi 2^-10 = 0.06 %)"""
    c = _siren_case(I, J, K, w0, planes)
    share = float((np.abs(np.cos(c["z"])) < 2.0 ** -10).mean())
    print(f"left out: {100 * share:.3f} % at w0 = {w0:g}, planes = {planes}")
    assert share <= 0.01
    assert w0 < 30 or share > 0.0002          # (the w0 = 30 case does have near-uniform phases)


@pytest.mark.parametrize("planes", [1, 2])
@pytest.mark.parametrize("I,J,K,w0", [(300, 512, 64, 30.0), (300, 512, 512, 1.0)])
def test_standin_sine_and_derivative_epilogues_meet_their_bars(I, J, K, w0, planes):
    """The epilogues' operation sequences (bsp_kc.hip) in numpy fp32 on the stand-in's accumulators.  Forward: x = fma(acc, w0 / 2 pi,
    b w0 / 2 pi) in revolutions, rounded once; its sine (fp64: v_sin_f32 is not restated) stored under exponent 13.  Backward: s = the
    stored planes (exact), om = fma(-s, s, 2^26) (ONE rounding: formed exactly in fp64, then rounded), root = sqrt(om) in fp32,
    raw * root, times |w0| 2^-13, to planes.  Both meet the bars of the GPU module."""
    c = _siren_case(I, J, K, w0, planes)
    hw, lw, ew = N.weight_planes(c["W"], planes)
    wh, wl = N.deq(hw, lw, ew)
    acc = _acc32(*_qa(c["X"], planes), wh.T.copy(), wl.T.copy(), planes)
    su = np.float32(np.float32(w0) * np.float32(0.15915494309189533577))
    x = (acc.astype(np.float64) * float(su) + (c["b"] * su).astype(np.float64)).astype(np.float32)
    hh, hl = N.split(np.ldexp(np.sin(2.0 * np.pi * x.astype(np.float64)).astype(np.float32).astype(np.float64), 13), planes)
    H = N.from_planes(hh, hl, 13).astype(np.float64)
    assert N.on_grid_near(H, c["h"], c["dh"], planes, e_fixed=13)["ok"]
    h2, l2, e2 = N.to_planes(H.astype(np.float32), planes)                       # the hook re-quantises the stored activation: the identity
    assert np.array_equal(N.from_planes(h2, l2, N.expand(e2, I, J)).astype(np.float64), H)
    hw2, lw2, ew2 = N.weight_planes(c["W2"], planes)
    w2h, w2l = N.deq(hw2, lw2, ew2)
    raw = _acc32(*_qa(c["G"], planes), w2h.T.copy(), w2l.T.copy(), planes)
    sgn = np.sign(np.cos(c["z"]))
    sv = np.ldexp(H, 13)
    gw, gmag = c["gw"]
    cosr = np.sqrt(np.clip(1.0 - H * H, 0.0, None))
    ref = gw * (w0 * sgn * cosr)
    delta = w0 * cosr * N.acc_bound(c["Kg"], gmag) + SINREC_REL * np.abs(ref)
    skip = np.abs(np.cos(c["z"])) < 2.0 ** -10
    om = (2.0 ** 26 - sv * sv).astype(np.float32)
    v = raw * np.sqrt(np.abs(om))
    D = _as_planes((v * np.float32(w0) * np.float32(2.0 ** -13) * sgn.astype(np.float32)).astype(np.float32), planes)
    res = N.on_grid_near(D, ref, delta, planes, skip=skip)
    print(f"derivative stand-in w0 {w0:g} planes {planes}: error / bound {res['ratio']:.3g}")
    assert res["ok"], res
