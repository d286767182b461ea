"""Kernel-level GPU tests of the block-scaled fp16-plane path (csrc/bsp.h): storage round trip, the K-contiguous GEMM
with every epilogue the passes use, the 32-wide variant, and the weight-gradient GEMM -- each against an fp64 reference
of the same operation, through the C-ABI test hooks.

Accuracy bar: the three-product fp16 contraction of 22-bit operands is fp32-class -- normwise error below that of a plain
fp32 GEMM of the same shape -- and, because every 128 x 128 block carries its own exponent, ROW-wise too: a quiet row
block next to a loud one keeps its own precision (the heavy-tail cases)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ACT_NONE, ACT_SIN, ACT_RELU = 0, 1, 2
AUX_NONE, AUX_RELU_MASK, AUX_SINREC = 0, 2, 3


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _lib():
    from snerf_amd import _lib
    return _lib.lib(), _lib


def _relerr(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-300))


def test_planes_round_trip_and_block_exponents():
    L, lib = _lib()
    g = torch.Generator().manual_seed(0)
    rows, cols = 300, 200
    x = torch.randn(rows, cols, generator=g)
    x[:128] *= 1e-6           # a quiet row block
    x[128:256, :128] *= 3e3   # a loud block
    x = x.to(DEV)
    ld, col0 = 384, 128
    y = torch.empty_like(x)
    E = torch.zeros(3 * 3, dtype=torch.int32, device=DEV)
    lib.check(L.snerf_test_bsp_roundtrip(_p(x), rows, cols, ld, col0, _p(y), _p(E), 2, _st()), "roundtrip")
    # 22 significant bits relative to each BLOCK's maximum
    for rb in range(3):
        for cb in range(2):
            blk = (slice(128 * rb, min(rows, 128 * rb + 128)), slice(128 * cb, min(cols, 128 * cb + 128)))
            m = float(x[blk].abs().max())
            assert float((y[blk] - x[blk]).abs().max()) <= m * 2.0 ** -21, (rb, cb)
            e = int(E[rb * 3 + 1 + cb])
            assert 2.0 ** 13 <= m * 2.0 ** e < 2.0 ** 14, (rb, cb, e, m)
    # ONE plane (SNERF_FLAG_F16X1): the same exponents, 11 significant bits relative to each block's maximum
    y1 = torch.empty_like(x)
    E1 = torch.zeros_like(E)
    lib.check(L.snerf_test_bsp_roundtrip(_p(x), rows, cols, ld, col0, _p(y1), _p(E1), 1, _st()), "roundtrip, one plane")
    assert torch.equal(E1, E)
    for rb in range(3):
        for cb in range(2):
            blk = (slice(128 * rb, min(rows, 128 * rb + 128)), slice(128 * cb, min(cols, 128 * cb + 128)))
            assert float((y1[blk] - x[blk]).abs().max()) <= float(x[blk].abs().max()) * 2.0 ** -10, (rb, cb)


@pytest.fixture(params=[0, 3, 2], ids=["grid_default", "grid_3_workgroups", "grid_2_workgroups"])
def kc_grid(request):
    """Every K-contiguous case runs with the default persistent grid (two workgroups per CU: one tile each at these sizes) and
    with a forced grid of 3 / 2 workgroups (snerf_test_set_kc_grid), where every workgroup walks several tiles and draws them
    from the tile counters: the tile loop, the next-tile prefetch during the epilogue and the hand-counted waits behind it."""
    L, _ = _lib()
    L.snerf_test_set_kc_grid(request.param)
    yield request.param
    L.snerf_test_set_kc_grid(0)


def _kc(A, W, bias=None, A2=None, act=ACT_NONE, w0=1.0, aux=AUX_NONE, Hact=None, Hsign=None, a_col0=0, c_col0=0,
        want_sign=False, want_colsum=False, narrow=False, planes=2, nd_w=None, nd_rows=None):
    L, lib = _lib()
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
    if nd_w is not None:
        return Cm, sign, nd_out
    return Cm, sign, cs


@pytest.mark.parametrize("I,J,K", [(128, 256, 16), (300, 512, 512), (1000, 544, 528), (257, 48, 64), (4096, 1024, 544)])
def test_kc_plain_and_bias(I, J, K, kc_grid):
    g = torch.Generator().manual_seed(I + J + K)
    A = torch.randn(I, K, generator=g).to(DEV)
    W = (torch.randn(J, K, generator=g) * 0.05).to(DEV)
    b = torch.randn(J, generator=g).to(DEV)
    Cm, _, _ = _kc(A, W, b)                       # forward launches carry the bias ...
    ref = A.double() @ W.double().T + b.double()
    fp32 = A @ W.T + b
    err, err32 = _relerr(Cm, ref), _relerr(fp32, ref)
    assert err <= max(2.0 * err32, 2e-7), (err, err32)
    # ... backward launches the bias-gradient partials: per 128-row tile column sums of the stored values (never both)
    Cm0, _, cs = _kc(A, W, None, want_colsum=True)
    ref0 = A.double() @ W.double().T
    assert _relerr(Cm0, ref0) <= max(2.0 * _relerr(A @ W.T, ref0), 2e-7)
    want = torch.stack([ref0[r:r + 128].sum(0) for r in range(0, I, 128)])
    assert _relerr(cs, want) <= 1e-5


def test_kc_two_segments_offsets_and_exponent_changes(kc_grid):
    """[gamma | h] style two-segment A, A placed at a column offset, output at a column offset, and A blocks whose
    magnitudes differ by 2^20 along k: the accumulators are rescaled between column blocks (and segments)"""
    g = torch.Generator().manual_seed(7)
    I, Ka, Kb, J = 384, 256, 272, 512
    A = torch.randn(I, Ka, generator=g)
    A[:, 128:] *= 2.0 ** -20
    A[128:256] *= 2.0 ** 9
    A2 = torch.randn(I, Kb, generator=g) * 37.0
    W = torch.randn(J, Ka + Kb, generator=g)
    A, A2, W = A.to(DEV), A2.to(DEV), W.to(DEV)

    def check(Am, A2m, Wm, **kw):
        Cm, _, _ = _kc(Am, Wm, None, A2=A2m, **kw)
        cat = Am if A2m is None else torch.cat([Am, A2m], 1)
        ref = cat.double() @ Wm.double().T
        rows = (Cm.double() - ref).norm(dim=1) / ref.norm(dim=1)
        rows32 = ((cat @ Wm.T).double() - ref).norm(dim=1) / ref.norm(dim=1)
        assert float(rows.max()) <= max(4.0 * float(rows32.max()), 4e-7), (float(rows.max()), float(rows32.max()))
    check(A, A2, W, a_col0=128, c_col0=256)            # loud, quiet (2^-20), loud segment: two rescales up / down
    check(A, None, W[:, :Ka].contiguous(), a_col0=128)  # ends on the quiet block
    # the quiet block alone decides the result when the loud columns meet zero weights: it must keep its own 22 bits
    Wz = W.clone()
    Wz[:, :128] = 0
    Wz[:, Ka:] = 0
    check(A, A2, Wz, a_col0=128, c_col0=128)


@pytest.mark.parametrize("I,J,K,w0", [(300, 512, 64, 30.0), (1000, 1024, 544, 1.0)])
def test_kc_siren_forward_then_derivative_epilogue(I, J, K, w0, kc_grid):
    """forward: h = sin(w0 (x W^T + b)) + sign words of cos; backward epilogue: (g W2^T) * w0 cos(w0 z) rebuilt from the
    stored h and the sign bits, + column sums"""
    g = torch.Generator().manual_seed(I + K)
    X = (torch.rand(I, K, generator=g) * 2 - 1).to(DEV)
    W = (torch.randn(J, K, generator=g) * (0.3 / K ** 0.5)).to(DEV)
    b = (torch.randn(J, generator=g) * 0.1).to(DEV)
    H, sign, _ = _kc(X, W, b, act=ACT_SIN, w0=w0, want_sign=True, c_col0=128)
    z = (X.double() @ W.double().T + b.double()) * w0
    assert float((H.double() - torch.sin(z)).abs().max()) <= 4e-6 * max(1.0, w0 / 8)
    Kg = 256
    G = torch.randn(I, Kg, generator=g).to(DEV)
    G[:128] *= 1e-7                                     # a quiet block of gradient rows
    W2 = (torch.randn(J, Kg, generator=g) * 0.05).to(DEV)
    D, _, cs = _kc(G, W2, None, aux=AUX_SINREC, Hact=H, Hsign=sign, w0=w0, want_colsum=True, c_col0=128)
    ref = (G.double() @ W2.double().T) * (w0 * torch.cos(z))
    # where |cos| is tiny the rebuilt sqrt(1 - h^2) carries h's rounding: compare normwise per row
    rows = (D.double() - ref).norm(dim=1) / ref.norm(dim=1)
    tol = 2e-5 * max(1.0, w0 / 6)   # |cos| = sqrt(1 - h^2) amplifies h's rounding by w0 |tan|: measured 4e-5 at w0 = 30, 1e-5 at 1
    assert float(rows.max()) <= tol, float(rows.max())
    assert float(rows[:128].max()) <= tol                 # the quiet rows are as accurate as the loud ones
    want = torch.stack([ref[r:r + 128].sum(0) for r in range(0, I, 128)])
    assert _relerr(cs, want) <= 1e-4


@pytest.mark.parametrize("planes", [2, 1])
@pytest.mark.parametrize("I,J,K,w0,signs", [(300, 512, 512, 1.0, True), (1000, 256, 256, 1.0, False), (257, 1024, 64, 30.0, True)])
def test_kc_siren_forward_with_folded_projection(I, J, K, w0, signs, planes, kc_grid):
    """ACT_SIN launches of whole 256-column tiles can take the 1-wide projection that follows the layer (sigma after the trunk, the
    sun-visibility output) in their epilogue: every wave writes, per point, the dot product of its 64 fp32 sine values with nd_w;
    the tiles_j * 4 partials summed in order equal h . nd_w (h = the sine values BEFORE they are rounded to planes), and the layer's
    own output is what it is without the projection."""
    g = torch.Generator().manual_seed(I + J)
    X = (torch.rand(I, K, generator=g) * 2 - 1).to(DEV)
    W = (torch.randn(J, K, generator=g) * (0.3 / K ** 0.5)).to(DEV)
    b = (torch.randn(J, generator=g) * 0.1).to(DEV)
    nw = torch.randn(J, generator=g).to(DEV)
    H0, s0, _ = _kc(X, W, b, act=ACT_SIN, w0=w0, want_sign=signs, planes=planes)
    H1, s1, parts = _kc(X, W, b, act=ACT_SIN, w0=w0, want_sign=signs, planes=planes, nd_w=nw)
    assert torch.equal(H0, H1) and (s0 is None or torch.equal(s0, s1))
    assert parts.shape == ((J // 256) * 4, I) and bool(torch.isfinite(parts).all())
    got = parts[0].clone()
    for q in range(1, parts.shape[0]):
        got += parts[q]
    z = (X.double() @ W.double().T + b.double()) * w0
    want = torch.sin(z) @ nw.double()
    tol = (4e-6 if planes == 2 else 2.0 ** -10 * (1.0 + float(z.abs().max()))) * float(nw.abs().sum())
    assert float((got.double() - want).abs().max()) <= tol, float((got.double() - want).abs().max())
    # each partial is one wave's 64 columns
    hq = torch.sin(z)
    for q in range(parts.shape[0]):
        assert float((parts[q].double() - hq[:, 64 * q: 64 * q + 64] @ nw.double()[64 * q: 64 * q + 64]).abs().max()) <= tol


@pytest.mark.parametrize("planes", [2, 1])
@pytest.mark.parametrize("I,rows,signs", [(300, (3, 5, 1, 0), True), (1000, (3, 1, 1, 0, 0), False), (257, (0, 5, 5), True)])
def test_kc_siren_forward_with_folded_final_layers(I, rows, signs, planes, kc_grid):
    """The general form of the folded projection: column tile tj of the launch takes rows[tj] <= 5 projections of ITS 256 columns (the
    fused first head layer: one tile per head, whose final layer is rows[tj] x 256 -- 3 colours, C classes, 1 beta; the sun block's
    tile takes none).  Partials land at nd_out[(tj * 4 + wave) * 5 + o]; slots beyond rows[tj] are never written."""
    J, K = 256 * len(rows), 528
    g = torch.Generator().manual_seed(I + J)
    X = (torch.rand(I, K, generator=g) * 2 - 1).to(DEV)
    W = (torch.randn(J, K, generator=g) * (0.3 / K ** 0.5)).to(DEV)
    b = (torch.randn(J, generator=g) * 0.1).to(DEV)
    nw = torch.randn(sum(rows), J, generator=g).to(DEV)
    H0, s0, _ = _kc(X, W, b, act=ACT_SIN, want_sign=signs, planes=planes)
    H1, s1, parts = _kc(X, W, b, act=ACT_SIN, want_sign=signs, planes=planes, nd_w=nw, nd_rows=rows)
    assert torch.equal(H0, H1) and (s0 is None or torch.equal(s0, s1))
    parts = parts.view(len(rows), 4, 5, I)
    hq = torch.sin(X.double() @ W.double().T + b.double())
    r0 = 0
    for tj, n in enumerate(rows):
        assert bool(torch.isnan(parts[tj, :, n:]).all()), "a slot beyond the tile's projections was written"
        for o in range(n):
            wrow = nw[r0 + o].double()
            tol = (4e-6 if planes == 2 else 2.0 ** -10 * 2.0) * float(wrow[256 * tj: 256 * tj + 256].abs().sum())
            for w in range(4):
                c0 = 256 * tj + 64 * w
                want = hq[:, c0: c0 + 64] @ wrow[c0: c0 + 64]
                assert float((parts[tj, w, o].double() - want).abs().max()) <= tol, (tj, w, o)
        r0 += n


@pytest.mark.parametrize("planes", [2, 1])
def test_kc_planes_at_full_size_do_not_depend_on_the_epilogue_variant(planes):
    """262,144 rows (the headline launch: 2 workgroups per CU, LDS and the store path busy): the layer's output planes must be the same
    bits whether or not projections ride in the epilogue, with and without sign words, run after run.  This is the launch on which
    the round-4 store hazard showed (csrc/bsp_dev.h store_data_guard: ~1.5 % of the rows wrong in one instantiation, different rows every
    run, invisible at test sizes); tests/test_build_cpu.py checks the generated code for the pattern, this checks the behaviour."""
    I, rows, K = 262144, (3, 5, 1, 0), 528
    J = 256 * len(rows)
    g = torch.Generator().manual_seed(5)
    X = (torch.rand(I, K, generator=g) * 2 - 1).to(DEV)
    W = (torch.randn(J, K, generator=g) * (0.3 / K ** 0.5)).to(DEV)
    b = (torch.randn(J, generator=g) * 0.1).to(DEV)
    nw = torch.randn(sum(rows), J, generator=g).to(DEV)
    ref = None
    for signs in (False, True):
        for nd in (None, "five", "one"):
            for rep in range(2):
                if nd == "five":
                    H, _, _ = _kc(X, W, b, act=ACT_SIN, want_sign=signs, planes=planes, nd_w=nw, nd_rows=rows)
                elif nd == "one":
                    H, _, _ = _kc(X, W, b, act=ACT_SIN, want_sign=signs, planes=planes, nd_w=nw[0].contiguous())
                else:
                    H, _, _ = _kc(X, W, b, act=ACT_SIN, want_sign=signs, planes=planes)
                if ref is None:
                    ref = H
                else:
                    assert torch.equal(H, ref), (signs, nd, rep, int((H != ref).sum()))
    # the backward launches (stored activation in, column sums out) likewise: the same bits run after run
    G = (torch.randn(I, J, generator=g) * 0.1).to(DEV)
    outs = [_kc(G, W.T.contiguous()[:K - 16], None, act=ACT_NONE, want_colsum=True, planes=planes)[0] for _ in range(3)]
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


def test_kc_relu_forward_and_mask(kc_grid):
    g = torch.Generator().manual_seed(11)
    I, J, K = 520, 256, 96
    X = torch.randn(I, K, generator=g).to(DEV)
    W = torch.randn(J, K, generator=g).to(DEV)
    H, _, _ = _kc(X, W, None, act=ACT_RELU)
    ref = torch.relu(X.double() @ W.double().T)
    assert _relerr(H, ref) <= 3e-7
    G = torch.randn(I, 64, generator=g).to(DEV)
    W2 = torch.randn(J, 64, generator=g).to(DEV)
    D, _, _ = _kc(G, W2, None, aux=AUX_RELU_MASK, Hact=H)
    want = (G.double() @ W2.double().T) * (ref > 0)
    # entries whose pre-activation is within rounding of zero may flip the mask: exclude |z| < 1e-5
    sure = (X.double() @ W.double().T).abs() > 1e-5
    assert float(((D.double() - want) * sure).abs().max()) <= 1e-5 * float(want.abs().max())


@pytest.mark.parametrize("I,K", [(300, 512), (1000, 768), (129, 32)])
def test_kc_narrow_fp32_output(I, K):
    g = torch.Generator().manual_seed(I)
    A = torch.randn(I, K, generator=g)
    A[:100] *= 1e-5
    W = torch.randn(9, K, generator=g) * 0.1
    b = torch.randn(9, generator=g)
    A, W, b = A.to(DEV), W.to(DEV), b.to(DEV)
    Cm, _, _ = _kc(A, W, b, narrow=True)
    ref = A.double() @ W.double().T + b.double()
    assert float((Cm[:, :9].double() - ref).abs().max()) <= 2e-6 * float(ref.abs().max())
    C0, _, _ = _kc(A, W, None, narrow=True)              # without the bias the quiet rows show their own precision
    ref0 = A.double() @ W.double().T
    rows = (C0[:, :9].double() - ref0).norm(dim=1) / ref0.norm(dim=1)
    assert float(rows.max()) <= 3e-6, float(rows.max())


def _dw(A, B, I, J, a_col0=0, b_col0=0, k_split=1024, narrow=False, planes=2):
    L, lib = _lib()
    P = A.shape[0]
    Cm = torch.full((I, J), float("nan"), device=DEV)
    lib.check(L.snerf_test_bsp_dw(_p(A), A.shape[1], _p(B), B.shape[1], P, I, J, a_col0, b_col0, k_split, int(narrow), _p(Cm), planes, _st()),
              "test_bsp_dw")
    return Cm


@pytest.mark.parametrize("P,I,J,ks", [(2048, 256, 256, 1024), (5000, 512, 544, 1024), (650, 256, 64, 128), (20000, 1024, 528, 4096)])
def test_dw(P, I, J, ks):
    g = torch.Generator().manual_seed(P + I)
    A = torch.randn(P, I, generator=g)
    B = torch.randn(P, J, generator=g)
    # heavy tail along the contraction axis: blocks of points 2^18 apart
    scale = torch.ones(P)
    scale[: P // 3] = 2.0 ** -18
    scale[P // 3: P // 2] = 2.0 ** 6
    A = (A * scale[:, None]).to(DEV)
    B = B.to(DEV)
    Cm = _dw(A, B, I, J, k_split=ks)
    ref = A.double().T @ B.double()
    fp32 = A.T @ B
    err, err32 = _relerr(Cm, ref), _relerr(fp32, ref)
    assert err <= max(2.0 * err32, 3e-7), (err, err32)


def test_dw_column_offsets_and_narrow():
    g = torch.Generator().manual_seed(3)
    P = 3000
    A = torch.randn(P, 384, generator=g).to(DEV)
    B = torch.randn(P, 448, generator=g).to(DEV)
    Cm = _dw(A, B, 256, 320, a_col0=128, b_col0=128)
    ref = A[:, 128:384].double().T @ B[:, 128:448].double()
    assert _relerr(Cm, ref) <= max(2.0 * _relerr(A[:, 128:384].T @ B[:, 128:448], ref), 3e-7)
    An = torch.randn(P, 32, generator=g).to(DEV)
    An[:1000] *= 1e-6
    Cn = _dw(An, B, 32, 448, narrow=True)
    refn = An.double().T @ B.double()
    assert _relerr(Cn, refn) <= max(2.0 * _relerr(An.T @ B, refn), 3e-7)
    Cn2 = _dw(An, B, 9, 200, b_col0=192, narrow=True)
    assert _relerr(Cn2, An[:, :9].double().T @ B[:, 192:392].double()) <= 6e-7


def test_vanishing_blocks_next_to_loud_ones_stay_finite():
    """Blocks 2^90 ... 2^110 apart along a contraction: the exponent of a vanishing block is capped at 60
    (it loses bits, then flushes) and dW drops a chunk more than 2^64 below the frame of its accumulators, so the
    accumulator rescale cannot overflow: finite results, within the yardstick of an fp32 GEMM, where a lone quiet block
    used to end in Inf / NaN gradients."""
    g = torch.Generator().manual_seed(11)
    I, K, J = 300, 640, 256
    A = torch.randn(I, K, generator=g)
    A[:, 128:256] *= 2.0 ** -90      # nonzero, vanishing: between two ordinary blocks
    A[:, 256:384] *= 2.0 ** 20       # loud
    A[:, 384:512] *= 2.0 ** -110     # vanishing again, then an ordinary block ends the contraction
    W = torch.randn(J, K, generator=g)
    A, W = A.to(DEV), W.to(DEV)
    Cm, _, _ = _kc(A, W)
    ref = A.double() @ W.double().T
    assert bool(torch.isfinite(Cm).all())
    assert _relerr(Cm, ref) <= max(2.0 * _relerr(A @ W.T, ref), 3e-7)
    # ends ON a vanishing block (the epilogue's frame is the quiet one)
    Cq, _, _ = _kc(A[:, :512].contiguous(), W[:, :512].contiguous())
    refq = A[:, :512].double() @ W[:, :512].double().T
    assert bool(torch.isfinite(Cq).all()) and _relerr(Cq, refq) <= max(2.0 * _relerr(A[:, :512] @ W[:, :512].T, refq), 3e-7)
    # dW: chunks of points 2^-100 / 2^-60 (both operands) between ordinary ones, first and last chunk included
    P = 1536
    X = torch.randn(P, 256, generator=g)
    Z = torch.randn(P, 256, generator=g)
    sc = torch.ones(P)
    sc[:128] = 2.0 ** -100
    sc[384:512] = 2.0 ** -60
    sc[1408:] = 2.0 ** -100
    Xs = (X * sc[:, None]).to(DEV)
    Zs = (Z * sc[:, None]).to(DEV)     # products down to 2^-200: exponent sums far beyond the accumulators' reach
    Cd = _dw(Zs, Xs, 256, 256, k_split=1536)
    refd = Zs.double().T @ Xs.double()
    assert bool(torch.isfinite(Cd).all())
    assert _relerr(Cd, refd) <= max(2.0 * _relerr(Zs.T @ Xs, refd), 3e-7)


# ---------------------------------------------------------------------------------------------------------------------
# ONE-PLANE form (SNERF_FLAG_F16X1, the reduced-precision mode): the same kernels instantiated for one fp16 plane.  Yardstick:
# the error of the same contraction with both operands rounded to fp16 once (what one plane can hold at best); the block
# exponents must keep that relative precision for quiet blocks next to loud ones (where a plain .half() would flush).
# UNPINNED bars -- the reference runs no half-precision path here.
# ---------------------------------------------------------------------------------------------------------------------
def _err16(A, W, ref):
    return _relerr(A.half().double() @ W.half().double().T, ref)


@pytest.mark.parametrize("I,J,K", [(128, 256, 16), (300, 512, 512), (1000, 544, 528), (257, 48, 64), (4096, 1024, 544), (300, 256, 32)])
def test_one_plane_kc_plain_bias_colsum(I, J, K, kc_grid):
    g = torch.Generator().manual_seed(I + J + K)
    A = torch.randn(I, K, generator=g).to(DEV)
    W = (torch.randn(J, K, generator=g) * 0.05).to(DEV)
    b = torch.randn(J, generator=g).to(DEV)
    Cm, _, _ = _kc(A, W, b, planes=1)
    ref = A.double() @ W.double().T + b.double()
    assert _relerr(Cm, ref) <= 2.0 * _err16(A, W, A.double() @ W.double().T) + 1e-6 + 2.0 ** -11   # (+ the output's own rounding to one plane)
    Cm0, _, cs = _kc(A, W, None, want_colsum=True, planes=1)
    ref0 = A.double() @ W.double().T
    assert _relerr(Cm0, ref0) <= 2.0 * _err16(A, W, ref0) + 2.0 ** -11
    want = torch.stack([ref0[r:r + 128].sum(0) for r in range(0, I, 128)])
    assert _relerr(cs, want) <= 2e-3            # column sums are taken from the fp32 values before they are rounded to the plane


def test_one_plane_kc_two_segments_offsets_and_exponent_changes(kc_grid):
    g = torch.Generator().manual_seed(7)
    I, Ka, Kb, J = 384, 256, 288, 512
    A = torch.randn(I, Ka, generator=g)
    A[:, 128:] *= 2.0 ** -20
    A[128:256] *= 2.0 ** 9
    A2 = torch.randn(I, Kb, generator=g) * 37.0
    W = torch.randn(J, Ka + Kb, generator=g)
    A, A2, W = A.to(DEV), A2.to(DEV), W.to(DEV)

    def check(Am, A2m, Wm, **kw):
        Cm, _, _ = _kc(Am, Wm, None, A2=A2m, planes=1, **kw)
        cat = Am if A2m is None else torch.cat([Am, A2m], 1)
        ref = cat.double() @ Wm.double().T
        rows = (Cm.double() - ref).norm(dim=1) / ref.norm(dim=1)
        assert float(rows.max()) <= 2e-3, float(rows.max())
    check(A, A2, W, a_col0=128, c_col0=256)
    check(A, None, W[:, :Ka].contiguous(), a_col0=128)
    Wz = W.clone()
    Wz[:, :128] = 0
    Wz[:, Ka:] = 0
    check(A, A2, Wz, a_col0=128, c_col0=128)      # the quiet block alone decides the result: its own 11 bits, not the loud block's


@pytest.mark.parametrize("I,J,K,w0", [(300, 512, 64, 30.0), (1000, 1024, 544, 1.0)])
def test_one_plane_siren_forward_then_derivative_epilogue(I, J, K, w0, kc_grid):
    g = torch.Generator().manual_seed(I + K)
    X = (torch.rand(I, K, generator=g) * 2 - 1).to(DEV)
    W = (torch.randn(J, K, generator=g) * (0.3 / K ** 0.5)).to(DEV)
    b = (torch.randn(J, generator=g) * 0.1).to(DEV)
    H, sign, _ = _kc(X, W, b, act=ACT_SIN, w0=w0, want_sign=True, c_col0=128, planes=1)
    z = (X.double() @ W.double().T + b.double()) * w0
    # operand rounding 2^-11 enters the sine's argument times |w0 z| ...
    assert float((H.double() - torch.sin(z)).abs().max()) <= 2.0 ** -10 * (1.0 + float(z.abs().max())) + 2.0 ** -11
    zh = torch.asin(H.double().clamp(-1, 1))       # ... the derivative epilogue rebuilds |cos| from the STORED h and takes its sign from the bits
    Kg = 256
    G = torch.randn(I, Kg, generator=g).to(DEV)
    G[:128] *= 1e-7
    W2 = (torch.randn(J, Kg, generator=g) * 0.05).to(DEV)
    D, _, cs = _kc(G, W2, None, aux=AUX_SINREC, Hact=H, Hsign=sign, w0=w0, want_colsum=True, c_col0=128, planes=1)
    cos_stored = torch.sqrt((1 - H.double() ** 2).clamp_min(0)) * torch.sign(torch.cos(z))
    ref = (G.double() @ W2.double().T) * (w0 * cos_stored)
    # entries where cos(z) is within the forward's own error of zero may carry either sign: compare rows in the norm
    rows = (D.double() - ref).norm(dim=1) / ref.norm(dim=1)
    assert float(rows.max()) <= 2e-2, float(rows.max())
    assert float(rows[:128].max()) <= 2e-2


def test_one_plane_relu_forward_and_mask(kc_grid):
    g = torch.Generator().manual_seed(11)
    I, J, K = 520, 256, 96
    X = torch.randn(I, K, generator=g).to(DEV)
    W = torch.randn(J, K, generator=g).to(DEV)
    H, _, _ = _kc(X, W, None, act=ACT_RELU, planes=1)
    z = X.double() @ W.double().T
    assert _relerr(H, torch.relu(z)) <= 2.0 * _err16(X, W, z) + 2.0 ** -11
    G = torch.randn(I, 64, generator=g).to(DEV)
    W2 = torch.randn(J, 64, generator=g).to(DEV)
    D, _, _ = _kc(G, W2, None, aux=AUX_RELU_MASK, Hact=H, planes=1)
    want = (G.double() @ W2.double().T) * (H.double() > 0)
    assert _relerr(D, want) <= 2.0 * _err16(G, W2, G.double() @ W2.double().T) + 2.0 ** -11


@pytest.mark.parametrize("I,K", [(300, 512), (1000, 768), (129, 32), (257, 528)])
def test_one_plane_kc_narrow_fp32_output(I, K):
    g = torch.Generator().manual_seed(I)
    A = torch.randn(I, K, generator=g)
    A[:100] *= 1e-5
    W = torch.randn(9, K, generator=g) * 0.1
    b = torch.randn(9, generator=g)
    A, W, b = A.to(DEV), W.to(DEV), b.to(DEV)
    C0, _, _ = _kc(A, W, None, narrow=True, planes=1)
    ref0 = A.double() @ W.double().T
    rows = (C0[:, :9].double() - ref0).norm(dim=1) / ref0.norm(dim=1)
    assert float(rows.max()) <= 3e-3, float(rows.max())           # the quiet rows as accurate as the loud ones
    Cm, _, _ = _kc(A, W, b, narrow=True, planes=1)
    assert float((Cm[:, :9].double() - (ref0 + b.double())).abs().max()) <= 3e-3 * float(ref0.abs().max())


@pytest.mark.parametrize("P,I,J,ks", [(2048, 256, 256, 1024), (5000, 512, 544, 1024), (650, 256, 64, 128), (20000, 1024, 528, 4096), (1000, 256, 256, 1024)])
def test_one_plane_dw(P, I, J, ks):
    g = torch.Generator().manual_seed(P + I)
    A = torch.randn(P, I, generator=g)
    B = torch.randn(P, J, generator=g)
    scale = torch.ones(P)
    scale[: P // 3] = 2.0 ** -18
    scale[P // 3: P // 2] = 2.0 ** 6
    A = (A * scale[:, None]).to(DEV)
    B = B.to(DEV)
    Cm = _dw(A, B, I, J, k_split=ks, planes=1)
    ref = A.double().T @ B.double()
    err16 = _relerr(A.half().double().T @ B.half().double(), ref)
    assert _relerr(Cm, ref) <= 2.0 * err16 + 1e-6, (_relerr(Cm, ref), err16)


def test_one_plane_dw_column_offsets_and_narrow():
    g = torch.Generator().manual_seed(3)
    P = 3000
    A = torch.randn(P, 384, generator=g).to(DEV)
    B = torch.randn(P, 448, generator=g).to(DEV)
    Cm = _dw(A, B, 256, 320, a_col0=128, b_col0=128, planes=1)
    ref = A[:, 128:384].double().T @ B[:, 128:448].double()
    assert _relerr(Cm, ref) <= 1e-3
    An = torch.randn(P, 32, generator=g).to(DEV)
    An[:1000] *= 1e-6
    Cn = _dw(An, B, 32, 448, narrow=True, planes=1)
    refn = An.double().T @ B.double()
    assert _relerr(Cn, refn) <= 1e-3
    Cn2 = _dw(An, B, 9, 200, b_col0=192, narrow=True, planes=1)
    assert _relerr(Cn2, An[:, :9].double().T @ B[:, 192:392].double()) <= 1e-3


SIN_WIDE_STATS = []   # worst error beyond 256 revolutions per plane count (printed with -s)


@pytest.mark.parametrize("planes", [2, 1])
def test_siren_sine_beyond_256_revolutions(planes):
    """Every ACT_SIN epilogue hands v_sin_f32 its argument in revolutions WITHOUT range reduction (bsp_kc_epi.h: sin2pi8<SIN_DIRECT>); the
    instruction documents |x| <= 256 revolutions.  Pre-activations here span 0 ... 4,000 revolutions, about half beyond 256, on an EXACT
    GEMM: A and W are small integers / quarters that both plane layouts hold exactly and whose fp32 sums are exact, so the only rounding
    left before the sine is the fp32 argument x = z (w0 / 2 pi).  Bar, the same inside and outside the domain: 2 pi ulp(|x|) + 2e-6
    against the fp64 sin(2 pi x) (+ the fp16 storage of the value, 2^-12, with one plane).  The sign words of cos must match wherever
    x is more than one ulp from a zero of cos."""
    g = torch.Generator().manual_seed(17 + planes)
    I, J, K, w0 = 256, 256, 64, 30.0
    n_lo = torch.randint(-50, 51, (I // 2,), generator=g)                    # |x| <= ~240 revolutions
    n_hi = torch.randint(60, 841, (I - I // 2,), generator=g) * (torch.randint(0, 2, (I - I // 2,), generator=g) * 2 - 1)
    A = torch.randint(-2, 3, (I, K), generator=g).float()
    A[:, 0] = torch.cat([n_lo, n_hi]).float()
    W = torch.randint(-2, 3, (J, K), generator=g).float() / 4
    W[:, 0] = (torch.randint(0, 2, (J,), generator=g) * 2 - 1).float()
    z = A.double() @ W.double().T                                            # exact (and exact in fp32: multiples of 1/4 below 2^11)
    assert float(z.abs().max()) < 2 ** 11
    H, sign, _ = _kc(A.to(DEV), W.to(DEV), None, act=ACT_SIN, w0=w0, want_sign=True, planes=planes)
    # the kernel's scale: 2^-e w0 (exact) times fp32(1 / 2 pi), rounded once; the FMA then rounds x once
    su = float(np.float32(np.float32(w0) * np.float32(1.0 / (2 * np.pi))))
    xk = z * su                                                              # exact in fp64 (13 + 24 bits)
    x32 = xk.float().double()                                                # the argument v_sin_f32 receives
    ulp = torch.from_numpy(np.spacing(np.abs(x32.numpy()).astype(np.float32)).astype(np.float64))
    bar = 2 * np.pi * ulp + 2e-6 + (2.0 ** -12 if planes == 1 else 0.0)
    err = (H.double().cpu() - torch.sin(2 * np.pi * xk)).abs()
    wide = xk.abs() > 256
    frac_wide = float(wide.double().mean())
    assert 0.4 <= frac_wide <= 0.6 and float(xk.abs().max()) > 3500, (frac_wide, float(xk.abs().max()))
    assert bool((err <= bar).all()), (int((err > bar).sum()), float((err - bar).max()), float(xk.abs()[err > bar].min()) if bool((err > bar).any()) else None)
    # sign words: word (32-row block, 64-column group, lane = row % 32 + 32 ((col >> 3) & 1)), bit 8 ((col >> 4) & 3) + (col & 7)
    words = sign.cpu().numpy().astype(np.uint32).reshape(I // 32, J // 64, 64)
    rows = np.arange(I)[:, None]
    cols = np.arange(J)[None, :]
    lane = rows % 32 + 32 * ((cols >> 3) & 1)
    bit = 8 * ((cols >> 4) & 3) + (cols & 7)
    got_neg = (words[rows // 32, cols // 64, lane] >> bit.astype(np.uint32)) & 1
    x2 = 2 * x32.numpy()
    want_neg = (np.rint(x2).astype(np.int64) & 1)                           # cos(2 pi x) < 0  <=>  round(2 x) is odd
    clear = np.abs(np.abs(x2 - np.floor(x2)) - 0.5) > 2 * ulp.numpy()        # more than one ulp of x away from a zero of cos
    assert clear.mean() > 0.95
    assert np.array_equal(got_neg[clear], want_neg[clear]), int((got_neg[clear] != want_neg[clear]).sum())
    SIN_WIDE_STATS.append({"planes": planes, "worst_err_beyond_256": float(err[wide].max()), "worst_err_inside": float(err[~wide].max()),
                           "max_revolutions": float(xk.abs().max())})
    print("sine beyond 256 revolutions:", SIN_WIDE_STATS[-1])
