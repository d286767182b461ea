"""The references of the registration's table (tests/dsm_numpy.py shift_stats, shift_stats_pass0, centred_bound) and the checks of
tests/test_gpu_dsm_stats.py, on the CPU.

Two questions are answered without a GPU: are the references what they say they are (properties below), and do the checks see what
they are meant to see.  For the second a stand-in "kernel" in numpy -- the restated tiles in fp64, the tile partials written to a
guarded workspace, pass 1 with and without a fused multiply-add -- must pass every check on every case, and the same stand-in with
one planted defect must fail at least one check on at least one case; each defect's test names the case that catches it.  DEFECTS
is the source of the table in DESIGN.md section 5d (printed with -s).  The argument checks of snerf_dsm_ncc_search at the limits
of the centre, the radius and the workspace are in tests/test_dsm_cpu.py, with the other refusals."""
import math
from fractions import Fraction

import numpy as np
import pytest

from tests import dsm_numpy as N
from tests import test_gpu_dsm_stats as G          # cases, inputs, references and checks: no GPU at import


# ---- the references -----------------------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    """fl(a b + c) with ONE rounding, element-wise, without a hardware instruction (Boldo and Melquiond, "Emulation of a FMA and
    correctly rounded sums", 2008): a b = uh + ul and c + uh = th + tl exactly; v = tl + ul rounded to odd; th + v rounded to
    nearest is the fused result.  Held to exact rational arithmetic below."""
    uh, ul = N._two_prod(a, b)
    th, tl = N._two_sum(c, uh)
    vh, vl = N._two_sum(tl, ul)
    even = (np.ascontiguousarray(vh).view(np.int64) & 1) == 0
    vh = np.where((vl != 0) & even, np.nextafter(vh, np.where(vl > 0, np.inf, -np.inf)), vh)
    return th + vh


def test_fma_emulation_is_the_exact_product_and_sum_rounded_once():
    rng = np.random.default_rng(0)
    a = rng.normal(0, 1, 4000) * 2.0 ** rng.integers(-20, 20, 4000)
    b = rng.normal(0, 1, 4000) * 2.0 ** rng.integers(-20, 20, 4000)
    c = rng.normal(0, 1, 4000) * 2.0 ** rng.integers(-40, 40, 4000)
    c[:1000] = -(a[:1000] * b[:1000])                                # cancellation: the result is the product's rounding error
    c[1000:1200] = -(a[1000:1200] * b[1000:1200]) * (1 + 2.0 ** -30)
    a[1200:1400] = 1.0 + 2.0 ** -30                                  # a b + c a tie of fl(a b) + c: the unfused sequence rounds to even
    b[1200:1400] = 1.0 + 2.0 ** -23
    c[1200:1400] = 2.0 ** -53 * rng.choice([-1.0, 1.0], 200)
    got = _fma(a, b, c)
    want = np.array([float(Fraction(x) * Fraction(y) + Fraction(z)) for x, y, z in zip(a.tolist(), b.tolist(), c.tolist())])
    assert np.array_equal(got, want)
    if hasattr(math, "fma"):                                         # (Python 3.13 on: the instruction itself)
        assert got.tolist() == [math.fma(x, y, z) for x, y, z in zip(a.tolist(), b.tolist(), c.tolist())]
    assert (got != a * b + c).sum() > 1000                           # (and it is not the unfused sequence)


def test_two_prod_and_two_sum_are_exact():
    rng = np.random.default_rng(1)
    a, b = rng.normal(30, 5, 500), rng.normal(1e4, 0.01, 500)
    for f, op in ((N._two_prod, lambda x, y: x * y), (N._two_sum, lambda x, y: x + y)):
        hi, lo = f(a, b)
        assert all(Fraction(h) + Fraction(l) == op(Fraction(x), Fraction(y)) for h, l, x, y in zip(hi.tolist(), lo.tolist(), a.tolist(), b.tolist()))


@pytest.mark.parametrize("name", ["centre-east-partly", "holes-96x96-r5", "offset-1e4-64x64-r2"])
def test_shift_stats_against_exact_rational_arithmetic(name):
    """three rows of a case (the first, the middle, the last with pairs) in fractions: count and sums are the exact values correctly
    rounded; the centred sums lie within 2 eps^2-ish (1e-30 relative to their magnitude) of the exact ones about the exact mean"""
    c, (u, v), ref = G.CASES[name], G.inputs(name), G.reference(name)
    S1 = 2 * c["r"] + 1
    rows = [s for s in range(S1 * S1) if ref["table"][s, 0] > 0]
    for s in (rows[0], rows[len(rows) // 2], rows[-1]):
        vs = N._shifted(np.asarray(v, np.float64), c["cx"] - c["r"] + s % S1, c["cy"] - c["r"] + s // S1)
        m = np.isfinite(u) & np.isfinite(vs)
        a, b = [Fraction(x) for x in np.asarray(u, np.float64)[m].tolist()], [Fraction(x) for x in vs[m].tolist()]
        n = len(a)
        sa, sb = sum(a), sum(b)
        ca, cb = [x - sa / n for x in a], [x - sb / n for x in b]
        exact = [sum(x * y for x, y in zip(p, q)) for p, q in ((ca, ca), (cb, cb), (ca, cb))]
        mags = [sum(abs(x * y) for x, y in zip(p, q)) for p, q in ((ca, ca), (cb, cb), (ca, cb))]
        assert ref["table"][s, 0] == n and ref["table"][s, 1] == float(sa) and ref["table"][s, 2] == float(sb)
        for k in range(3):
            got = Fraction(float(ref["table"][s, 3 + k]))
            assert abs(got - exact[k]) <= abs(exact[k]) * Fraction(2) ** -53 + mags[k] * Fraction(2) ** -90, (name, s, k)
            assert mags[k] <= Fraction(float(ref["mags"][s, 2 + k])) <= mags[k] * (1 + Fraction(2) ** -39)
        assert float(sum(abs(x) for x in a)) <= ref["mags"][s, 0] and float(sum(abs(x) for x in b)) <= ref["mags"][s, 1]


def test_pass0_restatement_by_hand():
    """4 x 40 (two tiles): tile 0 holds columns 0 ... 31, summed row by row; tile 1 the eight columns left"""
    rng = np.random.default_rng(2)
    u, v = rng.normal(1e4, 1.0, (4, 40)), rng.normal(1e4, 1.0, (4, 40))
    u[1, 5] = np.nan
    v[2, 33] = np.inf
    got = N.shift_stats_pass0(u, v, 1, 0, 0)
    vs = N._shifted(v, 1, 0)
    tiles = []
    for cols in (range(0, 32), range(32, 40)):
        cnt, su, sv = 0, 0.0, 0.0
        for j in range(4):
            for i in cols:
                if np.isfinite(u[j, i]) and np.isfinite(vs[j, i]):
                    cnt, su, sv = cnt + 1, su + u[j, i], sv + vs[j, i]
        tiles.append((cnt, su, sv))
    assert got.shape == (1, 3) and got[0].tolist() == [tiles[0][0] + tiles[1][0], tiles[0][1] + tiles[1][1], tiles[0][2] + tiles[1][2]]
    assert got[0, 0] == 4 * 39 - 2                                # the shift's last column has no partner; one NaN, one inf


def test_bound_arithmetic():
    assert N.centred_bound(1, 0.0, 0.0, 0.0) == 0.0
    assert N.centred_bound(100, 2.0, 3.0, 5.0) == 104 * N.EPS * 2.0 + 100 * 15.0
    assert N.mean_delta(1, 7.0, 7.0) == N.EPS * 7.0
    assert N.mean_delta(4, 8.0, -2.0) == (3 * N.EPS * 8.0 / 4) * (1 + N.EPS) + N.EPS * 2.0
    row = np.array([10.0, 0.0, 0.0, 4.0, 9.0, 3.0])
    assert N.ncc_of_row(row) == 0.5 and N.ncc_error(row, (4.0, 0.0, 0.0)) == np.inf
    assert abs(N.ncc_error(row, (0.0, 0.0, 0.6)) - 0.1) <= 1e-12


def test_the_cases_are_what_they_are_for():
    G.expected_shape_of_cases()
    for name, (h, w, init, shift) in G.REGISTRATIONS.items():
        p = G.registration_pair(name)
        assert (p["dx"], p["dy"]) == shift and abs(p["b"] - 0.7) < 0.05
        assert np.isnan(p["v"][:, 31:33]).all() and np.isinf(p["u"]).sum() == 2
    assert [len(G.registration_pair(k)["trace"]) for k in G.REGISTRATIONS] == [3, 2, 1]
    assert [t[2:4] for t in G.registration_pair("401x203")["trace"]][0] == (-2, 1)      # (-5, 7) floor-halved twice


def test_a_table_without_a_pair_raises_in_both():
    from snerf_amd.eval.utils import dsm as D
    c = G.CASES[G.ALL_ZERO]
    with pytest.raises(ValueError, match="all NaN"):
        N.compute_ncc(*G.inputs(G.ALL_ZERO), c["r"], c["cx"], c["cy"])
    with pytest.raises(RuntimeError, match="all NaN"):
        D._ncc(G.reference(G.ALL_ZERO)["table"][0].tolist())


# ---- the checks' reach: a stand-in kernel, honest and with planted defects -------------------------------------------------------------
DEFECTS = {
    "halo": "the halo read one column to the right for ox == 0, in the tiles of the first tile column",
    "tiles>256": "the tile partials beyond the first 256 dropped from the reduction",
    "means s-1": "pass 1 using the means of row s - 1",
    "one-pass": "a one-pass variance: sum u^2 - n mu^2 in column 3",
    "unshifted mask": "pass 1 masking on uu, vv of the unshifted v",
}
CAUGHT = {}           # defect -> [(case, the check that failed)]


def workspace_bytes(h, w, r):
    """snerf_dsm_workspace_bytes"""
    return max(-(-h // 32) * -(-w // 32) * 3 * (2 * r + 1) ** 2 * 8, 2 * 1024 * 8)


def standin(name, fused, defect=None):
    """snerf_dsm_ncc_search in numpy on a case's inputs -> ((S, 6) table, the guard bytes behind its workspace).  Pass 0 and the
    reduction are the restatement's; pass 1 centres about fl(sum / count) of the stand-in's own pass 0, masks on the centred
    values as the kernel does, and accumulates a tile serially, with fl(a + fl(du dv)) or with one rounding (fused)."""
    c = G.CASES[name]
    u, v = (np.asarray(a, np.float64) for a in G.inputs(name))
    h, w, r, cx, cy = c["h"], c["w"], c["r"], c["cx"], c["cy"]
    S1 = 2 * r + 1
    U, V = N.ncc_tiles(u, v, cx, cy, r)
    S, nblk = V.shape[0], V.shape[1]
    if defect == "halo":
        first = np.arange(nblk) % -(-w // 32) == 0
        right = N.ncc_tiles(u, v, cx + 1, cy, r)[1]
        for s in range(0, S, S1):
            V[s, first] = right[s, first]
    need = workspace_bytes(h, w, r)
    ws = np.full(need + G.GUARD, 0xA5, np.uint8)
    partial = ws[:nblk * 3 * S * 8].view(np.float64).reshape(nblk, 3, S)
    kept = slice(0, 256) if defect == "tiles>256" else slice(None)
    table = np.zeros((S, 6))
    Ub = np.broadcast_to(U[None], V.shape)
    ok = np.isfinite(Ub) & np.isfinite(V)
    partial[:] = np.stack([ok.sum(-1).astype(np.float64), N.serial_tile_sums(Ub, ok), N.serial_tile_sums(V, ok)], 1).transpose(2, 1, 0)
    for k in range(3):
        table[:, k] = N.reduce_tiles(partial[kept, k].T)
    with np.errstate(invalid="ignore", divide="ignore"):
        muu, muv = table[:, 1] / table[:, 0], table[:, 2] / table[:, 0]
        if defect == "means s-1":
            muu[1:], muv[1:] = muu[:-1].copy(), muv[:-1].copy()
        du, dv = Ub - muu[:, None, None], V - muv[:, None, None]
    ok = np.isfinite(du) & np.isfinite(dv)
    if defect == "unshifted mask":
        inside = np.isfinite(N.ncc_tiles(u, np.zeros_like(v), cx, cy, r)[1])
        ok = np.isfinite(Ub) & np.isfinite(N.ncc_tiles(u, v, 0, 0, 0)[1]) & inside
    pairs = [(Ub, Ub) if defect == "one-pass" else (du, du), (dv, dv), (du, dv)]
    for k, (p, q) in enumerate(pairs):
        a = np.zeros((S, nblk))
        with np.errstate(invalid="ignore", over="ignore"):
            for cell in range(1024):
                a = np.where(ok[..., cell], _fma(p[..., cell], q[..., cell], a) if fused else a + p[..., cell] * q[..., cell], a)
        partial[:, k] = a.T
        table[:, 3 + k] = N.reduce_tiles(partial[kept, k].T)
    if defect == "one-pass":
        with np.errstate(invalid="ignore"):
            table[:, 3] = np.where(table[:, 0] > 0, table[:, 3] - table[:, 0] * muu * muu, 0.0)
    return table, ws[need:]


def _verdict(name, fused, defect):
    """None when every check passes, else the message of the check that failed"""
    table, guard = standin(name, fused, defect)
    try:
        ratio = G.check_table(name, table, table.copy(), np.stack([guard, guard]))
    except AssertionError as e:
        return str(e).split("\n")[0][:60]
    if defect is None:
        RATIOS[(name, fused)] = ratio
    return None


RATIOS = {}


@pytest.mark.parametrize("fused", [False, True], ids=["unfused", "fused"])
@pytest.mark.parametrize("name", list(G.CASES))
def test_honest_standin_passes_every_check(name, fused):
    assert _verdict(name, fused, None) is None
    print(f"stand-in {name} {'fused' if fused else 'unfused'}: worst error / bound {RATIOS[(name, fused)]:.3g}")


def _catch(defect, name, fused=True):
    why = _verdict(name, fused, defect)
    print(f"{DEFECTS[defect]}: {name}: {why or 'NOT caught'}")
    CAUGHT.setdefault(defect, []).append((name, why))
    return why


def test_defect_halo_column_is_caught():
    """caught by pitch-33x65-r1 (and every case with ox == 0 shifts left of the image): at x = cx - r < 0 the first -x columns of
    u have no partner, the defect gives one of them a partner: the count is off.  Radius 0 at centre 0 has no such shift, and the
    stand-in passes there: the pitch cases need r >= 1 to see it."""
    assert _catch("halo", "pitch-33x65-r1") is not None
    assert _catch("halo", "pitch-33x65-r7") is not None
    assert _catch("halo", "centre-inside") is not None


def test_defect_dropped_partials_are_caught():
    """caught by tiles-514-40x8200-r2, the only case with more than 256 tiles; every other case has at most 9 and cannot see it"""
    assert _catch("tiles>256", "tiles-514-40x8200-r2") is not None
    assert _catch("tiles>256", "holes-96x96-r5") is None


def test_defect_neighbouring_means_are_caught():
    """caught by pitch-33x65-r1 and by the fp64 cases: n (mu_s - mu_{s-1})^2 lies far above the bound wherever two shifts' means
    differ; with one shift (radius 0) there is no neighbouring row"""
    assert _catch("means s-1", "pitch-33x65-r1") is not None
    assert _catch("means s-1", "f64-f64-65x33-r3") is not None
    assert _catch("means s-1", "offset-1e4-64x64-r2") is not None
    assert _catch("means s-1", "pitch-33x65-r0") is None


def test_defect_one_pass_variance_is_caught():
    """caught by offset-1e4-64x64-r2 (sum u^2 ~ 4e11 against a centred sum of 0.4: an error ~1e-5 against a bound of 3e-13) and,
    at the offset of 30 m, already by the plain cases"""
    assert _catch("one-pass", "offset-1e4-64x64-r2") is not None
    assert _catch("one-pass", "size-32x32-r5") is not None


def test_defect_unshifted_mask_is_caught():
    """caught by holes-96x96-r5 alone: without NaN or inf in v the masks of the shifted and the unshifted v agree wherever the
    shifted one is inside the image, so a dense case cannot see it"""
    assert _catch("unshifted mask", "holes-96x96-r5") is not None
    assert _catch("unshifted mask", "size-65x33-r5") is None
