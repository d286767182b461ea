"""CPU-side checks of the cast-shadow entries (include/snerf_hip.h, csrc/shadow.hip, eval/utils/shadow.py; DESIGN.md section
5o): the header's constants against the binding (tests/test_abi_cpu.py compares the prototypes with their rows, as for every
entry), every refusal of both entries (none reaches a launch), the Python refusals,
sun_rows against construct_sun_dir, and the numpy restatement (tests/shadow_numpy.py, the oracle of tests/test_gpu_shadow.py)
against an independent brute-force formulation."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import shadow_numpy as SN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "snerf_hip.h")


def test_header_constants_match_the_binding():
    from snerf_amd import _lib
    src = open(HEADER).read()
    assert _lib.lib().snerf_version() == _lib.ABI_VERSION == 6
    assert int(re.search(r"#define SNERF_SHADOW_MAX_SUNS (\d+)", src).group(1)) == _lib.SHADOW_MAX_SUNS == 64
    assert int(re.search(r"#define SNERF_SHADOW_UNKNOWN (\d+)", src).group(1)) == _lib.SHADOW_UNKNOWN == 255


DUMMY = 4096        # a non-null address no refusal path dereferences
S2 = math.sqrt(0.5)
GOOD = (1.0, 0.0, 0.5, S2, -S2, 0.25)


def _rows(*vals):
    return (C.c_double * len(vals))(*vals)


def _cast(dsm=DUMMY, h=3, w=4, suns=None, n=2, bias=0.0, z_top=math.inf, lit=DUMMY, dist=None):
    from snerf_amd import _lib
    suns = _rows(*GOOD) if suns is None else suns
    return _lib.lib().snerf_shadow_cast(dsm, h, w, suns, n, bias, z_top, lit, dist, None)


def _agree(sun=DUMMY, lit=DUMMY, valid=None, cells=12, n=1, threshold=0.5, acc=DUMMY):
    from snerf_amd import _lib
    return _lib.lib().snerf_shadow_agreement(sun, lit, valid, cells, n, threshold, acc, None)


def _bad_row(col, value, row=1):
    v = list(GOOD)
    v[3 * row + col] = value
    return _rows(*v)


REFUSALS = [
    ("cast-null-dsm", lambda: _cast(dsm=None), 3, "null"),
    ("cast-null-suns", lambda: _cast(suns=0), 3, "null"),
    ("cast-null-lit", lambda: _cast(lit=None), 3, "null"),
    ("cast-h0", lambda: _cast(h=0), 1, "h = 0"),
    ("cast-w-neg", lambda: _cast(w=-1), 1, "w = -1"),
    ("cast-2^31-cells", lambda: _cast(h=1 << 16, w=1 << 15), 1, "2^31"),
    ("cast-K0", lambda: _cast(n=0), 1, "n_suns = 0"),
    ("cast-K65", lambda: _cast(n=65), 1, "n_suns = 65"),
    ("cast-ux-nan", lambda: _cast(suns=_bad_row(0, math.nan)), 1, "sun 1 is not finite"),
    ("cast-uy-inf", lambda: _cast(suns=_bad_row(1, math.inf)), 1, "sun 1 is not finite"),
    ("cast-rise-inf", lambda: _cast(suns=_bad_row(2, math.inf)), 1, "sun 1 is not finite"),
    ("cast-not-unit", lambda: _cast(suns=_bad_row(0, 1.0 + 1e-8, row=0)), 1, "sun 0: (ux, uy)"),
    ("cast-rise-0", lambda: _cast(suns=_bad_row(2, 0.0)), 1, "sun 1: rise"),
    ("cast-rise-neg", lambda: _cast(suns=_bad_row(2, -0.25)), 1, "sun 1: rise"),
    ("cast-bias-inf", lambda: _cast(bias=math.inf), 1, "bias"),
    ("cast-bias-nan", lambda: _cast(bias=math.nan), 1, "bias"),
    ("cast-ztop-nan", lambda: _cast(z_top=math.nan), 1, "z_top"),
    ("agree-null-sun", lambda: _agree(sun=None), 3, "null"),
    ("agree-null-lit", lambda: _agree(lit=None), 3, "null"),
    ("agree-null-acc", lambda: _agree(acc=None), 3, "null"),
    ("agree-cells-0", lambda: _agree(cells=0), 1, "cells"),
    ("agree-cells-neg", lambda: _agree(cells=-3), 1, "cells"),
    ("agree-K0", lambda: _agree(n=0), 1, "n_suns = 0"),
    ("agree-K65", lambda: _agree(n=65), 1, "n_suns = 65"),
    ("agree-threshold-nan", lambda: _agree(threshold=math.nan), 1, "threshold"),
    ("agree-threshold-inf", lambda: _agree(threshold=-math.inf), 1, "threshold"),
]


@pytest.mark.parametrize("call,code,needle", [r[1:] for r in REFUSALS], ids=[r[0] for r in REFUSALS])
def test_every_refusal_returns_its_code_and_a_message(call, code, needle):
    """null required pointers; h, w < 1 or h * w >= 2^31; K outside [1, 64]; a sun row that is not finite, not a unit vector to
    1e-9, or with rise <= 0; a bias that is not finite; a NaN z_top; a threshold that is not finite; cells < 1 -- all before the
    device is touched: the addresses are dummies (the sun rows, which ARE read, are host arrays)"""
    from snerf_amd import _lib
    assert call() == code
    msg = _lib.lib().snerf_last_error().decode()
    assert needle in msg and msg.startswith("snerf_shadow_"), msg


def test_the_unit_vector_bound_is_1e_9():
    """ux^2 + uy^2 = 1 + 1.2e-9 is refused (1 + 2e-8 is among the cases above)"""
    from snerf_amd import _lib
    assert _cast(suns=_bad_row(0, 1.0 + 6e-10, row=0)) == 1
    assert "not a unit vector" in _lib.lib().snerf_last_error().decode()


def test_python_refusals():
    from snerf_amd.eval.utils import shadow as S
    dsm = torch.zeros(5, 7)
    with pytest.raises(ValueError, match="GPU tensor"):
        S.cast_shadows(dsm, [(30.0, 100.0)], 0.5)
    with pytest.raises(ValueError, match="GPU tensors"):
        S.shadow_agreement(torch.zeros(1, 5, 7), torch.zeros(1, 5, 7, dtype=torch.uint8))
    for el in (0.0, -3.0, 90.0001, math.nan):
        with pytest.raises(ValueError, match=r"elevation in \(0, 90\]"):
            S.sun_rows([(45.0, 10.0), (el, 10.0)], 0.5)
    with pytest.raises(ValueError, match="azimuth"):
        S.sun_rows([(45.0, math.inf)], 0.5)
    with pytest.raises(ValueError, match="no sun"):
        S.sun_rows([], 0.5)
    with pytest.raises(ValueError, match="res"):
        S.sun_rows([(45.0, 10.0)], 0.0)
    assert S.sun_rows([(90.0, 0.0)], 0.5).shape == (1, 3)            # the zenith is a sun: tan(90 deg) is finite in fp64
    prod = {"dsm": torch.zeros(5, 7), "sun": torch.zeros(2, 5, 6), "suns": [(30.0, 10.0), (40.0, 20.0)],
            "grid": type("G", (), {"resolution": 0.5})()}
    with pytest.raises(ValueError, match="do not belong together"):   # shape mismatches are refused before anything is cast
        S.shadow_check(prod)
    prod["sun"] = torch.zeros(3, 5, 7)
    with pytest.raises(ValueError, match="do not belong together"):
        S.shadow_check(prod)


def test_sun_rows_follow_construct_sun_dir():
    """(ux, uy) is the horizontal direction of construct_sun_dir's (east, north, up) unit vector -- north is -row -- and rise / res
    its slope; construct_sun_dir rounds to fp32, hence the bar of a few fp32 ulps on components of size <= 1"""
    from snerf_amd.baseline.components.rays import construct_sun_dir
    from snerf_amd.eval.utils import shadow as S
    res = 0.3
    for el, az in ((2.0, 0.0), (35.0, 90.0), (35.0, 33.3), (61.5, 180.0), (12.25, 270.0), (45.0, 45.0), (80.0, 359.0)):
        d = construct_sun_dir(el, az, 1)[0].double().numpy()
        ux, uy, rise = S.sun_rows([(el, az)], res)[0]
        hor = math.hypot(d[0], d[1])
        assert abs(ux * hor - d[0]) <= 2e-7 and abs(-uy * hor - d[1]) <= 2e-7, (el, az)
        assert abs(rise / res - d[2] / hor) <= 4e-7 * (1.0 + d[2] / hor) / hor, (el, az)
        assert abs(ux * ux + uy * uy - 1.0) <= 1e-15
    assert np.array_equal(S.sun_rows([(30.0, 10.0), (40.0, 200.0)], res), SN.sun_rows([(30.0, 10.0), (40.0, 200.0)], res))


# ---- the restatement against a brute-force formulation ---------------------------------------------------------------------------
def _brute(dsm, row):
    """Per ray and per cell of the window, analytically (the slab method): does the ground track x0 + t (ux, uy), t > 0, pass
    through the cell's interior, and at which t does it enter?  The ray is shadowed iff some entered cell is higher than the ray
    at its entry; dist is the smallest such entry.  No marching, no accumulated tMax: every entry distance is one division."""
    h, w = dsm.shape
    d64 = dsm.astype(np.float64)
    ux, uy, rise = row
    ci, cj = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    lit = np.ones((h, w), np.uint8)
    dist = np.full((h, w), np.nan)

    def slab(lo, x0, u):
        if u == 0.0:
            inside = (lo < x0) & (x0 < lo + 1.0)
            return np.where(inside, -np.inf, np.inf), np.where(inside, np.inf, -np.inf)
        a, b = (lo - x0) / u, (lo + 1.0 - x0) / u
        return np.minimum(a, b), np.maximum(a, b)

    for j0 in range(h):
        for i0 in range(w):
            if np.isnan(d64[j0, i0]):
                lit[j0, i0] = SN.UNKNOWN
                continue
            x0, y0 = i0 + 0.5, j0 + 0.5
            ax, bx = slab(ci, x0, ux)
            ay, by = slab(cj, y0, uy)
            enter, leave = np.maximum(ax, ay), np.minimum(bx, by)
            crossed = (leave > enter) & (enter > 0.0)
            crossed[j0, i0] = False
            with np.errstate(invalid="ignore"):
                blocks = crossed & (d64 > d64[j0, i0] + rise * enter)
            if blocks.any():
                lit[j0, i0] = 0
                dist[j0, i0] = enter[blocks].min()
    return lit, dist


# seeds for which the restatement's own margins leave out fewer than 1 % of the (cell, sun) pairs (asserted below)
BRUTE_CASES = [((9, 11), 11), ((16, 17), 12)]


@pytest.mark.parametrize("shape,seed", BRUTE_CASES, ids=["9x11", "16x17"])
def test_restatement_agrees_with_the_brute_force_formulation(shape, seed):
    """random DSMs (10 % NaN holes) under 8 random suns.  The two agree in lit wherever the smallest |dsm - hr| and the smallest
    |tMaxX - tMaxY| along the ray exceed 1e-9 -- the rays whose outcome a last-bit difference between an accumulated tMax and a
    single division could flip; fewer than 1 % of the pairs may be left out by that rule."""
    rng = np.random.default_rng(seed)
    h, w = shape
    dsm = rng.uniform(0.0, 12.0, shape).astype(np.float32)
    dsm[rng.random(shape) < 0.1] = np.nan
    suns = np.stack([rng.uniform(3.0, 70.0, 8), rng.uniform(0.0, 360.0, 8)], 1)
    rows = SN.sun_rows(suns, 0.5)
    kept = total = 0
    for row in rows:
        lit, dist, (mh, mt) = SN.cast_one(dsm, row, want_margins=True)
        blit, bdist = _brute(dsm, row)
        keep = (mh > 1e-9) & (mt > 1e-9)
        kept += int(keep.sum())
        total += keep.size
        assert np.array_equal(lit[keep], blit[keep])
        hit = keep & (lit == 0)
        assert np.array_equal(np.isnan(dist[keep]), np.isnan(bdist[keep]))
        # the march accumulates tMax (one rounding per step, at most h + w steps of size <= 1e2); dist is its fp32 rounding
        assert np.allclose(dist[hit], bdist[hit], rtol=2e-7, atol=0.0)
        assert np.array_equal(lit == SN.UNKNOWN, np.isnan(dsm))
        assert ((lit == 0).sum() > 0) and ((lit == 1).sum() > 0)
    print(f"{shape}: {total - kept} of {total} pairs left out")
    assert total - kept < 0.01 * total


def test_restatement_ties_holes_and_the_analytic_box():
    """what the GPU test derives analytically, held on the restatement too: a 10 m box on a plane at res 0.5, elevation 45 deg, sun
    due east -- hr = t * 0.5 at the entries t = 0.5, 1.5, ... of the cells east of a ground cell, so a ground cell d cells west of
    the box's west face first meets the box at t = d - 0.5 and is shadowed iff 10 > (d - 0.5) * 0.5 with bias 0, i.e. d <= 20"""
    dsm = np.zeros((5, 40), np.float32)
    dsm[1:4, 30:33] = 10.0
    rows = SN.sun_rows([(45.0, 90.0)], 0.5)
    rows[0, 1] = -0.0                                                 # due east exactly (cos 90 deg is 6e-17 in fp64)
    rows[0, 2] = 0.5                                                  # tan 45 deg * 0.5, exactly
    lit, dist = SN.cast(dsm, rows)
    for j in (1, 2, 3):
        assert (lit[0, j, :30] == 0).sum() == 20 and bool((lit[0, j, 10:30] == 0).all())
        assert np.array_equal(dist[0, j, 10:30], np.arange(20, 0, -1, dtype=np.float32) - 0.5)
    assert bool((lit[0, (0, 4)] == 1).all()) and bool((lit[0, :, 30:] == 1).all())
    # the tie: ux == uy exactly -> x steps first, then y at the same t; the cell beside the diagonal is tested, and blocks
    s = math.sqrt(0.5)
    d = np.zeros((3, 3), np.float32)
    d[2, 1] = 5.0                                                     # from (i, j) = (0, 1): x to (1, 1), then y to (1, 2) at the same t
    lit, dist = SN.cast(d, [(s, s, 0.1)])
    assert lit[0, 1, 0] == 0 and dist[0, 1, 0] == np.float32(0.5 / s)
    d = np.zeros((3, 3), np.float32)
    d[1, 0] = 5.0                                                     # below the start (0, 0): the y step of a tie never lands there
    lit, _ = SN.cast(d, [(s, s, 0.1)])
    assert lit[0, 0, 0] == 1
    # all NaN: every cell unknown; a NaN cell never blocks
    lit, dist = SN.cast(np.full((2, 3), np.nan, np.float32), rows)
    assert bool((lit == SN.UNKNOWN).all()) and bool(np.isnan(dist).all())


def test_agreement_restatement_words_and_metrics():
    sun = np.array([[0.9, 0.2, 0.5, np.nan, 0.7, 0.1, np.inf, 0.25]], np.float32)
    lit = np.array([[1, 1, 0, 1, 255, 0, 0, 1]], np.uint8)
    valid = np.array([1, 1, 1, 1, 1, 1, 1, 0], np.uint8)
    w = SN.agreement(sun, lit, valid, 0.5)[0].tolist()
    q = lambda v: int(np.rint(np.float64(np.float32(v)) * 2 ** 24))      # noqa: E731
    assert w == [1, 1, 1, 1, 4, q(0.9) + q(0.2), q(0.5) + q(0.1), 0]   # 0.5 >= 0.5: predicted lit
    m = SN.metrics(w)
    assert m["n"] == 4 and m["left_out"] == 4 and m["accuracy"] == 0.5 and m["iou_shadow"] == 1 / 3
    assert abs(m["mean_sun_lit"] - 0.55) < 1e-7 and abs(m["mean_sun_shadow"] - 0.3) < 1e-7
    from snerf_amd.eval.utils import shadow as S
    got = S.agreement_metrics(w)
    assert got.pop("words") == w and got == m and tuple(m) == S.METRICS
    empty = S.agreement_metrics([0, 0, 0, 0, 9, 0, 0, 0])
    assert empty["n"] == 0 and all(math.isnan(empty[k]) for k in ("accuracy", "iou_shadow", "mean_sun_lit", "mean_sun_shadow"))
    neg = SN.agreement(np.array([[-1.5]], np.float32), np.array([[0]], np.uint8))[0]
    assert int(neg[6]) == 2 ** 64 - 3 * 2 ** 23 and SN.metrics(neg)["mean_sun_shadow"] == -1.5
