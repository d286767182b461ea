"""CPU-side checks of the fused altitude quantiles (include/snerf_fuse.h, csrc/fuse.hip, eval/utils/fuse.py):
the new header's prototypes and constant against the binding (_lib.HEADER_SIGNATURES), the rank rule and the restatement
(tests/fuse_numpy.py, the oracle of tests/test_gpu_fuse.py) against numpy's own quantile and against its plain-loop form, the
floater case as exact values, and every refusal of the three entries through the binding (none reaches a launch)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from snerf_amd import _lib
from snerf_amd.eval.utils import fuse as F               # the feature under test: every test of this file needs it
from tests import fuse_numpy as N
from tests import ortho_numpy as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "snerf_fuse.h")
DUMMY = 4096        # a non-null address no refusal path dereferences
NAMES = {
    "snerf_fuse_count": ["xyz", "n", "grid", "radius", "z0", "q", "count", "stats", "stream"],
    "snerf_fuse_scatter": ["xyz", "n", "index0", "grid", "radius", "z0", "q", "offsets", "capacity", "cursor", "keys", "stats", "stream"],
    "snerf_fuse_select": ["keys", "offsets", "capacity", "cursor", "cells", "quantiles_host", "n_quantiles", "words", "stats", "stream"],
}


def test_the_new_header_matches_its_binding_rows():
    """include/snerf_fuse.h against its rows of _lib.HEADER_SIGNATURES (tests/abi_header.py), then the constants; the main header, the
    main table, the other headers' rows and the ABI version are untouched"""
    from tests.abi_header import check_header
    check_header("snerf_fuse.h", NAMES)
    text = open(HEADER).read()
    assert int(re.search(r"#define SNERF_FUSE_MAX_QUANTILES (\d+)", text).group(1)) == _lib.FUSE_MAX_QUANTILES == F.MAX_QUANTILES == 8
    assert F.QUARTILES == N.QUARTILES == ((1, 4), (1, 2), (3, 4))


# ---- the rank rule ------------------------------------------------------------------------------------------------------------------
def test_the_rank_rule():
    qs = [(0, 1), (1, 4), (1, 2), (3, 4), (1, 1), (1, 3), (65535, 65536), (7, 10)]
    for num, den in qs:
        assert N.rank(1, num, den) == 0                                    # one point: that point, for every quantile
    for m in range(1, 71):
        assert N.rank(m, 0, 1) == 0 and N.rank(m, 1, 1) == m - 1           # min and max
        assert N.rank(m, 1, 2) == (m - 1) // 2                             # the lower median
    assert [N.rank(m, 1, 2) for m in (2, 4, 6, 64)] == [0, 1, 2, 31]       # even m: the lower of the two middle points
    assert N.rank(2 ** 32 - 1, 65535, 65536) == ((2 ** 32 - 2) * 65535) // 65536 < 2 ** 32


def test_the_rule_agrees_with_numpy_lower_quantiles():
    """m = 1 ... 70 points in one cell at distinct quantised altitudes: every word's altitude is np.quantile(..., method="lower") of
    the quantised altitudes, for quantiles whose (m - 1) num / den numpy's fp64 position holds exactly (den a power of two)"""
    rng = np.random.default_rng(11)
    g = R.grid(0.0, 1.0, 1.0, 1, 1)
    qs = [(0, 1), (1, 4), (1, 2), (3, 4), (1, 1), (3, 8), (1, 65536), (65535, 65536)]
    for m in range(1, 71):
        k = rng.choice(np.arange(-4000, 4000), size=m, replace=False)
        xyz = np.stack([np.full(m, 0.5), np.full(m, 0.5), k * R.Q], 1)
        out = N.fuse([xyz], g, 0, qs)
        assert out["offers"].tolist() == [m] and out["stats"] == [0, m]
        alts = (k * R.Q).astype(np.float64)
        for j, (num, den) in enumerate(qs):
            want = np.quantile(alts, num / den, method="lower")
            assert out["alt"][j, 0] == np.float32(want), (m, num, den)
            assert k[out["index"][j, 0]] * R.Q == want                     # the word's index is that point's


def test_the_floater_case():
    """one cell, five views at 10 m and one point at 40 m: the top surface says 40, the mean 15, the median 10, the spread 0"""
    g = R.grid(100.0, 200.0, 0.5, 3, 3)
    z = [10.0, 10.0, 40.0, 10.0, 10.0, 10.0]
    clouds = [np.array([[100.7, 199.2, v]]) for v in z]                   # six views, one point each, all in cell (1, 1)
    out = N.fuse(clouds, g, 0, N.QUARTILES + ((1, 1), (0, 1)))
    c = 1 * 3 + 1
    assert out["offers"].tolist() == [0, 0, 0, 0, 6, 0, 0, 0, 0]
    q1, med, q3, top, low = (float(v) for v in out["alt"][:, c])
    assert (q1, med, q3, top, low) == (10.0, 10.0, 10.0, 40.0, 10.0) and sum(z) / len(z) == 15.0
    assert float(N.spread(out["words"][0], out["words"][2])[c]) == 0.0
    assert out["index"][:, c].tolist() == [4, 3, 1, 2, 5]                  # equal altitudes: ascending keys are DESCENDING indices
    top_words, _ = R.top_at(np.concatenate(clouds), g)
    assert np.array_equal(out["words"][3], top_words)                      # (1, 1) is snerf_ortho_top's word
    empty = np.delete(np.arange(9), c)
    assert np.isnan(out["alt"][:, empty]).all() and (out["index"][:, empty] == -1).all() and (out["words"][:, empty] == 0).all()
    assert np.isnan(N.spread(out["words"][0], out["words"][2])[empty]).all()
    # the device layer's spread on the same words (plain torch on the words: no GPU needed)
    w = torch.from_numpy(out["words"].view(np.int64))
    got = F.spread(w[0], w[2]).numpy()
    assert np.array_equal(got.view(np.int32), N.spread(out["words"][0], out["words"][2]).view(np.int32))


def test_spread_is_exact_across_the_sign_of_the_altitude():
    lo = np.array([R.encode(-3, 5), R.encode(-2 ** 31, 0), 0, R.encode(7, 1)], np.uint64)
    hi = np.array([R.encode(4, 9), R.encode(2 ** 31 - 1, 1), R.encode(1, 1), 0], np.uint64)
    want = N.spread(lo, hi)
    assert want[:2].tolist() == [7 * R.Q, np.float32((2 ** 32 - 1) * R.Q)] and np.isnan(want[2:]).all()
    got = F.spread(torch.from_numpy(lo.view(np.int64)), torch.from_numpy(hi.view(np.int64))).numpy()
    assert np.array_equal(got.view(np.int32), want.view(np.int32))


def test_the_vectorised_restatement_is_the_loop():
    rng = np.random.default_rng(3)
    g = R.grid(10.0, 22.0, 0.5, 9, 8, ioff=2, joff=1, out_w=5, out_h=6)
    clouds = []
    for n in (40, 1, 500):
        xyz = np.stack([rng.uniform(9.0, 15.5, n), rng.uniform(17.0, 23.0, n), np.round(rng.uniform(-3, 3, n), 1)], 1)
        xyz[::17, 2] = np.nan
        xyz[5::29, 0] = np.inf
        clouds.append(xyz)
    qs = ((0, 1), (1, 3), (1, 2), (1, 1))
    for radius in (0, 1, 2):
        lists, stats = N.offers_loop(clouds, g, radius)
        out = N.fuse(clouds, g, radius, qs)
        assert stats == out["stats"] and [len(v) for v in lists] == out["offers"].tolist()
        assert np.array_equal(N.select_loop(lists, qs), out["words"])
    assert max(out["offers"]) > 64 and min(out["offers"]) >= 0


# ---- refusals of the entries ----------------------------------------------------------------------------------------------------------
def _grid(**kw):
    g = _lib.SnerfDsmGrid(1000.0, 2000.0, 0.5, 4, 3, 0, 0, 4, 3)
    for k, v in kw.items():
        setattr(g, k, v)
    return g


def _quantiles(*pairs):
    flat = [v for p in pairs for v in p]
    return (C.c_int * len(flat))(*flat)


def _call(symbol, **kw):
    """an entry through the binding with dummy addresses: (rc, message); every refusal returns before a launch"""
    L = _lib.lib()
    a = dict(xyz=DUMMY, n=2, index0=0, grid=_grid(), radius=0, z0=0.0, q=2.0 ** -16, count=DUMMY, offsets=DUMMY, capacity=8, cursor=DUMMY,
             keys=DUMMY, stats=DUMMY, cells=12, quantiles_host=_quantiles((1, 2)), n_quantiles=1, words=DUMMY)
    a.update(kw)
    a["grid"] = C.byref(a["grid"]) if a["grid"] is not None else None
    rc = getattr(L, symbol)(*[a[name] for name in NAMES[symbol][:-1]], None)
    return rc, L.snerf_last_error().decode()


WALK_REFUSALS = [
    ({"xyz": None}, 3, "null"), ({"grid": None}, 3, "null"), ({"stats": None}, 3, "null"),
    ({"n": -1}, 1, "n = -1"), ({"n": 2 ** 31 + 1}, 1, "[0, 2^31]"),
    ({"radius": -1}, 1, "radius = -1"), ({"radius": 8}, 1, "radius = 8"),
    ({"grid": _grid(res=0.0)}, 1, "res > 0"), ({"grid": _grid(res=math.nan)}, 1, "res > 0"), ({"grid": _grid(xoff=math.inf)}, 1, "res > 0"),
    ({"grid": _grid(out_h=0)}, 1, "positive sizes"), ({"grid": _grid(xsize=-2)}, 1, "positive sizes"),
    ({"grid": _grid(joff=2 ** 31 - 3)}, 1, "int32"), ({"grid": _grid(ioff=2 ** 31 - 4)}, 1, "int32"),
    ({"q": 0.0}, 1, "q > 0"), ({"q": -1.0}, 1, "q > 0"), ({"q": math.inf}, 1, "q > 0"), ({"q": math.nan}, 1, "q > 0"),
    ({"z0": math.nan}, 1, "z0 finite"), ({"z0": -math.inf}, 1, "z0 finite"),
    ({"n": 0, "radius": 9}, 1, "radius = 9"),                              # n == 0 does not excuse a bad argument
]
SCATTER_REFUSALS = [
    ({"cursor": None}, 3, "null"), ({"offsets": None}, 3, "null"), ({"keys": None}, 3, "null"),
    ({"index0": -1}, 1, "index0 = -1"), ({"index0": 2 ** 32 - 2, "n": 2}, 1, "index0 + n <= 2^32 - 1"), ({"index0": 2 ** 32}, 1, "index0"),
    ({"capacity": -1}, 1, "capacity = -1"),
]
SELECT_REFUSALS = [
    ({"keys": None}, 3, "null"), ({"offsets": None}, 3, "null"), ({"cursor": None}, 3, "null"), ({"quantiles_host": None}, 3, "null"),
    ({"words": None}, 3, "null"), ({"stats": None}, 3, "null"),
    ({"capacity": -5}, 1, "capacity = -5"), ({"cells": 0}, 1, "cells = 0"), ({"cells": 2 ** 31}, 1, "cells = 2147483648"), ({"cells": -1}, 1, "cells"),
    ({"n_quantiles": 0}, 1, "n_quantiles = 0"), ({"n_quantiles": 9}, 1, "n_quantiles = 9"),
    ({"quantiles_host": _quantiles((3, 2))}, 1, "(3, 2)"), ({"quantiles_host": _quantiles((-1, 2))}, 1, "(-1, 2)"),
    ({"quantiles_host": _quantiles((0, 0))}, 1, "(0, 0)"), ({"quantiles_host": _quantiles((1, 65537))}, 1, "(1, 65537)"),
    ({"quantiles_host": _quantiles((1, 2), (1, -4)), "n_quantiles": 2}, 1, "quantile 1 = (1, -4)"),
]
CASES = ([("snerf_fuse_count", kw, code, needle) for kw, code, needle in WALK_REFUSALS + [({"count": None}, 3, "null")]]
         + [("snerf_fuse_scatter", kw, code, needle) for kw, code, needle in WALK_REFUSALS + SCATTER_REFUSALS]
         + [("snerf_fuse_select", kw, code, needle) for kw, code, needle in SELECT_REFUSALS])


@pytest.mark.parametrize("symbol,kw,code,needle", CASES, ids=[f"{s[11:]}-{n}" for n, (s, _, _, _) in enumerate(CASES)])
def test_the_entries_refuse_bad_arguments_before_any_launch(symbol, kw, code, needle):
    rc, msg = _call(symbol, **dict(kw))
    assert rc == code and msg.startswith(symbol + ": ") and needle in msg, (rc, msg)


def test_zero_points_are_accepted_and_launch_nothing():
    """n == 0 with good arguments returns SNERF_OK before the launch: the dummy addresses are never handed to a kernel, and no GPU is
    needed for it"""
    assert _call("snerf_fuse_count", n=0)[0] == 0 and _call("snerf_fuse_count", n=0, xyz=None)[0] == 0
    assert _call("snerf_fuse_scatter", n=0)[0] == 0 and _call("snerf_fuse_scatter", n=0, xyz=None, capacity=0)[0] == 0


def test_python_refusals():
    with pytest.raises(ValueError, match="the cloud must be a GPU tensor"):
        F.count_offers(torch.zeros(2, 3, dtype=torch.float64), _grid())
    with pytest.raises(ValueError, match="no cloud"):
        F.fuse_clouds([], _grid())
    with pytest.raises(ValueError, match="no cloud"):
        F.fuse_walks(lambda: iter(()), _grid())
    with pytest.raises(ValueError, match="9 quantiles"):
        F.quantile_table([(1, 2)] * 9)
    with pytest.raises(ValueError, match="0 quantiles"):
        F.quantile_table([])
    for bad in ((3, 2), (-1, 2), (0, 0), (1, 65537)):
        with pytest.raises(ValueError, match=re.escape(f"quantile ({bad[0]}, {bad[1]})")):
            F.quantile_table([bad])
    table, k = F.quantile_table(F.QUARTILES)
    assert k == 3 and list(table) == [1, 4, 1, 2, 3, 4]
    offsets, total = F.offsets_of(torch.tensor([[3, 0], [-1, 2]], dtype=torch.int32))      # -1 holds the u32 word 2^32 - 1
    assert offsets.dtype == torch.int64 and offsets.tolist() == [0, 3, 3, 2 ** 32 + 2, 2 ** 32 + 4] and total == 2 ** 32 + 4
