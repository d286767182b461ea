"""The fused altitude quantiles on the device (csrc/fuse.hip, eval/utils/fuse.py, eval/utils/ortho.py robust=True, eval/ortho.py)
against the numpy restatement (tests/fuse_numpy.py), bit for bit: the spec is integer arithmetic, so no comparison here carries a
tolerance.  Run with -m gpu on an MI355X."""
import json
import os

import numpy as np
import pytest
import torch

from snerf_amd import _lib
from snerf_amd.eval.utils import fuse as F               # the feature under test: every test of this file needs it
from snerf_amd.eval.utils import ortho as OR
from tests import fuse_numpy as N
from tests import ortho_numpy as R
from tests.test_gpu_ortho import SEED, scene             # noqa: F401  (the fixture scene and its seeded, untrained model)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIVE = ((0, 1), (1, 4), (1, 2), (3, 4), (1, 1))
EIGHT = ((0, 1), (1, 1), (1, 2), (1, 65536), (65535, 65536), (32768, 65536), (1, 3), (7, 10))


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _u64(t):
    return t.detach().cpu().numpy().reshape(-1).view(np.uint64)


def _struct(g):
    return _lib.SnerfDsmGrid(**g)


def _same(a, b):
    """two device tensors: the same dtype, shape and bytes"""
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def _check(clouds, g, radius=0, qs=N.QUARTILES, index0s=None):
    """fuse_clouds against the restatement: words, offers, altitudes, indices, stats -> (got, want)"""
    want = N.fuse(clouds, g, radius, qs, index0s)
    got = F.fuse_clouds([_t(np.asarray(c, np.float64).reshape(-1, 3)) for c in clouds], _struct(g), radius, qs, index0s)
    h, w, K = g["out_h"], g["out_w"], len(qs)
    assert tuple(got["words"].shape) == tuple(got["alt"].shape) == tuple(got["index"].shape) == (K, h, w)
    assert tuple(got["offers"].shape) == (h, w) and got["offers"].dtype == torch.int32 and got["alt"].dtype == torch.float32
    assert np.array_equal(_u64(got["words"]).reshape(K, -1), want["words"])
    assert np.array_equal(got["offers"].cpu().numpy().reshape(-1).view(np.uint32), want["offers"].astype(np.uint32))
    assert np.array_equal(_bits(got["alt"].cpu().numpy()), _bits(want["alt"]))
    assert np.array_equal(got["index"].cpu().numpy().reshape(K, -1), want["index"])
    # the count walk and the scatter walk each count their bad and their reaching points; nothing dropped, nothing refused
    assert got["stats"].tolist() == [2 * want["stats"][0], 2 * want["stats"][1], 0, 0]
    return got, want


def _scatter_points(n, g, seed, margin=4.0, zlo=-30.0, zhi=90.0):
    """n points over the window of g and `margin` cells beyond it on every side, altitudes on a 1 cm grid (so many are equal)"""
    rng = np.random.default_rng(seed)
    res = g["res"]
    x0, y1 = g["xoff"] + g["ioff"] * res, g["yoff"] - g["joff"] * res
    x = rng.uniform(x0 - margin * res, x0 + (g["out_w"] + margin) * res, n)
    y = rng.uniform(y1 - (g["out_h"] + margin) * res, y1 + margin * res, n)
    return np.stack([x, y, np.round(rng.uniform(zlo, zhi, n), 2)], 1)


# ---- lattices and radii ---------------------------------------------------------------------------------------------------------------
LATTICES = {
    "1x1": R.grid(500.0, 900.0, 0.5, 1, 1),
    "5x7": R.grid(500.0, 900.0, 0.5, 5, 7),
    "window": R.grid(432000.0, 3352000.0, 0.5, 130, 150, ioff=61, joff=97, out_w=37, out_h=41),
    "clipped": R.grid(500.0, 900.0, 0.5, 6, 5, ioff=-2, joff=3, out_w=5, out_h=4),      # a window that leaves the extent on two sides
}


@pytest.mark.parametrize("radius", (0, 1, 2, 7))
@pytest.mark.parametrize("name", list(LATTICES))
def test_lattices_and_radii(name, radius):
    g = LATTICES[name]
    n = 1500 if radius == 7 else 4000
    clouds = [_scatter_points(n, g, 100 + radius, margin=radius + 2.0), _scatter_points(n // 3, g, 200 + radius, margin=1.0)]
    got, want = _check(clouds, g, radius, FIVE)
    print(name, radius, "offers max", int(want["offers"].max()), "filled", int((want["offers"] > 0).sum()))
    assert 0 < want["stats"][1] < sum(len(c) for c in clouds)              # some points miss the window altogether


# ---- segment lengths: every path of the select ----------------------------------------------------------------------------------------
ONE_CELL = R.grid(10.0, 20.0, 1.0, 3, 2)


def _in_cell(m, seed, i=1, j=0, zlo=-5.0, zhi=5.0):
    rng = np.random.default_rng(seed)
    return np.stack([10.0 + i + rng.uniform(0.01, 0.99, m), 20.0 - j - rng.uniform(0.01, 0.99, m), np.round(rng.uniform(zlo, zhi, m), 2)], 1)


@pytest.mark.parametrize("m", (1, 2, 63, 64, 65, 255, 256, 257, 4097, 20000))
def test_segment_lengths(m):
    got, want = _check([_in_cell(m, m)], ONE_CELL, 0, FIVE)
    assert want["offers"].tolist() == [0, m, 0, 0, 0, 0]
    k = np.sort(np.rint(_in_cell(m, m)[:, 2] / R.Q))
    assert got["alt"][:, 0, 1].tolist() == [float(np.float32(k[N.rank(m, a, b)] * R.Q)) for a, b in FIVE]


def test_empty_single_and_crowded_cells_as_neighbours():
    clouds = [_in_cell(5000, 1, i=1, j=0), _in_cell(1, 2, i=0, j=0), _in_cell(70, 3, i=2, j=1), _in_cell(3000, 4, i=1, j=1)]
    got, want = _check(clouds, ONE_CELL, 0, FIVE)
    assert want["offers"].tolist() == [1, 5000, 0, 0, 3000, 70]
    got, want = _check(clouds, ONE_CELL, 1, N.QUARTILES)                   # radius 1: every cell holds all of its neighbours' points
    assert want["offers"].min() >= 3001


# ---- keys that differ in one byte -----------------------------------------------------------------------------------------------------
def _explicit(ks, indices):
    """one cloud of one point per (quantised altitude, global index) pair, all in cell (1, 0) of ONE_CELL"""
    return [np.array([[11.5, 19.5, k * R.Q]]) for k in ks], [int(i) for i in indices]


def _byte_cases():
    rng = np.random.default_rng(5)
    cases = {}
    for m in (40, 70):                                                     # the short path and the radix select
        j = rng.permutation(m)
        for b in range(4):                                                 # index bytes: equal altitudes, indices differ in byte b only
            cases[f"index-byte{b}-m{m}"] = _explicit([12345] * m, 0x01020304 ^ (j << (8 * b)))
        for b in range(4):                                                 # altitude bytes: k differs in byte b only; indices run against it
            ks = (0x01020304 ^ (j.astype(np.int64) << (8 * b))) - 2 ** 31 if b == 3 else 0x01020304 ^ (j.astype(np.int64) << (8 * b))
            cases[f"altitude-byte{b}-m{m}"] = _explicit(ks, 1000 + np.arange(m))
        cases[f"steps-of-q-m{m}"] = _explicit(-7 + rng.permutation(m), 5 + np.arange(m))                     # 2^-16 m apart
        cases[f"2^15-m-apart-m{m}"] = _explicit(np.where(j % 2 == 0, -2 ** 31, 0), 9 + np.arange(m))           # -32,768 m and 0 m
        cases[f"both-signs-m{m}"] = _explicit(rng.integers(-2 ** 31, 2 ** 31, m), rng.permutation(m) * 3)
        cases[f"range-ends-m{m}"] = _explicit(np.where(j % 3 == 0, 2 ** 31 - 1, np.where(j % 3 == 1, -2 ** 31, j)), np.arange(m))
        cases[f"last-indices-m{m}"] = _explicit(rng.integers(-50, 50, m), 2 ** 32 - 2 - np.arange(m))          # up to index 2^32 - 2
    return cases


BYTE_CASES = _byte_cases()


@pytest.mark.parametrize("name", list(BYTE_CASES))
def test_keys_that_differ_in_one_byte(name):
    clouds, index0s = BYTE_CASES[name]
    got, want = _check(clouds, ONE_CELL, 0, FIVE, index0s)
    assert want["offers"][1] == len(clouds) and len(set(want["words"][:, 1].tolist())) >= 2


def test_index0_near_the_end_of_the_index_range():
    n = 300
    cloud = _in_cell(n, 8, zlo=0.0, zhi=0.05)                              # six altitudes: ties are decided by the index
    got, want = _check([cloud], ONE_CELL, 0, FIVE, [2 ** 32 - 1 - n])
    assert want["index"][:, 1].min() >= 2 ** 32 - 1 - n and want["index"][:, 1].max() <= 2 ** 32 - 2
    with pytest.raises(ValueError, match="index0 \\+ n <= 2\\^32 - 1"):
        F.fuse_clouds([_t(cloud)], _struct(ONE_CELL), 0, FIVE, [2 ** 32 - n])


# ---- bad points -----------------------------------------------------------------------------------------------------------------------
def test_bad_points_are_counted_and_offer_nothing():
    g = R.grid(10.0, 22.0, 0.5, 5, 4)
    good = _scatter_points(600, g, 17, margin=2.0, zlo=-3.0, zhi=3.0)
    bad = np.array([[10.6, 21.9, np.nan], [10.6, 21.9, np.inf], [10.6, 21.9, -np.inf], [10.6, 21.9, 4.0e4], [10.6, 21.9, -4.0e4],
                    [10.6, 21.9, 32768.0], [np.nan, 21.9, 1.0], [10.6, np.inf, 1.0], [-np.inf, 21.9, 1.0], [100.0, 21.9, 9.0],
                    [10.6, 21.9, 32767.9], [10.6, 21.9, -32768.0]])
    cloud = np.concatenate([good[:300], bad, good[300:]])
    for radius in (0, 1):
        got, want = _check([cloud], g, radius, EIGHT)
        assert want["stats"][0] == 6                                       # NaN, +-inf, +-4e4 and 32,768 m: no key
    alone, _ = _check([good], g, 0, FIVE)
    both, _ = _check([good, bad[:10]], g, 0, FIVE)                          # the ten that offer nothing change no word
    assert torch.equal(alone["words"], both["words"]) and torch.equal(alone["offers"], both["offers"])


# ---- quantile sets ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("qs", [((1, 2),), ((1, 1),), EIGHT, ((0, 1),) * 8, ((0, 65536), (65536, 65536), (21845, 65536))], ids=lambda q: f"K{len(q)}-{q[0][0]}")
def test_quantile_sets(qs):
    g = LATTICES["5x7"]
    _check([_scatter_points(6000, g, 23, margin=1.0), _in_cell(0, 1)], g, 1, qs)


def test_the_maximum_plane_is_the_top_surface():
    g = LATTICES["window"]
    clouds = [_scatter_points(5000, g, 31 + k, margin=3.0) for k in range(3)]
    for radius in (0, 2):
        got, _ = _check(clouds, g, radius, ((1, 1), (1, 2)))
        top, at = None, 0
        for c in clouds:
            top, _ = OR.top_surface(_t(c), _struct(g), radius, at, top)
            at += len(c)
        assert torch.equal(got["words"][0], top)
        assert (got["words"][1].view(torch.int64) != top).any()


# ---- order freedom --------------------------------------------------------------------------------------------------------------------
def test_chunking_and_order_do_not_change_a_word():
    g = LATTICES["5x7"]
    clouds = [_scatter_points(n, g, 41 + k, margin=2.0) for k, n in enumerate((300, 1, 250, 77, 400))]
    starts = np.concatenate([[0], np.cumsum([len(c) for c in clouds])[:-1]]).tolist()
    ref, _ = _check(clouds, g, 1, FIVE)
    for chunk in (1, 7, 1000):
        for backwards in (False, True):
            parts, index0s = [], []
            for c, s in zip(clouds, starts):
                for lo in range(0, len(c), chunk):
                    parts.append(_t(c[lo:lo + chunk]))
                    index0s.append(s + lo)
            if backwards:
                parts, index0s = parts[::-1], index0s[::-1]
            got = F.fuse_clouds(parts, _struct(g), 1, FIVE, index0s)
            assert torch.equal(got["words"], ref["words"]) and torch.equal(got["offers"], ref["offers"]), (chunk, backwards)
            assert torch.equal(got["alt"].view(torch.int32), ref["alt"].view(torch.int32)) and torch.equal(got["index"], ref["index"])


# ---- the guard: a scatter walk that differs from the count walk -----------------------------------------------------------------------
SENTINEL = 0x5A5A5A5A5A5A5A5A


def _walks(counted, scattered, g, qs, pad=96):
    """count `counted`, scatter `scattered` into a buffer of exactly `total` words that lies in front of `pad` sentinel words, then the
    select entry itself (fuse.select raises on the counts): -> (words, stats, offsets, cursor, sentinel region, total)"""
    gs = _struct(g)
    count = stats = None
    for c in counted:
        count, stats = F.count_offers(_t(c), gs, 0, count, stats)
    offsets, total = F.offsets_of(count)
    big = torch.full((total + pad,), SENTINEL, dtype=torch.int64, device=DEV)
    keys = big[:total]
    cursor = torch.zeros(count.numel(), dtype=torch.int32, device=DEV)
    at = 0
    for c in scattered:
        F.scatter_keys(_t(c), gs, offsets, cursor, keys, 0, at, stats)
        at += len(c)
    with pytest.raises(ValueError, match=r"offer\(s\) found no slot and \d+ cell\(s\) were refused"):
        F.select(keys, offsets, cursor, qs, g["out_h"], g["out_w"], stats.clone())
    table, K = F.quantile_table(qs)
    words = torch.full((K, g["out_h"], g["out_w"]), SENTINEL, dtype=torch.int64, device=DEV)
    _lib.call("snerf_fuse_select", keys, offsets, total, cursor, count.numel(), table, K, words, stats)
    return words, stats.tolist(), offsets.cpu().numpy(), cursor.cpu().numpy().view(np.uint32), big[total:], total


def test_a_scatter_walk_that_differs_is_counted_never_written_out_of_place():
    g = LATTICES["5x7"]
    a, b = _scatter_points(900, g, 51, margin=0.0), _scatter_points(700, g, 52, margin=0.0)
    extra = _scatter_points(40, g, 53, margin=-1.0)                        # lands in the inner cells only: the border stays good
    cells = g["out_h"] * g["out_w"]
    # one cloud more than was counted
    words, stats, offsets, cursor, tail, total = _walks([a, b], [a, b, extra], g, FIVE)
    m = np.diff(offsets)
    flagged = cursor.astype(np.int64) != m
    assert 0 < flagged.sum() < cells and stats[2] == int((cursor.astype(np.int64) - m)[flagged].sum()) == 40 and stats[3] == int(flagged.sum())
    w = _u64(words).reshape(len(FIVE), cells)
    assert (w[:, flagged] == 0).all() and (tail == SENTINEL).all()
    want = N.fuse([a, b], g, 0, FIVE)["words"]
    assert np.array_equal(w[:, ~flagged], want[:, ~flagged])               # the cells the extra cloud did not touch are right
    # one cloud fewer
    words, stats, offsets, cursor, tail, total = _walks([a, b, extra], [a, b], g, FIVE)
    m = np.diff(offsets)
    flagged = cursor.astype(np.int64) != m
    assert 0 < flagged.sum() < cells and stats[2] == 0 and stats[3] == int(flagged.sum())
    w = _u64(words).reshape(len(FIVE), cells)
    assert (w[:, flagged] == 0).all() and (tail == SENTINEL).all()
    assert np.array_equal(w[:, ~flagged], N.fuse([a, b, extra], g, 0, FIVE)["words"][:, ~flagged])


def test_a_garbage_offsets_table_is_counted():
    """offsets that run backwards, below zero and beyond the buffer: every offer is dropped or stored inside keys[0, capacity), every
    such cell is refused, and the words behind the buffer keep their bytes"""
    g = ONE_CELL
    cloud = np.concatenate([_in_cell(100, 1, i=i, j=j) for j in range(2) for i in range(3)])
    gs = _struct(g)
    capacity = 600
    big = torch.full((capacity + 96,), SENTINEL, dtype=torch.int64, device=DEV)
    offsets = torch.tensor([0, 100, -50, 2 ** 62, 90, 700, 600], dtype=torch.int64, device=DEV)
    cursor = torch.zeros(6, dtype=torch.int32, device=DEV)
    stats = F.scatter_keys(_t(cloud), gs, offsets, cursor, big[:capacity], 0, 0)
    assert cursor.tolist() == [100] * 6 and (big[capacity:] == SENTINEL).all()
    stored = int((big[:capacity] != SENTINEL).sum())
    assert stats.tolist()[2] == 400 and stored == 190                           # cell 0 took [0, 100), cell 4 the slots [90, 190) of its [90, 700)
    table, K = F.quantile_table(FIVE)
    words = torch.full((K, 2, 3), SENTINEL, dtype=torch.int64, device=DEV)
    _lib.call("snerf_fuse_select", big[:capacity], offsets, capacity, cursor, 6, table, K, words, stats)
    w = _u64(words).reshape(K, 6)
    assert stats.tolist()[3] == 5 and (w[:, 1:] == 0).all() and (w[:, 0] != 0).all() and (big[capacity:] == SENTINEL).all()


# ---- no stale bytes ---------------------------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_the_bytes_under_them():
    g = LATTICES["5x7"]
    gs = _struct(g)
    clouds = [_scatter_points(2500, g, 61, margin=1.0), _in_cell(0, 1), _scatter_points(800, g, 62, margin=1.0)]
    cell, key, _ = N.offers(clouds, g, 1)
    want_words, want_count = N.select(cell, key, g["out_h"] * g["out_w"], EIGHT)
    order = np.lexsort((key, cell))
    results = []
    for fill in (0x00, 0xFF, 0x7B):
        count = stats = None
        for c in clouds:
            count, stats = F.count_offers(_t(c), gs, 1, count, stats)
        offsets, total = F.offsets_of(count)
        assert total == len(key)
        keys = torch.empty(total + 50, dtype=torch.int64, device=DEV)
        keys.view(torch.uint8).fill_(fill)
        cursor = torch.zeros(count.numel(), dtype=torch.int32, device=DEV)
        at = 0
        for c in clouds:
            F.scatter_keys(_t(c), gs, offsets, cursor, keys[:total], 1, at, stats)
            at += len(c)
        words = torch.empty((len(EIGHT), g["out_h"], g["out_w"]), dtype=torch.int64, device=DEV)
        words.view(torch.uint8).fill_(fill)
        F.select(keys[:total], offsets, cursor, EIGHT, g["out_h"], g["out_w"], stats, words=words)
        # every slot below the total holds a key: each cell's segment, sorted, is the restatement's list
        off = offsets.cpu().numpy()
        seg = _u64(keys[:total])
        got = np.concatenate([np.sort(seg[off[c]:off[c + 1]]) for c in range(len(off) - 1)])
        assert np.array_equal(got, key[order]) and (keys[total:].view(torch.uint8) == fill).all()
        assert np.array_equal(_u64(words).reshape(len(EIGHT), -1), want_words)
        pl = F.planes(words)
        results.append((words.clone(), pl["alt"], pl["index"]))
    for other in results[1:]:
        assert all(_same(a, b) for a, b in zip(results[0], other))


def test_zero_points_launch_nothing_and_change_nothing():
    gs = _struct(ONE_CELL)
    empty = torch.zeros((0, 3), dtype=torch.float64, device=DEV)
    count, stats = F.count_offers(empty, gs)
    assert not count.any() and not stats.any()
    got = F.fuse_clouds([empty, empty], gs)
    assert not got["words"].any() and not got["offers"].any() and torch.isnan(got["alt"]).all() and (got["index"] == -1).all()


# ---- end to end on the fixture scene ----------------------------------------------------------------------------------------------------
TODAY = {"grid", "dsm", "top_alt", "top_index", "rgb", "n_points", "label_top", "label_vote", "vote_share", "bad_labels", "max_votes",
         "bad_points"}
ADDED = {"median_alt", "median_index", "rgb_median", "label_median", "alt_q1", "alt_q3", "alt_spread", "offers"}


@pytest.fixture(scope="module")
def products(scene):       # noqa: F811
    """one robust walk over the split, one plain walk (with _lib.call's names recorded), and the frames the restatement needs"""
    from snerf_amd.eval.utils.ortho import ortho_products
    from snerf_amd.eval.utils.util import lean_inference
    c, pipe, images, geo = scene
    todo = images[1:]
    frames = []
    torch.manual_seed(SEED)                                    # the renderer jitters the depths: the same draws as the walks under test
    for im in todo:
        res = lean_inference(c, pipe.renderer, pipe.models, im["rays"], im["extras"],
                             keys=("rgb_coarse", "depth_coarse", "semantic_label_coarse"))
        cloud, _ = geo.cloud(im["rays"], res["depth_coarse"])
        frames.append({"xyz": cloud.cpu().numpy(), "rgb": res["rgb_coarse"].cpu().numpy(), "labels": res["semantic_label_coarse"].cpu().numpy()})
    called = []
    real = _lib.call

    def recording(name, *a, **kw):
        called.append(name)
        return real(name, *a, **kw)
    _lib.call = recording
    try:
        torch.manual_seed(SEED)
        plain = ortho_products(c, pipe.renderer, pipe.models, todo, geo=geo, radius=1)
        plain_calls = list(called)
        del called[:]
        torch.manual_seed(SEED)
        robust = ortho_products(c, pipe.renderer, pipe.models, todo, geo=geo, radius=1, robust=True)
        robust_calls = list(called)
    finally:
        _lib.call = real
    return {"plain": plain, "plain_calls": plain_calls, "robust": robust, "robust_calls": robust_calls, "frames": frames}


def test_without_robust_nothing_new_is_called_or_returned(products):
    plain, robust = products["plain"], products["robust"]
    assert set(plain) == TODAY and set(robust) == TODAY | ADDED
    assert not [n for n in products["plain_calls"] if n.startswith("snerf_fuse")] and "snerf_ortho_top" in products["plain_calls"]
    n = len(products["frames"])
    assert [products["robust_calls"].count(s) for s in ("snerf_fuse_count", "snerf_fuse_scatter", "snerf_fuse_select")] == [n, n, 1]
    for key in TODAY - {"grid", "n_points", "bad_labels", "max_votes", "bad_points"}:      # the shared products keep their bytes
        assert _same(plain[key], robust[key]), key
    assert all(plain[k] == robust[k] for k in ("grid", "n_points", "bad_labels", "max_votes", "bad_points"))


def test_robust_products_of_the_fixture_scene_equal_the_restatement(products):
    prod, frames = products["robust"], products["frames"]
    grid = prod["grid"]
    g = R.grid(grid.xoff, grid.yoff, grid.resolution, grid.xsize, grid.ysize)
    h, w = grid.ysize, grid.xsize
    want = N.fuse([f["xyz"] for f in frames], g, 1, N.QUARTILES)
    for key, plane in (("alt_q1", 0), ("median_alt", 1), ("alt_q3", 2)):
        assert prod[key].dtype == torch.float32 and np.array_equal(_bits(prod[key].cpu().numpy()), _bits(want["alt"][plane])), key
    assert np.array_equal(prod["median_index"].cpu().numpy().reshape(-1), want["index"][1])
    assert np.array_equal(prod["offers"].cpu().numpy().reshape(-1).view(np.uint32), want["offers"].astype(np.uint32))
    assert np.array_equal(_bits(prod["alt_spread"].cpu().numpy()), _bits(N.spread(want["words"][0], want["words"][2])))
    # colour and label: the frames' values at the median point
    idx = want["index"][1]
    full = idx >= 0
    rgb = np.concatenate([f["rgb"] for f in frames])
    labels = np.concatenate([f["labels"] for f in frames])
    want_rgb = np.full((3, h * w), np.nan, np.float32)
    want_rgb[:, full] = rgb[idx[full]].T
    want_label = np.full(h * w, 255, np.uint8)
    want_label[full] = labels[idx[full]]
    assert np.array_equal(_bits(prod["rgb_median"].cpu().numpy()), _bits(want_rgb))
    assert np.array_equal(prod["label_median"].cpu().numpy().reshape(-1), want_label)
    # against the top surface of the same walk
    top, med, offers = (prod[k].cpu().numpy().reshape(-1) for k in ("top_alt", "median_alt", "offers"))
    assert full.any() and (~full).any() and np.array_equal(np.isfinite(top), full) and np.array_equal(np.isfinite(med), full)
    assert (top[full] >= med[full]).all()
    assert np.array_equal(_bits(top[offers == 1]), _bits(med[offers == 1]))
    assert np.array_equal(prod["top_index"].cpu().numpy().reshape(-1)[offers == 1], idx[offers == 1])
    q1, q3 = prod["alt_q1"].cpu().numpy().reshape(-1), prod["alt_q3"].cpu().numpy().reshape(-1)
    assert (q1[full] <= med[full]).all() and (med[full] <= q3[full]).all() and (prod["alt_spread"].cpu().numpy().reshape(-1)[full] >= 0).all()
    print("grid", tuple(grid), "offers max", int(offers.max()), "filled", int(full.sum()), "cells where median < top", int((top[full] > med[full]).sum()),
          "cells of one offer", int((offers == 1).sum()))


def test_export_ortho_robust_writes_the_fused_files_and_scores_three_surfaces(scene, tmp_path):      # noqa: F811
    from snerf_amd.eval.ortho import export_ortho
    from snerf_amd.eval.utils import dsm as D
    from snerf_amd.framework.util import img_utils as I
    c, pipe, images, geo = scene
    d = os.path.join(ROOT, "tests", "golden", "scene_small_dsm", "dsm")
    truth = I.load_dsm_ground_truth(os.path.join(d, "JAX_068_DSM.tif"), os.path.join(d, "JAX_068_DSM.txt"), os.path.join(d, "JAX_068_CLS.tif"))
    roi = D.roi_grid(truth["roi"])
    torch.manual_seed(SEED)
    prod = export_ortho(c, pipe.renderer, pipe.models, images, str(tmp_path), geo=geo, roi=roi, robust=True, gt=truth["gt"].to(DEV),
                        water_mask=truth["water_mask"].to(DEV))
    stems = ["rgb", "label_top", "label_vote", "top_alt", "dsm", "vote_share", "median_alt", "alt_spread", "offers", "rgb_median", "label_median"]
    names = {s + e for s in stems for e in (".png", ".tif")} | {"fused_eval.json"}
    assert set(prod["files"]) == names == set(os.listdir(tmp_path / "ortho" / "test"))
    assert prod["grid"] == roi and tuple(prod["median_alt"].shape) == (roi.ysize, roi.xsize)
    tf = (roi.xoff, roi.yoff, roi.resolution, roi.resolution)
    for key in ("median_alt", "alt_spread"):
        a, got_tf = I.load_dsm_geotiff(prod["files"][key + ".tif"])
        assert a.dtype == np.float32 and got_tf == tf and np.array_equal(_bits(a), _bits(prod[key].cpu().numpy())), key
    a, _ = I.load_dsm_geotiff(prod["files"]["offers.tif"])
    assert np.array_equal(a, prod["offers"].cpu().numpy().astype(np.float32))
    a, _ = I.load_dsm_geotiff(prod["files"]["label_median.tif"])
    assert a.dtype == np.uint8 and np.array_equal(a, prod["label_median"].cpu().numpy())
    with open(prod["files"]["fused_eval.json"]) as f:
        doc = json.load(f)
    assert sorted(doc) == ["mae"] and sorted(doc["mae"]) == ["dsm", "median_alt", "top_alt"]
    assert all(sorted(v) == ["mean", "median"] and all(isinstance(x, float) for x in v.values()) for v in doc["mae"].values())
    assert json.dumps(doc["mae"], sort_keys=True) == json.dumps(prod["mae"], sort_keys=True)       # (a NaN would not equal itself)
    print("altitude MAE of the untrained model on the ROI (mean, median; no bar):",
          {k: (round(v["mean"], 3), round(v["median"], 3)) for k, v in doc["mae"].items()}, "filled", int((prod["offers"] > 0).sum()))
    # without robust the export is what it was, and a ground truth without robust is refused
    with pytest.raises(ValueError, match="needs robust=True"):
        export_ortho(c, pipe.renderer, pipe.models, images, str(tmp_path / "x"), geo=geo, roi=roi, gt=truth["gt"].to(DEV))
