"""NumPy restatement of the fused altitude quantiles (tests only), written from include/snerf_fuse.h: for every point the cells of
tests/ortho_numpy.py (cell_window's arithmetic in fp64) and its 64-bit key, per cell the sorted list of its keys, the word at rank
((m - 1) num) // den, the offers and the spread.  Two forms: a plain loop over points and cells on Python ints (the spec read aloud)
and a vectorised one for the larger cases; tests/test_fuse_cpu.py holds the two to each other, the GPU tests hold the kernels to
them bit for bit."""
import numpy as np

from tests import ortho_numpy as R

Z0, Q = R.Z0, R.Q
QUARTILES = ((1, 4), (1, 2), (3, 4))
_M32 = 0xFFFFFFFF


def rank(m, num, den):
    """the 0-based rank of quantile num / den among m sorted values: numpy's method="lower\""""
    assert m >= 1 and 1 <= den <= 65536 and 0 <= num <= den
    return ((m - 1) * num) // den


def offers_loop(clouds, g, radius=0, index0s=None, z0=Z0, q=Q):
    """point by point: (lists: per cell the Python-int keys in arrival order, stats [bad altitudes, points that reached a cell])"""
    cells = g["out_h"] * g["out_w"]
    lists = [[] for _ in range(cells)]
    stats = [0, 0]
    at = 0
    for n, xyz in enumerate(clouds):
        xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
        index0 = at if index0s is None else index0s[n]
        at += len(xyz)
        kq, ok = R.quantise(xyz[:, 2], z0, q)
        fi, fj = R._cells(xyz, g)
        for p in range(len(xyz)):
            if not ok[p]:
                stats[0] += 1
                continue
            cs = R._offered(float(fi[p]), float(fj[p]), g, radius)
            if not cs:
                continue
            key = R.encode(int(kq[p]), index0 + p)
            for c in cs:
                lists[c].append(key)
            stats[1] += 1
    return lists, stats


def select_loop(lists, quantiles):
    """words (K, cells) uint64: per cell the sorted list's entry at rank(m, num, den), 0 for an empty cell"""
    words = np.zeros((len(quantiles), len(lists)), np.uint64)
    for c, keys in enumerate(lists):
        if keys:
            s = sorted(keys)
            for k, (num, den) in enumerate(quantiles):
                words[k, c] = s[rank(len(s), num, den)]
    return words


def offers(clouds, g, radius=0, index0s=None, z0=Z0, q=Q):
    """vectorised: (cell (T,) int64, key (T,) uint64 of every offer, stats [bad altitudes, points that reached a cell])"""
    cell, key, stats, at = [], [], [0, 0], 0
    for n, xyz in enumerate(clouds):
        xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
        index0 = at if index0s is None else index0s[n]
        at += len(xyz)
        assert index0 >= 0 and index0 + len(xyz) <= 2 ** 32 - 1
        kq, ok = R.quantise(xyz[:, 2], z0, q)
        fi, fj = R._cells(xyz, g)
        fi, fj = np.where(ok, fi, np.nan), np.where(ok, fj, np.nan)
        ku = (np.where(ok, kq, 0.0).astype(np.int64) + 2 ** 31).astype(np.uint64)
        keys = (ku << np.uint64(32)) | (np.uint64(_M32) - (np.uint64(index0) + np.arange(len(xyz), dtype=np.uint64)))
        rows, cs = R._window_cells(fi, fj, g, radius)
        cell.append(cs)
        key.append(keys[rows])
        stats[0] += int((~ok).sum())
        stats[1] += len(np.unique(rows))
    return np.concatenate(cell).astype(np.int64), np.concatenate(key).astype(np.uint64), stats


def select(cell, key, cells, quantiles):
    """words (K, cells) uint64 and offers (cells,) int64 from the offers' (cell, key) pairs"""
    order = np.lexsort((key, cell))                            # by cell, ascending keys inside a cell
    cell, key = cell[order], key[order]
    count = np.bincount(cell, minlength=cells).astype(np.int64)
    start = np.concatenate([[0], np.cumsum(count)[:-1]])
    words = np.zeros((len(quantiles), cells), np.uint64)
    full = count > 0
    for k, (num, den) in enumerate(quantiles):
        assert 1 <= den <= 65536 and 0 <= num <= den
        r = ((count[full] - 1) * num) // den
        words[k, full] = key[start[full] + r]
    return words, count


def decode(words, z0=Z0, q=Q):
    """snerf_ortho_gather's reading of a plane of words: (alt f32, NaN where 0; index int64, -1 where 0)"""
    words = np.asarray(words, np.uint64)
    k = (words >> np.uint64(32)).astype(np.int64) - 2 ** 31
    alt = (z0 + q * k.astype(np.float64)).astype(np.float32)
    idx = (np.uint64(_M32) - (words & np.uint64(_M32))).astype(np.int64)
    empty = words == 0
    return np.where(empty, np.float32(np.nan), alt), np.where(empty, np.int64(-1), idx)


def spread(words_lo, words_hi, q=Q):
    """q (k_hi - k_lo) as f32, exact in the integers; NaN where either word is 0"""
    lo, hi = np.asarray(words_lo, np.uint64), np.asarray(words_hi, np.uint64)
    d = (hi >> np.uint64(32)).astype(np.int64) - (lo >> np.uint64(32)).astype(np.int64)
    return np.where((lo == 0) | (hi == 0), np.float32(np.nan), (d.astype(np.float64) * q).astype(np.float32))


def fuse(clouds, g, radius=0, quantiles=QUARTILES, index0s=None, z0=Z0, q=Q):
    """the whole feature: {"words" (K, cells) u64, "offers" (cells,) int64, "alt" (K, cells) f32, "index" (K, cells) int64, "stats"}"""
    cells = g["out_h"] * g["out_w"]
    cell, key, stats = offers(clouds, g, radius, index0s, z0, q)
    words, count = select(cell, key, cells, quantiles)
    alt, idx = decode(words, z0, q)
    return {"words": words, "offers": count, "alt": alt, "index": idx, "stats": stats}
