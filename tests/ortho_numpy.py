"""NumPy restatement of the ortho products (tests only), written from the ortho section of include/snerf_hip.h: the lattice of the DSM
rasteriser, the 64-bit top-surface key in Python / NumPy integer arithmetic, the gather of the winners' payloads and the label
votes.  Two forms of each accumulating stage: a plain loop over points and window cells (Python ints, the spec read aloud) and
a vectorised one on np.maximum.at / np.add.at for the larger cases; tests/test_ortho_cpu.py holds the two to each other, the
GPU tests hold the kernels to them bit for bit.  np.rint on the fp64 quotient rounds ties to even, as llrint does."""
import math

import numpy as np

Z0 = 0.0
Q = 2.0 ** -16
NO_LABEL = 255
_M32 = 0xFFFFFFFF


def grid(xoff, yoff, res, xsize, ysize, ioff=0, joff=0, out_w=None, out_h=None):
    """the fields of SnerfDsmGrid as a dict; the window defaults to the whole extent"""
    return dict(xoff=float(xoff), yoff=float(yoff), res=float(res), xsize=int(xsize), ysize=int(ysize), ioff=int(ioff),
                joff=int(joff), out_w=int(xsize if out_w is None else out_w), out_h=int(ysize if out_h is None else out_h))


def encode(k, index):
    """the key of quantised altitude k in [-2^31, 2^31) and global point index in [0, 2^32 - 2]"""
    k, index = int(k), int(index)
    assert -2 ** 31 <= k < 2 ** 31 and 0 <= index <= 2 ** 32 - 2
    return ((k + 2 ** 31) << 32) | (_M32 - index)


def decode(key):
    """key -> (k, index); None for 0 (no point)"""
    key = int(key)
    if key == 0:
        return None
    return (key >> 32) - 2 ** 31, _M32 - (key & _M32)


def quantise(z, z0=Z0, q=Q):
    """(k as float64, ok): k = rint((z - z0)/q); ok where it is finite and inside [-2^31, 2^31)"""
    with np.errstate(invalid="ignore", over="ignore"):
        kq = np.rint((np.asarray(z, np.float64) - z0) / q)
        ok = (kq >= -2.0 ** 31) & (kq < 2.0 ** 31)
    return kq, ok


def _cells(xyz, g):
    with np.errstate(invalid="ignore", over="ignore"):
        return np.floor((xyz[:, 0] - g["xoff"]) / g["res"]), np.floor((g["yoff"] - xyz[:, 1]) / g["res"])


def _bounds(g):
    lo_i, hi_i = max(g["ioff"], 0), min(g["ioff"] + g["out_w"], g["xsize"])
    lo_j, hi_j = max(g["joff"], 0), min(g["joff"] + g["out_h"], g["ysize"])
    return lo_i, hi_i, lo_j, hi_j


def _offered(fi, fj, g, radius):
    """window cell indices a point with cell (fi, fj) (floats, maybe NaN / inf) offers itself to -- the loop form"""
    if not (math.isfinite(fi) and math.isfinite(fj)):
        return []
    lo_i, hi_i, lo_j, hi_j = _bounds(g)
    if not (fi + radius >= lo_i and fi - radius < hi_i and fj + radius >= lo_j and fj - radius < hi_j):
        return []
    ci, cj = int(fi), int(fj)
    out = []
    for ky in range(-radius, radius + 1):
        for kx in range(-radius, radius + 1):
            li, lj = ci + kx, cj + ky
            if lo_i <= li < hi_i and lo_j <= lj < hi_j:
                out.append((lj - g["joff"]) * g["out_w"] + (li - g["ioff"]))
    return out


def top_loop(xyz, g, radius=0, index0=0, z0=Z0, q=Q, top=None, stats=None):
    """snerf_ortho_top, point by point: top (cells,) uint64 and stats (4,) uint64, both accumulated when given"""
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    cells = g["out_h"] * g["out_w"]
    top = [0] * cells if top is None else [int(v) for v in top]
    stats = [0] * 4 if stats is None else [int(v) for v in stats]
    assert index0 >= 0 and index0 + len(xyz) <= 2 ** 32 - 1
    kq, ok = quantise(xyz[:, 2], z0, q)
    fi, fj = _cells(xyz, g)
    for p in range(len(xyz)):
        if not ok[p]:
            stats[0] += 1
            continue
        cs = _offered(float(fi[p]), float(fj[p]), g, radius)
        if not cs:
            continue
        key = encode(int(kq[p]), index0 + p)
        for c in cs:
            top[c] = max(top[c], key)
        stats[1] += 1
    return np.array(top, np.uint64), np.array(stats, np.uint64)


def _window_cells(fi, fj, g, radius):
    """vectorised: (point rows, window cell indices) of every offer, over the points whose (fi, fj) are finite"""
    lo_i, hi_i, lo_j, hi_j = _bounds(g)
    fin = np.isfinite(fi) & np.isfinite(fj)
    rows, cells = [], []
    for ky in range(-radius, radius + 1):
        for kx in range(-radius, radius + 1):
            with np.errstate(invalid="ignore"):
                li, lj = fi + kx, fj + ky
                m = fin & (li >= lo_i) & (li < hi_i) & (lj >= lo_j) & (lj < hi_j)
            r = np.nonzero(m)[0]
            rows.append(r)
            cells.append(((lj[r] - g["joff"]) * g["out_w"] + (li[r] - g["ioff"])).astype(np.int64))
    return np.concatenate(rows), np.concatenate(cells)


def top_at(xyz, g, radius=0, index0=0, z0=Z0, q=Q, top=None, stats=None):
    """snerf_ortho_top on np.maximum.at"""
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    cells = g["out_h"] * g["out_w"]
    top = np.zeros(cells, np.uint64) if top is None else np.array(top, np.uint64)
    stats = np.zeros(4, np.uint64) if stats is None else np.array(stats, np.uint64)
    n = len(xyz)
    assert index0 >= 0 and index0 + n <= 2 ** 32 - 1
    kq, ok = quantise(xyz[:, 2], z0, q)
    fi, fj = _cells(xyz, g)
    fi, fj = np.where(ok, fi, np.nan), np.where(ok, fj, np.nan)
    ku = (np.where(ok, kq, 0.0).astype(np.int64) + 2 ** 31).astype(np.uint64)
    keys = (ku << np.uint64(32)) | (np.uint64(_M32) - (np.uint64(index0) + np.arange(n, dtype=np.uint64)))
    rows, cs = _window_cells(fi, fj, g, radius)
    np.maximum.at(top, cs, keys[rows])
    stats[0] += np.uint64(int((~ok).sum()))
    stats[1] += np.uint64(len(np.unique(rows)))
    return top, stats


def gather(top, index0, n, z0=Z0, q=Q, rgb=None, labels=None, scalar=None, out=None):
    """snerf_ortho_gather: {"alt" f32, "index" i64[, "rgb" (3, cells) f32, "label" u8, "scalar" f32]}; payload arrays of `out`
    (the caller's pre-filled buffers) are written only where the winner's index lies in [index0, index0 + n)"""
    top = np.asarray(top, np.uint64)
    cells = top.size
    out = {} if out is None else {k: np.array(v) for k, v in out.items()}
    alt, idx = np.full(cells, np.nan, np.float32), np.full(cells, -1, np.int64)
    if rgb is not None:
        out.setdefault("rgb", np.full((3, cells), np.nan, np.float32))
        rgb = np.asarray(rgb, np.float32).reshape(-1, 3)
    if labels is not None:
        out.setdefault("label", np.full(cells, NO_LABEL, np.uint8))
    if scalar is not None:
        out.setdefault("scalar", np.full(cells, np.nan, np.float32))
    for c in range(cells):
        d = decode(top[c])
        if d is None:
            continue
        k, i = d
        alt[c] = np.float32(z0 + q * float(k))
        idx[c] = i
        row = i - index0
        if not 0 <= row < n:
            continue
        if rgb is not None:
            out["rgb"][:, c] = rgb[row]
        if labels is not None:
            l = int(labels[row])
            out["label"][c] = l if 0 <= l <= 254 else NO_LABEL
        if scalar is not None:
            out["scalar"][c] = np.float32(scalar[row])
    if n > 0:
        out["alt"], out["index"] = alt, idx
    return out


def votes_loop(xyz, labels, g, n_classes, radius=0, votes=None, stats=None):
    """snerf_ortho_votes, point by point: votes (n_classes, cells) uint32, stats (4,) uint64"""
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    cells = g["out_h"] * g["out_w"]
    votes = np.zeros((n_classes, cells), np.uint32) if votes is None else np.array(votes, np.uint32).reshape(n_classes, cells)
    stats = [0] * 4 if stats is None else [int(v) for v in stats]
    fi, fj = _cells(xyz, g)
    for p in range(len(xyz)):
        l = int(labels[p])
        if not 0 <= l < n_classes or not (math.isfinite(xyz[p, 0]) and math.isfinite(xyz[p, 1])):
            stats[0] += 1
            continue
        for c in _offered(float(fi[p]), float(fj[p]), g, radius):
            votes[l, c] += 1
    return votes, np.array(stats, np.uint64)


def votes_at(xyz, labels, g, n_classes, radius=0, votes=None, stats=None):
    """snerf_ortho_votes on np.add.at"""
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    labels = np.asarray(labels, np.int64).reshape(-1)
    cells = g["out_h"] * g["out_w"]
    votes = np.zeros((n_classes, cells), np.uint32) if votes is None else np.array(votes, np.uint32).reshape(n_classes, cells)
    stats = np.zeros(4, np.uint64) if stats is None else np.array(stats, np.uint64)
    ok = (labels >= 0) & (labels < n_classes) & np.isfinite(xyz[:, 0]) & np.isfinite(xyz[:, 1])
    fi, fj = _cells(xyz, g)
    fi, fj = np.where(ok, fi, np.nan), np.where(ok, fj, np.nan)
    rows, cs = _window_cells(fi, fj, g, radius)
    np.add.at(votes.reshape(-1), labels[rows] * cells + cs, np.uint32(1))
    stats[0] += np.uint64(int((~ok).sum()))
    return votes, stats


def votes_finish(votes, stats=None):
    """snerf_ortho_votes_finish: (label u8 -- the lowest class among the maxima, 255 when empty --, share f32, stats)"""
    votes = np.asarray(votes, np.uint32)
    stats = np.zeros(4, np.uint64) if stats is None else np.array(stats, np.uint64)
    total = votes.astype(np.uint64).sum(0)
    best = votes.max(0)
    label = np.where(total > 0, votes.argmax(0), NO_LABEL).astype(np.uint8)       # argmax: the first (lowest) maximum
    with np.errstate(invalid="ignore", divide="ignore"):
        share = np.where(total > 0, best.astype(np.float64) / total.astype(np.float64), np.nan).astype(np.float32)
    stats[1] = max(int(stats[1]), int(total.max()) if total.size else 0)
    return label, share, stats
