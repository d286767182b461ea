"""numpy restatement of the objects entries, written from include/snerf_objects.h (never from csrc/objects.hip): the oracle of
tests/test_gpu_objects.py.  `link` is a sequential union-find, `rows` plain loops over Python ints (no sum can overflow); neither is
fast, and neither is meant to be."""
import numpy as np

Z0 = 0.0
Q = 2.0 ** -16
NO_LABEL = 255
ROW_WORDS = 16
U64_MAX = 2 ** 64 - 1
BIAS = 2 ** 31
ROW_INIT = [0, 0, 0, U64_MAX, 0, U64_MAX, 0, 0, 0, U64_MAX, 0, 0, 0, U64_MAX, 0, 0]


def table(classes):
    """the 256-byte class table of a set of classes"""
    t = np.zeros(256, np.uint8)
    for c in classes:
        if not 0 <= int(c) < NO_LABEL:
            raise ValueError(f"class {c} outside [0, 255)")
        t[int(c)] = 1
    return t


def link(label, classes, connectivity=4):
    """-> (parent (h * w) int32, stats [0, member cells]): -1 off the classes, else the smallest index of the cell's component"""
    if connectivity not in (4, 8):
        raise ValueError("connectivity must be 4 or 8")
    label = np.asarray(label, np.uint8)
    h, w = label.shape
    member = table(classes)
    lab = label.reshape(-1).tolist()
    parent = [c if member[lab[c]] else -1 for c in range(h * w)]

    def find(a):
        while parent[a] != a:
            a = parent[a]
        return a

    def unite(a, b):
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)

    for c in range(h * w):
        if parent[c] < 0:
            continue
        j, i = divmod(c, w)
        if i > 0 and lab[c - 1] == lab[c]:
            unite(c, c - 1)
        if j > 0:
            if lab[c - w] == lab[c]:
                unite(c, c - w)
            if connectivity == 8 and i > 0 and lab[c - w - 1] == lab[c]:
                unite(c, c - w - 1)
            if connectivity == 8 and i + 1 < w and lab[c - w + 1] == lab[c]:
                unite(c, c - w + 1)
    out = np.array([find(c) if parent[c] >= 0 else -1 for c in range(h * w)], np.int32).reshape(-1)
    return out, [0, int((out >= 0).sum())]


def ids_of(parent, h, w):
    """-> (ids (h, w) int32, K): 0 = background, 1..K in the raster order of the roots"""
    parent = np.asarray(parent).reshape(-1)
    is_root = parent == np.arange(parent.size)
    rank = np.cumsum(is_root)
    ids = np.where(parent < 0, 0, rank[np.maximum(parent, 0)]).astype(np.int32)
    return ids.reshape(h, w), int(is_root.sum())


def quantise(alt, z0=Z0, q=Q):
    """k = rint((alt - z0) / q) of one f32 altitude as a Python int, or None when it is not in [-2^31, 2^31)"""
    with np.errstate(all="ignore"):
        kq = np.rint((np.float64(np.float32(alt)) - np.float64(z0)) / np.float64(q))
    if not (kq >= -2147483648.0 and kq < 2147483648.0):
        return None
    return int(kq)


def new_rows(K):
    return [list(ROW_INIT) for _ in range(K)]


def rows_loop(ids, K, label, alt, ground, ring=2, z0=Z0, q=Q, band=None, rows=None, stats=None):
    """-> (rows: K lists of 16 Python ints in [0, 2^64), stats [4]); `band` = (row0, row1), default the whole raster; `rows` /
    `stats`: accumulators of earlier calls"""
    ids, label, alt = np.asarray(ids), np.asarray(label, np.uint8), np.asarray(alt, np.float32)
    h, w = ids.shape
    gtab = table(ground)
    rows = new_rows(K) if rows is None else rows
    stats = [0, 0, 0, 0] if stats is None else stats
    row0, row1 = (0, h) if band is None else band
    ks = [[quantise(alt[j, i], z0, q) for i in range(w)] for j in range(h)]
    for j in range(row0, row1):
        for i in range(w):
            n = int(ids[j, i])
            if n < 0 or n > K:
                stats[2] += 1
                continue
            if n == 0:
                continue
            r = rows[n - 1]
            r[0] += 1
            r[1] += i
            r[2] += j
            r[3], r[4], r[5], r[6] = min(r[3], i), max(r[4], i), min(r[5], j), max(r[6], j)
            k = ks[j][i]
            if k is None:
                stats[0 if np.isfinite(alt[j, i]) else 1] += 1
            else:
                r[7] += 1
                r[8] += k
                r[9], r[10] = min(r[9], k + BIAS), max(r[10], k + BIAS)
            for dj, di in ((0, -1), (0, 1), (-1, 0), (1, 0)):
                nj, ni = j + dj, i + di
                if nj < 0 or nj >= h or ni < 0 or ni >= w or int(ids[nj, ni]) != n:
                    r[14] += 1
            r[15] = max(r[15], int(label[j, i]))
            if ring > 0:
                for gj in range(max(j - ring, 0), min(j + ring + 1, h)):
                    for gi in range(max(i - ring, 0), min(i + ring + 1, w)):
                        if int(ids[gj, gi]) != 0 or not gtab[label[gj, gi]] or ks[gj][gi] is None:
                            continue
                        r[11] += 1
                        r[12] += ks[gj][gi]
                        r[13] = min(r[13], ks[gj][gi] + BIAS)
                        stats[3] += 1
    return rows, stats


def words(rows):
    """rows of Python ints (signed sums may be negative) -> (K, 16) uint64, two's complement"""
    return np.array([[v % 2 ** 64 for v in r] for r in rows], np.uint64).reshape(len(rows), ROW_WORDS)


# ---- the rasters the CPU and the GPU tests share --------------------------------------------------------------------------------------
RANDOM_SHAPES = [(1, 1), (1, 130), (130, 1), (7, 65), (33, 64), (70, 129)]


def random_label(h, w, seed=0):
    rng = np.random.default_rng(1000 * h + w + seed)
    return np.array([0, 3, 4, 255], np.uint8)[rng.integers(0, 4, (h, w))]


def serpentine(h=33, w=67, cls=3):
    """full rows at even j, joined alternately at the east and the west end: one component, one long chain"""
    out = np.zeros((h, w), np.uint8)
    out[0::2] = cls
    for j in range(1, h, 2):
        out[j, w - 1 if (j // 2) % 2 == 0 else 0] = cls
    return out


def spiral(n=65, cls=3):
    """a square spiral: walk from the north-west corner, a step ahead is free while it stays inside, off the path and one cell clear
    of it; else turn right; stop at two turns in a row"""
    on = np.zeros((n, n), bool)
    on[0, 0] = True
    j = i = 0
    dj, di, turns = 0, 1, 0

    def is_on(jj, ii):
        return 0 <= jj < n and 0 <= ii < n and on[jj, ii]

    while turns < 2:
        nj, ni = j + dj, i + di
        if 0 <= nj < n and 0 <= ni < n and not on[nj, ni] and not is_on(nj + dj, ni + di):
            j, i, turns = nj, ni, 0
            on[j, i] = True
        else:
            dj, di, turns = di, -dj, turns + 1
    return np.where(on, cls, 0).astype(np.uint8)


def checkerboard(h=16, w=70, cls=3):
    jj, ii = np.mgrid[0:h, 0:w]
    return np.where((ii + jj) % 2 == 0, cls, 0).astype(np.uint8)


def one_class(h=64, w=256, cls=3):
    return np.full((h, w), cls, np.uint8)


def comb(h=40, w=129, cls=4):
    """teeth in every second column that meet only in the last row"""
    out = np.zeros((h, w), np.uint8)
    out[:, 0::2] = cls
    out[h - 1] = cls
    return out


def alternating_columns(h=20, w=66):
    out = np.full((h, w), 3, np.uint8)
    out[:, 1::2] = 4
    return out


def structured():
    return {"serpentine": serpentine(), "spiral": spiral(), "checkerboard": checkerboard(), "one_class": one_class(), "comb": comb(),
            "alternating_columns": alternating_columns(), "no_member": np.full((9, 70), NO_LABEL, np.uint8)}


def town(shift=0):
    """the synthetic town of the tests: 96 x 130 cells, ground class 0 at 3.0 m, three class-3 boxes and a 2 x 2 class-4 blob; `shift`
    moves everything `shift` columns east.  -> (label u8, alt f32, boxes [(j0, i0, rows, cols, altitude)])"""
    h, w = 96, 130
    label, alt = np.zeros((h, w), np.uint8), np.full((h, w), 3.0, np.float32)
    boxes = [(10, 12, 10, 12, 9.0), (12, 60, 17, 9, 15.5), (50, 40, 24, 30, 23.0)]
    for j0, i0, nj, ni, z in boxes:
        label[j0:j0 + nj, i0 + shift:i0 + shift + ni] = 3
        alt[j0:j0 + nj, i0 + shift:i0 + shift + ni] = z
    label[80:82, 100 + shift:102 + shift] = 4
    alt[80:82, 100 + shift:102 + shift] = 4.5
    return label, alt, [(j0, i0 + shift, nj, ni, z) for j0, i0, nj, ni, z in boxes]
