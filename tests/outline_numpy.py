"""numpy restatement of the outline entries, written from include/snerf_outline.h (never from csrc/outline.hip): the oracle of
tests/test_gpu_outline.py.  Everything is given twice: `trace` states every entry over whole arrays (the pointer jumping of
snerf_outline_rank round by round), `walk` builds the edges by plain loops, takes a corner to be an edge whose predecessor has another
heading, and follows `next` from each ring's lowest edge.  tests/test_outline_cpu.py holds the two to each other bit for bit."""
import numpy as np

from tests import objects_numpy as ON

ROW_WORDS = 8
U64_MAX = 2 ** 64 - 1
ROW_INIT = [0, 0, 0, 0, U64_MAX, 0, U64_MAX, 0]
CORNER = 1
NIL = -1
STEP = [(0, 1), (1, 0), (0, -1), (-1, 0)]          # E, S, W, N in (row, column)
TAIL = [(0, 0), (1, 0), (1, 1), (0, 1)]            # (dx, dy) of the tail of side N, E, S, W from the cell's (i, j)
POPCOUNT = np.array([bin(k).count("1") for k in range(16)], np.int64)


def normalised(ids, K):
    ids = np.asarray(ids, np.int64)
    return np.where((ids < 0) | (ids > K), 0, ids)


def _shifted(P, h, w, dj, di):
    return P[1 + dj:1 + dj + h, 1 + di:1 + di + w]


# ---- entry by entry, over whole arrays --------------------------------------------------------------------------------------------------
def sides(ids, K):
    """-> (sides (h * w) u8, stats [bad ids, object cells, edges, corners])"""
    raw = np.asarray(ids, np.int64)
    h, w = raw.shape
    n = normalised(raw, K)
    P = np.pad(n, 1)
    mask = np.zeros((h, w), np.int64)
    corners = 0
    for s in range(4):
        oj, oi = STEP[(s + 3) % 4]
        exists = (n > 0) & (_shifted(P, h, w, oj, oi) != n)
        mask |= exists.astype(np.int64) << s
        corners += int((exists & _corner(P, n, h, w, s)).sum())
    return mask.reshape(-1).astype(np.uint8), [int(((raw < 0) | (raw > K)).sum()), int((n > 0).sum()), int(POPCOUNT[mask].sum()), corners]


def _corner(P, n, h, w, d):
    rj, ri = -STEP[d][0], -STEP[d][1]
    lj, li = rj + STEP[(d + 3) % 4][0], ri + STEP[(d + 3) % 4][1]
    return ~((_shifted(P, h, w, rj, ri) == n) & (_shifted(P, h, w, lj, li) != n))


def offsets_of(side_bits):
    """the exclusive cumulative sum of popcount(sides) -> (offsets (h * w) int32, E)"""
    counts = POPCOUNT[np.asarray(side_bits, np.int64)]
    total = np.cumsum(counts)
    return (total - counts).astype(np.int32), int(total[-1]) if len(total) else 0


def link(ids, side_bits, offsets, K, connectivity, E, fill=0):
    """-> (slot, next, flags (E) int32 -- `fill` where nothing is written --, stats [guard trips, edges written])"""
    if connectivity not in (4, 8):
        raise ValueError("connectivity must be 4 or 8")
    h, w = np.asarray(ids).shape
    n = normalised(ids, K)
    P = np.pad(n, 1)
    sb = np.asarray(side_bits, np.int64).reshape(h, w)
    off = np.asarray(offsets, np.int64).reshape(h, w)
    jj, ii = np.mgrid[0:h, 0:w]
    slot, nxt, flags = (np.full(E, fill, np.int32) for _ in range(3))
    trips = written = 0
    for d in range(4):
        left = (d + 3) % 4
        bj, bi = STEP[d]
        aj, ai = bj + STEP[left][0], bi + STEP[left][1]
        B, A = _shifted(P, h, w, bj, bi) == n, _shifted(P, h, w, aj, ai) == n
        turn_left = A & (B | (connectivity == 8))
        straight = ~turn_left & B
        tj = np.where(turn_left, jj + aj, np.where(straight, jj + bj, jj))
        ti = np.where(turn_left, ii + ai, np.where(straight, ii + bi, ii))
        ts = np.where(turn_left, left, np.where(straight, d, (d + 1) % 4))
        has = (n > 0) & (((sb >> d) & 1) == 1)
        p = off + POPCOUNT[sb & ((1 << d) - 1)]
        sel = np.nonzero(has)
        tjs, tis, tss, ps = tj[sel], ti[sel], ts[sel], p[sel]
        tp = off[tjs, tis] + POPCOUNT[sb[tjs, tis] & ((1 << tss) - 1)]
        ok = (ps >= 0) & (ps < E) & (tp >= 0) & (tp < E)
        trips += int((~ok).sum())
        written += int(ok.sum())
        cells = (sel[0] * w + sel[1])[ok]
        slot[ps[ok]] = 4 * cells + d
        nxt[ps[ok]] = tp[ok]
        flags[ps[ok]] = np.where(_corner(P, n, h, w, d)[sel][ok], CORNER, 0) | d << 1
    return slot, nxt, flags, [trips, written]


def rounds(E):
    R = 1
    while (1 << R) < E:
        R += 1
    return R


def rank(nxt, flags):
    """snerf_outline_rank pass by pass -> (ring, rank, ordinal (E) int32, totals (E, 2) int32, stats [guard trips, sum of ring edges])"""
    raw = np.asarray(nxt, np.int64)
    E = len(raw)
    if E == 0:
        z = np.zeros(0, np.int32)
        return z, z.copy(), z.copy(), np.zeros((0, 2), np.int32), [0, 0]
    at = np.arange(E)
    bad = (raw < 0) | (raw >= E)
    t0 = np.where(bad, at, raw)
    corner = (np.asarray(flags, np.int64) & CORNER).astype(np.uint32)
    R = rounds(E)
    m, t = at.copy(), t0.copy()
    for _ in range(R):
        m, t = np.minimum(m, m[t]), t[t]
    ring = m
    cut = ring[t0] == t0
    q = np.where(cut, NIL, t0)
    u = np.where(cut, 0, 1).astype(np.uint32)
    v = np.where(cut, 0, corner[t0]).astype(np.uint32)
    for _ in range(R):
        live = q != NIL
        qq = np.where(live, q, 0)
        u, v, q = np.where(live, u + u[qq], u), np.where(live, v + v[qq], v), np.where(live, q[qq], NIL)
    one = np.uint32(1)
    L, C = u[ring] + one, v[ring] + corner[ring]
    rk = (L - one - u).view(np.int32)
    ordinal = (C - v - corner).view(np.int32)
    start = ring == at
    totals = np.stack([np.where(start, L.view(np.int32), 0), np.where(start, C.view(np.int32), 0)], 1).astype(np.int32)
    trips = int(bad.sum()) + int((ring[t0] != ring).sum())
    trips += int(((t0 != ring) & (rk[t0].view(np.uint32) != rk.view(np.uint32) + one)).sum())
    return ring.astype(np.int32), rk, ordinal, totals, [trips, int(totals[:, 0].view(np.uint32).astype(np.int64).sum())]


def ring_rows(ring, totals):
    """what the host derives between rank and emit -> (ring_row (E) int32: the ring's row at its start, -1 elsewhere; vertex_offset
    (n_rings) int64; n_rings; V)"""
    ring = np.asarray(ring, np.int64)
    starts = np.flatnonzero(ring == np.arange(len(ring)))
    ring_row = np.full(len(ring), -1, np.int32)
    ring_row[starts] = np.arange(len(starts), dtype=np.int32)
    counts = np.asarray(totals, np.int64).reshape(-1, 2)[starts, 1]
    total = np.cumsum(counts)
    return ring_row, (total - counts).astype(np.int64), len(starts), int(total[-1]) if len(total) else 0


def emit(ids, slot, flags, ring, ordinal, ring_row, vertex_offset, n_rings, V, fill=0):
    """-> (vertices (V, 2) int32 -- `fill` where nothing is written --, rows (n_rings, 8) uint64, stats [guard trips, vertices written])"""
    raw = np.asarray(ids, np.int64)
    h, w = raw.shape
    slot, ring, ordinal = (np.asarray(a, np.int64) for a in (slot, ring, ordinal))
    E = len(slot)
    vertices = np.full((V, 2), fill, np.int32)
    rows = np.array([ROW_INIT] * n_rings, np.uint64).reshape(n_rings, ROW_WORDS)
    ok = (slot >= 0) & (slot < 4 * h * w) & (ring >= 0) & (ring < E)
    r = np.where(ok, np.asarray(ring_row, np.int64)[np.where(ok, ring, 0)], -1)
    ok2 = ok & (r >= 0) & (r < n_rings)
    trips = int((~ok2).sum())
    at = np.flatnonzero(ok2)
    sl, r = slot[at], r[at]
    c, s = sl >> 2, sl & 3
    j, i = c // w, c % w
    x0, y0 = i + np.array(TAIL)[s, 0], j + np.array(TAIL)[s, 1]
    x1, y1 = x0 + np.array(STEP)[s, 1], y0 + np.array(STEP)[s, 0]
    corner = (np.asarray(flags, np.int64)[at] & CORNER) == 1
    first = np.asarray(vertex_offset, np.int64)[r]
    first_ok = (first >= 0) & (first <= V)                  # tested before anything is added to it
    pos = np.where(first_ok, np.where(first_ok, first, 0) + ordinal[at], -1)
    place = corner & (pos >= 0) & (pos < V)
    trips += int((corner & ~place).sum())
    vertices[pos[place], 0], vertices[pos[place], 1] = x0[place], y0[place]
    signed = np.zeros((n_rings, 3), np.int64)
    np.add.at(signed[:, 0], r, 1)
    np.add.at(signed[:, 1], r, corner.astype(np.int64))
    np.add.at(signed[:, 2], r, x0 * y1 - x1 * y0)
    rows[:, 0], rows[:, 1], rows[:, 3] = signed[:, 0].view(np.uint64), signed[:, 1].view(np.uint64), signed[:, 2].view(np.uint64)
    np.maximum.at(rows[:, 2], r, np.maximum(raw.reshape(-1)[c], 0).astype(np.uint64))
    for word, val in ((4, x0), (6, y0)):
        np.minimum.at(rows[:, word], r, val.astype(np.uint64))
        np.maximum.at(rows[:, word + 1], r, val.astype(np.uint64))
    return vertices, rows, [trips, int(place.sum())]


def trace(ids, K, connectivity=4):
    """every output of the five entries and of the host plumbing between them, as a dict of arrays and Python ints"""
    ids = np.asarray(ids, np.int32)
    sb, sides_stats = sides(ids, K)
    offsets, E = offsets_of(sb)
    slot, nxt, flags, link_stats = link(ids, sb, offsets, K, connectivity, E)
    ring, rk, ordinal, totals, rank_stats = rank(nxt, flags)
    ring_row, vertex_offset, n_rings, V = ring_rows(ring, totals)
    vertices, rows, emit_stats = emit(ids, slot, flags, ring, ordinal, ring_row, vertex_offset, n_rings, V)
    return {"sides": sb, "sides_stats": sides_stats, "offsets": offsets, "E": E, "slot": slot, "next": nxt, "flags": flags,
            "link_stats": link_stats, "ring": ring, "rank": rk, "ordinal": ordinal, "totals": totals, "rank_stats": rank_stats,
            "ring_row": ring_row, "vertex_offset": vertex_offset, "n_rings": n_rings, "V": V, "vertices": vertices, "rows": rows,
            "emit_stats": emit_stats}


def rings_of(t):
    """a trace as eval/utils/outline.py rings() returns it"""
    rows = t["rows"].reshape(-1, ROW_WORDS)
    return {"vertices": t["vertices"], "ring_start": np.concatenate([t["vertex_offset"], [t["V"]]]).astype(np.int64),
            "ring_object": rows[:, 2].astype(np.int64), "ring_area2": rows[:, 3].view(np.int64).copy(), "ring_edges": rows[:, 0].astype(np.int64),
            "ring_bbox": rows[:, 4:8].astype(np.int64), "n_rings": t["n_rings"]}


# ---- the same by a sequential walk --------------------------------------------------------------------------------------------------------
def walk(ids, K, connectivity=4):
    """the keys of `trace` (without the guard words, which a walk does not have) from plain loops over Python ints"""
    raw = np.asarray(ids, np.int64)
    h, w = raw.shape

    def at(j, i):
        if not (0 <= j < h and 0 <= i < w):
            return 0
        v = int(raw[j, i])
        return 0 if v < 0 or v > K else v

    side_bits, slots = [0] * (h * w), []
    for j in range(h):
        for i in range(w):
            n = at(j, i)
            if n == 0:
                continue
            for s in range(4):
                oj, oi = STEP[(s + 3) % 4]
                if at(j + oj, i + oi) != n:
                    side_bits[j * w + i] |= 1 << s
                    slots.append(4 * (j * w + i) + s)
    E = len(slots)
    index = {sl: p for p, sl in enumerate(slots)}
    nxt = []
    for sl in slots:
        c, d = divmod(sl, 4)
        j, i = divmod(c, w)
        n = at(j, i)
        left = (d + 3) % 4
        b = (j + STEP[d][0], i + STEP[d][1])
        a = (b[0] + STEP[left][0], b[1] + STEP[left][1])
        B, A = at(*b) == n, at(*a) == n
        if B and A:
            t = 4 * (a[0] * w + a[1]) + left
        elif B:
            t = 4 * (b[0] * w + b[1]) + d
        elif A and connectivity == 8:
            t = 4 * (a[0] * w + a[1]) + left
        else:
            t = 4 * c + (d + 1) % 4
        nxt.append(index[t])
    pred = [None] * E
    for p, t in enumerate(nxt):
        assert pred[t] is None, "the successor map is no permutation"
        pred[t] = p
    corner = [int(slots[pred[p]] % 4 != slots[p] % 4) for p in range(E)]
    ring, rk, ordinal, totals = [None] * E, [0] * E, [0] * E, [[0, 0] for _ in range(E)]
    ring_row, vertex_offset, vertices, rows = [-1] * E, [], [], []
    for start in range(E):
        if ring[start] is not None:
            continue
        row = list(ROW_INIT)
        row[2] = at(*divmod(slots[start] // 4, w))
        vertex_offset.append(len(vertices))
        ring_row[start] = len(rows)
        p, steps, corners, area2 = start, 0, 0, 0
        while True:
            ring[p], rk[p], ordinal[p] = start, steps, corners
            c, s = divmod(slots[p], 4)
            j, i = divmod(c, w)
            x0, y0 = i + TAIL[s][0], j + TAIL[s][1]
            x1, y1 = x0 + STEP[s][1], y0 + STEP[s][0]
            area2 += x0 * y1 - x1 * y0
            row[4], row[5], row[6], row[7] = min(row[4], x0), max(row[5], x0), min(row[6], y0), max(row[7], y0)
            if corner[p]:
                vertices.append((x0, y0))
                corners += 1
            steps += 1
            p = nxt[p]
            if p == start:
                break
        totals[start] = [steps, corners]
        row[0], row[1], row[3] = steps, corners, area2 % 2 ** 64
        rows.append(row)
    counts = [bin(b).count("1") for b in side_bits]
    offsets = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int32)
    raw_bad = int(((raw < 0) | (raw > K)).sum())
    return {"sides": np.array(side_bits, np.uint8), "sides_stats": [raw_bad, int((normalised(raw, K) > 0).sum()), E, sum(corner)],
            "offsets": offsets, "E": E, "slot": np.array(slots, np.int32).reshape(-1), "next": np.array(nxt, np.int32).reshape(-1),
            "flags": np.array([corner[p] | (slots[p] % 4) << 1 for p in range(E)], np.int32).reshape(-1),
            "ring": np.array(ring, np.int32).reshape(-1), "rank": np.array(rk, np.int32).reshape(-1),
            "ordinal": np.array(ordinal, np.int32).reshape(-1), "totals": np.array(totals, np.int32).reshape(E, 2),
            "ring_row": np.array(ring_row, np.int32).reshape(-1), "vertex_offset": np.array(vertex_offset, np.int64).reshape(-1),
            "n_rings": len(rows), "V": len(vertices), "vertices": np.array(vertices, np.int32).reshape(-1, 2),
            "rows": np.array(rows, np.uint64).reshape(-1, ROW_WORDS)}


# ---- the rasters the CPU and the GPU tests share ----------------------------------------------------------------------------------------
CLASSES = (3, 4)


def bullseye():
    """a ring of class 3 round a hole that holds a single cell of class 3: an object inside the hole of another"""
    out = np.zeros((9, 10), np.uint8)
    out[1:8, 1:8] = 3
    out[2:7, 2:7] = 0
    out[4, 4] = 3
    return out


def saddle():
    """two cells that touch at a corner: two objects at connectivity 4, one at 8"""
    out = np.zeros((2, 2), np.uint8)
    out[0, 0] = out[1, 1] = 3
    return out


def labels():
    """name -> label raster: the random shapes and the structured rasters of tests/objects_numpy.py, and the hand-made ones; the rows of
    31 and 32 cells have E = 64 and 66 edges -- the round count at and just past a power of two"""
    out = {f"random_{h}x{w}": ON.random_label(h, w) for h, w in ON.RANDOM_SHAPES}
    out.update(ON.structured())
    out.update(bullseye=bullseye(), saddle=saddle(), row_31=np.full((1, 31), 3, np.uint8), row_32=np.full((1, 32), 3, np.uint8))
    return out


_IDS = {}


def ids_of(name, connectivity):
    """(ids (h, w) int32, K) of the components of CLASSES in labels()[name], by tests/objects_numpy.py; computed once"""
    if (name, connectivity) not in _IDS:
        label = labels()[name]
        parent, _ = ON.link(label, CLASSES, connectivity)
        _IDS[name, connectivity] = ON.ids_of(parent, *label.shape)
    return _IDS[name, connectivity]


_TRACES = {}


def trace_of(name, connectivity):
    """trace(*ids_of(name, connectivity), connectivity), computed once and shared: treat it as read-only"""
    if (name, connectivity) not in _TRACES:
        ids, K = ids_of(name, connectivity)
        _TRACES[name, connectivity] = trace(ids, K, connectivity)
    return _TRACES[name, connectivity]
