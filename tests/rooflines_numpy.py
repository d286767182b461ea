"""numpy restatement of include/snerf_rooflines.h (never of csrc/rooflines.hip): the oracle of tests/test_gpu_rooflines.py.  The facet
growth is stated as whole-array rounds.  The arcs are stated twice: `trace` states every entry and the host's cumulative sums over
whole arrays (positions, flags, row folds), `walk` follows `next` round each ring, cuts at the nodes and pairs the twins by looking the
reversed segment up in a dictionary.  tests/test_rooflines_cpu.py holds the two to each other bit for bit and both to facts that know
nothing of tracing."""
import numpy as np

from tests import outline_numpy as ON
from tests import roofs_numpy as RN

ROW_WORDS = 12
NO_FIRST = 2 ** 31 - 1
MAX_ROUNDS = 64
BIAS = 2 ** 31
STEP, TAIL, POPCOUNT, CORNER = ON.STEP, ON.TAIL, ON.POPCOUNT, ON.CORNER
NEIGHBOURS = [(-1, 0), (0, 1), (1, 0), (0, -1)]          # N, E, S, W in (row, column): the cell across side s
_STEP, _TAIL = np.array(STEP), np.array(TAIL)


def _valid(k):
    return (k != RN.HOLE) & (k != RN.NOT_A_KEY)


# ---- growth -----------------------------------------------------------------------------------------------------------------------------
def grow_round(f, ids, key, facet_root, planes, F, unit, max_rq):
    """one round of snerf_roofs_grow -> (the next raster int32, cells assigned, guard trips)"""
    f, ids, key = np.asarray(f, np.int64), np.asarray(ids, np.int64), np.asarray(key, np.int64)
    h, w = f.shape
    cells = h * w
    own_bad = (f < 0) | (f > F)
    trips = int(own_bad.sum())
    taker = ~own_bad & (f == 0) & (ids > 0) & _valid(key)
    best_n, best_rq = np.zeros((h, w), np.int64), np.zeros((h, w), np.int64)
    jj, ii = np.mgrid[0:h, 0:w]
    planes = np.asarray(planes, np.float64).reshape(-1, 3)
    root = np.asarray(facet_root, np.int64).reshape(-1)
    for dj, di in NEIGHBOURS:
        nj, ni = jj + dj, ii + di
        inside = (nj >= 0) & (nj < h) & (ni >= 0) & (ni < w)
        cj, ci = np.clip(nj, 0, h - 1), np.clip(ni, 0, w - 1)
        n = f[cj, ci]
        cand = taker & inside & (n >= 1) & (n <= F) & (ids[cj, ci] == ids)
        at = np.where(cand, n, 1) - 1
        if F == 0:
            continue
        g, a, b = planes[at, 0], planes[at, 1], planes[at, 2]
        cand &= np.isfinite(g) & np.isfinite(a) & np.isfinite(b)
        rt = root[at]
        rt_bad = cand & ((rt < 0) | (rt >= cells))
        trips += int(rt_bad.sum())
        cand &= ~rt_bad
        rt = np.where(cand, rt, 0)
        k0 = key.reshape(-1)[rt]
        cand &= _valid(k0)
        j0, i0 = rt // w, rt % w
        with np.errstate(all="ignore"):
            pred = (g + (a * (ii - i0).astype(np.float64))) + (b * (jj - j0).astype(np.float64))
            e = (key - k0).astype(np.float64) - pred
            t = np.rint(e / np.float64(unit))
        clamped = ~(t < 262144.0) | (t < -262144.0)
        mag = np.abs(np.where(clamped | ~cand, 0.0, t)).astype(np.int64)
        cand &= ~clamped & (mag <= max_rq)
        better = cand & ((best_n == 0) | (mag < best_rq) | ((mag == best_rq) & (n < best_n)))
        best_n, best_rq = np.where(better, n, best_n), np.where(better, mag, best_rq)
    return np.where(best_n > 0, best_n, f).astype(np.int32), int((best_n > 0).sum()), trips


def grow_rounds(fids, ids, key, facet_root, planes, F, unit, max_rq, rounds):
    """snerf_roofs_grow -> (the raster after `rounds` rounds, stats: [assigned in round r ..., guard trips])"""
    assert 1 <= rounds <= MAX_ROUNDS
    f = np.asarray(fids, np.int32)
    stats = [0] * (rounds + 1)
    if F == 0:
        return f.copy(), stats
    for r in range(rounds):
        f, stats[r], trips = grow_round(f, ids, key, facet_root, planes, F, unit, max_rq)
        stats[rounds] += trips
    return f, stats


def grow(fids, ids, key, facet_root, planes, F, unit=RN.UNIT, max_rq=256, max_rounds=None, batch=8):
    """roofs.grow: batches of `batch` rounds until a batch's last round assigns nothing, at most h + w rounds -> (raster, the rounds
    that assigned something, the cells assigned round by round)"""
    f = np.asarray(fids, np.int32)
    limit = sum(f.shape) if max_rounds is None else max_rounds
    counts = []
    while len(counts) < limit:
        n = min(batch, limit - len(counts))
        f, stats = grow_rounds(f, ids, key, facet_root, planes, F, unit, max_rq, n)
        assert stats[n] == 0
        counts += stats[:n]
        if stats[n - 1] == 0:
            break
    used = max([r + 1 for r, c in enumerate(counts) if c], default=0)
    return f, used, counts


# ---- arcs, entry by entry over whole arrays -----------------------------------------------------------------------------------------------
def _edge_cells(slot, w):
    c, s = np.asarray(slot, np.int64) >> 2, np.asarray(slot, np.int64) & 3
    return c, s, c // w, c % w


def nodes(ids, K):
    """the node bit of every lattice vertex -> (h + 1, w + 1) bool"""
    P = np.pad(ON.normalised(ids, K), 1)
    nw, ne, se, sw = P[:-1, :-1], P[:-1, 1:], P[1:, 1:], P[1:, :-1]
    return ((nw != ne).astype(int) + (ne != se) + (se != sw) + (sw != nw)) >= 3


def first(ids, K, slot, ring, rank):
    """snerf_arcs_first -> (node (E) int32, first (E) int32, stats [guard trips, break edges])"""
    h, w = np.asarray(ids).shape
    E = len(slot)
    c, s, j, i = _edge_cells(slot, w)
    node = nodes(ids, K)[j + _TAIL[s, 1], i + _TAIL[s, 0]].astype(np.int32) if E else np.zeros(0, np.int32)
    out = np.full(E, NO_FIRST, np.int32)
    at = np.flatnonzero(node)
    np.minimum.at(out, np.asarray(ring, np.int64)[at], np.asarray(rank, np.int32)[at])
    return node, out, [0, int(node.sum())]


def ring_base_of(ring, totals):
    """between rank and mark -> (ring_row (E) int32, ring_base (n_rings) int64, n_rings)"""
    ring = np.asarray(ring, np.int64)
    starts = np.flatnonzero(ring == np.arange(len(ring)))
    ring_row = np.full(len(ring), -1, np.int32)
    ring_row[starts] = np.arange(len(starts), dtype=np.int32)
    counts = np.asarray(totals, np.int64).reshape(-1, 2)[starts, 0]
    return ring_row, (np.cumsum(counts) - counts).astype(np.int64), len(starts)


def mark(ids, K, side_bits, offsets, slot, flags, ring, rank, totals, node, first_word, ring_row, ring_base):
    """snerf_arcs_mark on buffers that trip no guard but the twin's -> (left, twin, pos_of, order, hf, vf (E) int32, stats)"""
    h, w = np.asarray(ids).shape
    E = len(slot)
    n = ON.normalised(ids, K)
    P = np.pad(n, 1)
    c, s, j, i = _edge_cells(slot, w)
    ring = np.asarray(ring, np.int64)
    L = np.asarray(totals, np.int64).reshape(-1, 2)[ring, 0]
    f = np.asarray(first_word, np.int64)[ring]
    f = np.where(f == NO_FIRST, 0, f)
    base = np.asarray(ring_base, np.int64)[np.asarray(ring_row, np.int64)[ring]]
    pos = base + (np.asarray(rank, np.int64) - f) % np.maximum(L, 1)
    aj, ai = j + np.array(NEIGHBOURS)[s, 0], i + np.array(NEIGHBOURS)[s, 1]
    left = P[aj + 1, ai + 1]
    has = left > 0
    t = np.where(has, aj * w + ai, 0)
    ts = (s + 2) & 3
    sb = np.asarray(side_bits, np.int64)[t]
    tp = np.asarray(offsets, np.int64)[t] + POPCOUNT[sb & ((1 << ts) - 1)]
    good = has & (((sb >> ts) & 1) == 1) & (tp >= 0) & (tp < E)
    twin = np.where(good, tp, -1)
    brk = np.asarray(node, np.int64) != 0
    order, hf, vf = (np.zeros(E, np.int32) for _ in range(3))
    order[pos] = np.arange(E)
    hf[pos] = brk | (pos == base)
    vf[pos] = brk | ((np.asarray(flags, np.int64) & CORNER) == 1)
    return (left.astype(np.int32), twin.astype(np.int32), pos.astype(np.int32), order, hf, vf,
            [int((has & ~good).sum()), E, int(brk.sum()), int(good.sum())])


def between(order, hf, vf, node):
    """the host's cumulative sums between mark and fold -> (arc_of, ordinal, last (E) int32, vertex_offset (A) int64, A, V, open (A))"""
    E = len(order)
    hf, vf = np.asarray(hf, np.int64), np.asarray(vf, np.int64)
    arc_of = np.cumsum(hf) - 1
    A = int(arc_of[-1]) + 1 if E else 0
    heads = np.flatnonzero(hf)
    before = np.cumsum(vf) - vf                                   # the vf positions in front of each position
    ordinal = before - before[heads][arc_of] if E else before
    is_open = np.asarray(node, np.int64)[np.asarray(order, np.int64)[heads]] != 0
    ends = np.append(heads[1:], E) - 1 if E else heads
    last = np.zeros(E, np.int32)
    last[ends[is_open]] = 1
    counts = np.add.reduceat(vf, heads) + is_open if E else np.zeros(0, np.int64)
    total = np.cumsum(counts)
    return (arc_of.astype(np.int32), ordinal.astype(np.int32), last, (total - counts).astype(np.int64), A, int(total[-1]) if E else 0,
            is_open)


def fold(ids, key, slot, ring, left, twin, pos_of, node, ring_row, order, hf, vf, arc_of, ordinal, last, vertex_offset, A, V, n_rings,
         fill=0):
    """snerf_arcs_fold with its guards on arc_of, the twin's arc and the vertex positions -> (vertices (V, 2) int32 -- `fill` where
    nothing is written --, rows (A, 12) uint64, stats [guard trips, vertices written])"""
    raw = np.asarray(ids, np.int64)
    h, w = raw.shape
    E = len(order)
    vertices = np.full((V, 2), fill, np.int32)
    rows = np.zeros((A, ROW_WORDS), np.uint64)
    if E == 0:
        return vertices, rows, [0, 0]
    p = np.asarray(order, np.int64)
    a = np.asarray(arc_of, np.int64)
    ok = (a >= 0) & (a < A)
    trips = int((~ok).sum())
    c, s, j, i = _edge_cells(np.asarray(slot)[p], w)
    x0, y0 = i + _TAIL[s, 0], j + _TAIL[s, 1]
    x1, y1 = x0 + _STEP[s, 1], y0 + _STEP[s, 0]
    head, is_vf, is_last = np.asarray(hf)[:] != 0, (np.asarray(vf) != 0).astype(np.int64), np.asarray(last) != 0
    tw = np.asarray(twin, np.int64)[p]
    has = tw >= 0
    ta = a[np.asarray(pos_of, np.int64)[np.where(has, tw, 0)]]
    ta_ok = has & (ta >= 0) & (ta < A)
    trips += int((ok & has & ~ta_ok).sum())
    one = np.where(ta_ok, 1 + ta, 0)
    words = np.zeros((A, ROW_WORDS), np.int64)
    at = np.flatnonzero(ok)
    r = a[at]

    def add(word, v):
        np.add.at(words[:, word], r, np.asarray(v, np.int64)[at])

    def top(word, v):
        np.maximum.at(words[:, word], r, np.asarray(v, np.int64)[at])

    add(0, np.ones(E, np.int64))
    add(1, is_vf)
    top(2, np.maximum(raw.reshape(-1)[c], 0))
    top(3, np.maximum(np.asarray(left, np.int64)[p], 0))
    top(4, np.asarray(ring_row, np.int64)[np.asarray(ring, np.int64)[p]] + 1)
    top(5, np.where(head, one, 0))
    add(6, one)
    if key is not None:
        k = np.asarray(key, np.int64)
        aj, ai = j + np.array(NEIGHBOURS)[s, 0], i + np.array(NEIGHBOURS)[s, 1]
        inside = (aj >= 0) & (aj < h) & (ai >= 0) & (ai < w)
        kr, kl = k.reshape(-1)[c], k[np.clip(aj, 0, h - 1), np.clip(ai, 0, w - 1)]
        keyed = inside & _valid(kr) & _valid(kl)
        add(7, keyed)
        add(8, np.where(keyed, kr + BIAS, 0))
        add(9, np.where(keyed, kl + BIAS, 0))
    top(10, head & (np.asarray(node, np.int64)[p] != 0))
    rows[:] = words.view(np.uint64)
    v0 = np.asarray(vertex_offset, np.int64)[np.where(ok, a, 0)] if A else np.full(E, -1, np.int64)
    v_ok = (v0 >= 0) & (v0 <= V)
    placed = 0
    for want, plus, x, y in ((is_vf == 1, 0, x0, y0), (is_last, is_vf, x1, y1)):
        pos = np.where(v_ok, np.where(v_ok, v0, 0) + np.asarray(ordinal, np.int64) + plus, -1)
        place = ok & want & (pos >= 0) & (pos < V)
        trips += int((ok & want & ~place).sum())
        vertices[pos[place], 0], vertices[pos[place], 1] = x[place], y[place]
        placed += int(place.sum())
    return vertices, rows, [trips, placed]


def trace(ids, K, connectivity=4, key=None, outline=None):
    """every output of the three arc entries and of the host plumbing between them, on top of tests/outline_numpy.py trace"""
    ids = np.asarray(ids, np.int32)
    o = ON.trace(ids, K, connectivity) if outline is None else outline
    node, first_word, first_stats = first(ids, K, o["slot"], o["ring"], o["rank"])
    ring_row, ring_base, n_rings = ring_base_of(o["ring"], o["totals"])
    left, twin, pos_of, order, hf, vf, mark_stats = mark(ids, K, o["sides"], o["offsets"], o["slot"], o["flags"], o["ring"], o["rank"],
                                                         o["totals"], node, first_word, ring_row, ring_base)
    arc_of, ordinal, last, vertex_offset, A, V, is_open = between(order, hf, vf, node)
    vertices, rows, fold_stats = fold(ids, key, o["slot"], o["ring"], left, twin, pos_of, node, ring_row, order, hf, vf, arc_of, ordinal, last,
                                      vertex_offset, A, V, n_rings)
    return {"outline": o, "E": o["E"], "node": node, "first": first_word, "first_stats": first_stats, "ring_row": ring_row,
            "ring_base": ring_base, "n_rings": n_rings, "left": left, "twin": twin, "pos_of": pos_of, "order": order, "hf": hf, "vf": vf,
            "mark_stats": mark_stats, "arc_of": arc_of, "ordinal": ordinal, "last": last, "vertex_offset": vertex_offset, "A": A, "V": V,
            "vertices": vertices, "rows": rows, "fold_stats": fold_stats}


def arcs_of(t):
    """a trace as eval/utils/arcs.py arcs() returns it (without the rings and the stats)"""
    rows = t["rows"].astype(np.int64).reshape(-1, ROW_WORDS)
    A = len(rows)
    ring_of = rows[:, 4] - 1
    left, right = rows[:, 3], rows[:, 2]
    o = t["outline"]
    starts = np.flatnonzero(t["ring_row"] >= 0)
    starts_first = t["first"][starts].astype(np.int64)
    return {"arc_start": np.concatenate([t["vertex_offset"], [t["V"]]]).astype(np.int64), "vertices": t["vertices"], "right": right.copy(),
            "left": left.copy(), "edges": rows[:, 0].copy(), "twin": rows[:, 5] - 1, "closed": rows[:, 10] == 0,
            "owner": (left == 0) | (right < left), "key_edges": rows[:, 7].copy(), "key_sum_right": rows[:, 8] - BIAS * rows[:, 7],
            "key_sum_left": rows[:, 9] - BIAS * rows[:, 7], "arc_ring": ring_of,
            "ring_arcs": [np.flatnonzero(ring_of == r) for r in range(t["n_rings"])], "n_arcs": A,
            "ring_first": np.where(starts_first == NO_FIRST, 0, starts_first), "ring_edges": o["totals"][starts, 0].astype(np.int64),
            "rings": ON.rings_of(o)}


# ---- the same by a sequential walk ----------------------------------------------------------------------------------------------------------
def walk(ids, K, connectivity=4, key=None):
    """the per-edge, per-position and per-arc keys of `trace` from plain loops: every ring is followed along `next` from its lowest
    edge, turned to begin at its first node, cut at the nodes, and the twins are paired through a dictionary of directed segments"""
    raw = np.asarray(ids, np.int64)
    h, w = raw.shape
    o = ON.walk(raw, K, connectivity)
    E = o["E"]
    slot, nxt, ring, flags = (o[k].tolist() for k in ("slot", "next", "ring", "flags"))

    def at(j, i):
        if not (0 <= j < h and 0 <= i < w):
            return 0
        v = int(raw[j, i])
        return 0 if v < 0 or v > K else v

    def ends(p):
        c, s = divmod(slot[p], 4)
        j, i = divmod(c, w)
        x0, y0 = i + TAIL[s][0], j + TAIL[s][1]
        return (x0, y0), (x0 + STEP[s][1], y0 + STEP[s][0])

    def is_node(x, y):
        nw, ne, se, sw = at(y - 1, x - 1), at(y - 1, x), at(y, x), at(y, x - 1)
        return (nw != ne) + (ne != se) + (se != sw) + (sw != nw) >= 3

    segment = {ends(p): p for p in range(E)}
    assert len(segment) == E
    node = [int(is_node(*ends(p)[0])) for p in range(E)]
    left, twin = [0] * E, [-1] * E
    for p in range(E):
        c, s = divmod(slot[p], 4)
        j, i = divmod(c, w)
        left[p] = at(j + NEIGHBOURS[s][0], i + NEIGHBOURS[s][1])
        tail, head = ends(p)
        if left[p] > 0:
            twin[p] = segment[head, tail]
    pos_of, order, hf, vf, arc_of = [0] * E, [], [], [], []
    arcs, ring_row = [], {}
    for start in range(E):
        if ring[start] != start:
            continue
        ring_row[start] = len(ring_row)
        cycle, p = [], start
        while True:
            cycle.append(p)
            p = nxt[p]
            if p == start:
                break
        breaks = [k for k, p in enumerate(cycle) if node[p]]
        turn = breaks[0] if breaks else 0
        run = cycle[turn:] + cycle[:turn]
        for k, p in enumerate(run):
            pos_of[p] = len(order)
            head = bool(node[p]) or k == 0
            if head:
                arcs.append({"edges": [], "ring": ring_row[start], "open": bool(node[p])})
            order.append(p)
            hf.append(int(head))
            vf.append(int(bool(node[p]) or bool(flags[p] & CORNER)))
            arc_of.append(len(arcs) - 1)
            arcs[-1]["edges"].append(p)
    vertices, vertex_offset, rows = [], [], []
    k64 = None if key is None else np.asarray(key, np.int64)
    for arc in arcs:
        vertex_offset.append(len(vertices))
        row = [0] * ROW_WORDS
        for n, p in enumerate(arc["edges"]):
            c, s = divmod(slot[p], 4)
            j, i = divmod(c, w)
            if vf[pos_of[p]]:
                vertices.append(ends(p)[0])
                row[1] += 1
            row[0] += 1
            row[2] = max(row[2], max(int(raw[j, i]), 0))
            row[3] = max(row[3], left[p])
            row[4] = arc["ring"] + 1
            if twin[p] >= 0:
                one = 1 + arc_of[pos_of[twin[p]]]
                row[6] += one
                if n == 0:
                    row[5] = one
            if k64 is not None:
                aj, ai = j + NEIGHBOURS[s][0], i + NEIGHBOURS[s][1]
                if 0 <= aj < h and 0 <= ai < w and RN.valid(int(k64[j, i])) and RN.valid(int(k64[aj, ai])):
                    row[7] += 1
                    row[8] += int(k64[j, i]) + BIAS
                    row[9] += int(k64[aj, ai]) + BIAS
        if arc["open"]:
            vertices.append(ends(arc["edges"][-1])[1])
            row[10] = 1
        rows.append(row)
    return {"node": np.array(node, np.int32).reshape(-1), "left": np.array(left, np.int32).reshape(-1),
            "twin": np.array(twin, np.int32).reshape(-1), "pos_of": np.array(pos_of, np.int32).reshape(-1),
            "order": np.array(order, np.int32).reshape(-1), "hf": np.array(hf, np.int32).reshape(-1), "vf": np.array(vf, np.int32).reshape(-1),
            "arc_of": np.array(arc_of, np.int32).reshape(-1), "vertex_offset": np.array(vertex_offset, np.int64).reshape(-1), "A": len(arcs),
            "V": len(vertices), "vertices": np.array(vertices, np.int32).reshape(-1, 2),
            "rows": np.array(rows, np.uint64).reshape(-1, ROW_WORDS), "n_rings": len(ring_row)}


# ---- the rasters the CPU and the GPU tests share --------------------------------------------------------------------------------------------
def two_rows():
    """2 x 130: id 1 on the top row, id 2 on the bottom row -- their shared arc of 130 edges crosses two wave boundaries"""
    ids = np.ones((2, 130), np.int32)
    ids[1] = 2
    return ids, 2


def rasters():
    """name -> (ids (h, w) int32, K, connectivity)"""
    out = {}
    for name in ON.labels():
        for conn in (4, 8):
            ids, K = ON.ids_of(name, conn)
            out[f"{name}-{conn}"] = (ids, K, conn)
    out["checkerboard_5x7"] = RN.id_raster(5, 7, "checkerboard") + (4,)
    out["two_rectangles_37x53"] = RN.id_raster(37, 53, "two_rectangles") + (4,)
    out["blobs_37x53"] = RN.id_raster(37, 53, "blobs") + (4,)
    out["two_rows_2x130"] = two_rows() + (4,)
    out["one_cell"] = (np.ones((1, 1), np.int32), 1, 4)
    out["all_zero"] = (np.zeros((3, 5), np.int32), 0, 4)
    return out


_TRACES = {}


def trace_of(name):
    """trace of rasters()[name] with the key plane key_of(name), computed once and shared: treat it as read-only"""
    if name not in _TRACES:
        ids, K, conn = rasters()[name]
        _TRACES[name] = trace(ids, K, conn, key=key_of(name))
    return _TRACES[name]


def key_of(name):
    ids, _, _ = rasters()[name]
    h, w = ids.shape
    return RN.key_raster(h, w, "random", seed=3)


_TOWN = {}


def town():
    """the 48 x 64 town of tests/roofs_numpy.py with its kept facets (min_facet_m2 = 4) -> a dict: key, ids, K, fids (the kept facets),
    F, planes (F, 3), root (F), grown, rounds, counts, and `table`: the kept facets' host table.  Computed once."""
    if not _TOWN:
        import torch
        from snerf_amd.eval.utils import dsm as D
        from snerf_amd.eval.utils import roofs as RF
        key, ids, K, alt = RN.town()
        r = RN.roofs(key, ids, K, RN.TOWN_RES)
        grid = D.DsmGrid(500000.0, 4100000.0, RN.TOWN_RES, RN.TOWN_SHAPE[1], RN.TOWN_SHAPE[0])
        root_key = np.array([key.reshape(-1)[row[14]] for row in r["moments"]])
        table = RF.facet_table(RN.words(r["moments"]).view(np.int64), grid, root_key=root_key,
                               residual_rows=RN.words(r["residual_rows"]).view(np.int64))
        fids, kept = RF.filter_facets(torch.from_numpy(r["fids"]), table, min_facet_m2=4.0)
        fids = fids.numpy().astype(np.int32)
        F = len(kept["object"])
        grown, rounds, counts = grow(fids, ids, key, kept["root"], kept["plane"], F)
        _TOWN.update(key=key, ids=ids, K=K, alt=alt, fids=fids, F=F, planes=kept["plane"], root=kept["root"], table=kept, grid=grid,
                     grown=grown, rounds=rounds, counts=counts)
    return _TOWN
