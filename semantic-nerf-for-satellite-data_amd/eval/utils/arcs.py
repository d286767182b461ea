"""The arcs of a partition: the boundary of an id raster cut at its nodes into runs that two ids share, each traced once in either
direction and paired with its twin -- what lets neighbouring polygons keep one common border when they are simplified, and what a roof
line (ridge, hip, eave, step) is before it has a name.  The spec is include/snerf_rooflines.h, the stages are
the kernels of csrc/rooflines.hip on top of the outline entries (eval/utils/outline.py), torch is plumbing.

  first     snerf_arcs_first: the node bit of every edge's tail and the lowest rank among every ring's break edges;
  mark      snerf_arcs_mark: left, twin and ring-ordered position of every edge, the head and vertex flags of every position;
  between   the cumulative sums between mark and fold, in plain torch: the arc and the vertex ordinal of every position;
  fold      snerf_arcs_fold: the arcs' vertices and 12 integer words per arc;
  arcs      all of it in one call, checked: a dict of numpy arrays.

Everything a kernel writes is integer: the words are bit-reproducible and do not depend on launch order."""
import numpy as np
import torch

from ... import _lib
from . import outline as OL

ROW_WORDS = _lib.ARCS_ROW_WORDS
NO_FIRST = _lib.ARCS_NO_FIRST
_BIAS = 2 ** 31


def _buf(out, n, name, device):
    return torch.empty(n, dtype=torch.int32, device=device) if out is None else OL._words(out, n, name)


def first(ids, K, slot, ring, rank, out=None):
    """snerf_arcs_first -> (node (E) int32, first (E) int32: at a ring's start the lowest rank among its break edges, NO_FIRST where
    there is none and at every other edge; stats (2) int64: guard trips, break edges).  `out`: the node buffer.  E == 0 launches nothing."""
    ids = OL._ids(ids)
    h, w = ids.shape
    E = int(slot.numel())
    node = _buf(out, E, "node", ids.device)
    first_word = torch.full((E,), NO_FIRST, dtype=torch.int32, device=ids.device)
    stats = torch.zeros(2, dtype=torch.int64, device=ids.device)
    if E:
        _lib.call("snerf_arcs_first", ids, OL._words(slot, E, "slot"), OL._words(ring, E, "ring"), OL._words(rank, E, "rank"), h, w, OL._K(K), E,
                  node, first_word, stats, exc=ValueError)
    return node, first_word, stats


def ring_base_of(ring, totals):
    """between rank and mark, in plain torch -> (ring_row (E) int32: the ring's row at its start, -1 elsewhere; ring_base (n_rings) int64:
    the exclusive cumulative sum of the rings' edge counts; n_rings)"""
    E = ring.numel()
    starts = torch.nonzero(ring == torch.arange(E, dtype=torch.int32, device=ring.device)).reshape(-1)
    n_rings = int(starts.numel())
    ring_row = torch.full((E,), -1, dtype=torch.int32, device=ring.device)
    ring_row[starts] = torch.arange(n_rings, dtype=torch.int32, device=ring.device)
    counts = totals.reshape(-1, 2)[starts, 0].long()
    return ring_row, (torch.cumsum(counts, 0) - counts).contiguous(), n_rings


def mark(ids, K, side_bits, offsets, slot, flags, ring, rank, totals, node, first_word, ring_row, ring_base, out=None):
    """snerf_arcs_mark -> (left, twin, pos_of (E) int32 by edge; order, hf, vf (E) int32 by position; stats (4) int64: guard trips, edges
    written, break edges, edges with a twin).  `out`: the six buffers to write into.  E == 0 launches nothing."""
    ids = OL._ids(ids)
    h, w = ids.shape
    E, n_rings = int(slot.numel()), int(ring_base.numel())
    names = ("left", "twin", "pos_of", "order", "hf", "vf")
    bufs = tuple(_buf(None if out is None else out[k], E, name, ids.device) for k, name in enumerate(names))
    stats = torch.zeros(4, dtype=torch.int64, device=ids.device)
    if E:
        _lib.call("snerf_arcs_mark", ids, OL._words(side_bits, h * w, "sides", torch.uint8), OL._words(offsets, h * w, "offsets"),
                  OL._words(slot, E, "slot"), OL._words(flags, E, "flags"), OL._words(ring, E, "ring"), OL._words(rank, E, "rank"),
                  OL._words(totals, 2 * E, "totals"), OL._words(node, E, "node"), OL._words(first_word, E, "first"),
                  OL._words(ring_row, E, "ring_row"), OL._words(ring_base, n_rings, "ring_base", torch.int64), h, w, OL._K(K), E, n_rings,
                  *bufs, stats, exc=ValueError)
    return bufs + (stats,)


def between(order, hf, vf, node):
    """between mark and fold, in plain torch -> (arc_of, ordinal, last (E) int32 by position; vertex_offset (A) int64; A; V).  arc_of: the
    inclusive cumulative sum of hf, minus 1; ordinal: the vf positions of the same arc in front of the position; last: 1 at the last
    position of an open arc.  Reading A and V is a host synchronisation."""
    E = int(order.numel())
    dev = order.device
    if E == 0:
        z = torch.zeros(0, dtype=torch.int32, device=dev)
        return z, z.clone(), z.clone(), torch.zeros(0, dtype=torch.int64, device=dev), 0, 0
    arc_of = torch.cumsum(hf, 0, dtype=torch.int64) - 1
    heads = torch.nonzero(hf).reshape(-1)
    before = torch.cumsum(vf, 0, dtype=torch.int64) - vf
    ordinal = before - before[heads][arc_of]
    is_open = node[order[heads].long()] != 0
    ends = torch.cat([heads[1:], torch.tensor([E], dtype=heads.dtype, device=dev)]) - 1
    last = torch.zeros(E, dtype=torch.int32, device=dev)
    last[ends[is_open]] = 1
    inclusive = before + vf
    counts = inclusive[ends] - before[heads] + is_open.long()
    total = torch.cumsum(counts, 0)
    return arc_of.to(torch.int32), ordinal.to(torch.int32), last, (total - counts).contiguous(), int(heads.numel()), int(total[-1].item())


def fold(ids, key, slot, ring, left, twin, pos_of, node, ring_row, order, hf, vf, arc_of, ordinal, last, vertex_offset, A, V, n_rings,
         vertices=None):
    """snerf_arcs_fold -> (vertices (V, 2) int32, rows (A, 12) int64 holding the u64 words, stats (2) int64: guard trips, vertices
    written).  `key`: the key plane or None.  E == 0 launches nothing."""
    ids = OL._ids(ids)
    h, w = ids.shape
    E, A, V, n_rings = int(order.numel()), int(A), int(V), int(n_rings)
    if key is not None and not (torch.is_tensor(key) and key.is_cuda and key.dtype == torch.int32 and tuple(key.shape) == (h, w)):
        raise ValueError(f"arcs: key must be an int32 GPU raster of shape {(h, w)}")
    vertices = torch.empty((V, 2), dtype=torch.int32, device=ids.device) if vertices is None else OL._words(vertices, 2 * V, "vertices")
    rows = torch.zeros((A, ROW_WORDS), dtype=torch.int64, device=ids.device)
    stats = torch.zeros(2, dtype=torch.int64, device=ids.device)
    if E:
        by_edge = [OL._words(t, E, name) for t, name in ((slot, "slot"), (ring, "ring"), (left, "left"), (twin, "twin"), (pos_of, "pos_of"),
                                                         (node, "node"), (ring_row, "ring_row"), (order, "order"), (hf, "hf"), (vf, "vf"),
                                                         (arc_of, "arc_of"), (ordinal, "ordinal"), (last, "last"))]
        _lib.call("snerf_arcs_fold", ids, None if key is None else key.contiguous(), *by_edge,
                  OL._words(vertex_offset, A, "vertex_offset", torch.int64), h, w, E, A, n_rings, V, vertices, rows, stats,
                  exc=ValueError)
    return vertices, rows, stats


def arcs(ids, K, connectivity=4, key=None):
    """The arcs of the ids 1..K of `ids` ((H, W) int32 on the GPU), the rings traced at `connectivity`; `key`: the key plane of
    terrain.keys on the same lattice, for the key sums -> a dict of numpy arrays, per arc a (arcs are numbered in ring order):
      arc_start (A + 1) int64    arc a owns vertices[arc_start[a]:arc_start[a + 1]]
      vertices (V, 2) int32      lattice (x, y) = (column, row); an open arc from node to node, a closed one its ring's corners
      right, left (A) int64      the ids on the arc's right (its own ring's) and left (0: background or the raster's edge)
      edges (A) int64            the arc's length in unit edges
      twin (A) int64             the same arc in the left id's ring, which runs the other way; -1 for none
      closed (A) bool            the arc is a whole ring without a node
      owner (A) bool             left == 0 or right < left: of an arc and its twin exactly one is the owner
      key_edges, key_sum_right, key_sum_left (A) int64   the edges with valid keys on both sides, and the sums of those keys
      arc_ring (A) int64, ring_arcs: per ring the ids of its arcs in ring order (a list of int64 arrays)
      ring_first, ring_edges (R) int64   the rank at which the ring's first arc begins, the ring's edge count
      rings                      what outline.rings returns for the same raster
      stats                      {"edges", "arcs", "vertices", "rings", "breaks", "twin_edges"} as Python ints
    Any non-zero guard word raises a RuntimeError, as does a pairing that is no involution of arcs with equal lengths and swapped ids."""
    ids = OL._ids(ids)
    K = OL._K(K)
    side_bits, sstats = OL.sides(ids, K)
    offsets, E = OL.offsets_of(side_bits)
    s = [int(v) for v in sstats.cpu()]
    slot, nxt, flags, lstats = OL.link(ids, side_bits, offsets, K, connectivity, E)
    ring, rank, ordinal_c, totals, rstats = OL.rank_rings(nxt, flags)
    l, r = ([int(v) for v in t.cpu()] for t in (lstats, rstats))
    if s[2] != E or l != [0, E] or r != [0, E]:
        raise RuntimeError(f"arcs: the successor map is no permutation of the {E} edges (counted {s[2]}; link {l}; rank {r})")
    ring_row_v, vertex_offset_r, n_rings, V_r = OL.ring_rows(ring, totals)
    ring_vertices, ring_words, estats = OL.emit(ids, slot, flags, ring, ordinal_c, ring_row_v, vertex_offset_r, n_rings, V_r)
    node, first_word, fstats = first(ids, K, slot, ring, rank)
    ring_row, ring_base, _ = ring_base_of(ring, totals)
    left, twin, pos_of, order, hf, vf, mstats = mark(ids, K, side_bits, offsets, slot, flags, ring, rank, totals, node, first_word, ring_row,
                                                     ring_base)
    arc_of, ordinal, last, vertex_offset, A, V = between(order, hf, vf, node)
    vertices, rows, ostats = fold(ids, key, slot, ring, left, twin, pos_of, node, ring_row, order, hf, vf, arc_of, ordinal, last, vertex_offset,
                                  A, V, n_rings)
    e, f, m, o = ([int(v) for v in t.cpu()] for t in (estats, fstats, mstats, ostats))
    if e != [0, V_r] or f[0] or m[:2] != [0, E] or m[2] != f[1] or o != [0, V]:
        raise RuntimeError(f"arcs: a guard tripped or a count is off (emit {e} of {V_r}; first {f}; mark {m} of {E}; fold {o} of {V})")
    w = rows.cpu().numpy()
    right, lft, edges, twin_arc = w[:, 2].copy(), w[:, 3].copy(), w[:, 0].copy(), w[:, 5] - 1
    if int(edges.sum()) != E or (w[:, 6] != edges * w[:, 5]).any():
        raise RuntimeError("arcs: the twins of an arc's edges do not all lie in one arc")
    has = twin_arc >= 0
    t = twin_arc[has]
    if (has != (lft > 0)).any() or (twin_arc[t] != np.flatnonzero(has)).any() or (edges[t] != edges[has]).any() \
            or (right[t] != lft[has]).any() or (lft[t] != right[has]).any():
        raise RuntimeError("arcs: the pairing is no involution of arcs with equal lengths and swapped ids")
    ring_words = ring_words.cpu().numpy()
    starts = torch.nonzero(ring_row >= 0).reshape(-1)
    ring_first = first_word[starts].cpu().numpy().astype(np.int64)
    arc_ring = w[:, 4] - 1
    bounds = np.searchsorted(arc_ring, np.arange(n_rings + 1))
    rings = {"vertices": ring_vertices.cpu().numpy(), "ring_start": np.concatenate([vertex_offset_r.cpu().numpy(), [V_r]]).astype(np.int64),
             "ring_object": ring_words[:, 2].copy(), "ring_area2": ring_words[:, 3].copy(), "ring_edges": ring_words[:, 0].copy(),
             "ring_bbox": ring_words[:, 4:8].copy(),
             "stats": {"bad_ids": s[0], "object_cells": s[1], "edges": E, "corners": V_r, "rings": n_rings}}
    return {"arc_start": np.concatenate([vertex_offset.cpu().numpy(), [V]]).astype(np.int64), "vertices": vertices.cpu().numpy(),
            "right": right, "left": lft, "edges": edges, "twin": twin_arc, "closed": w[:, 10] == 0, "owner": (lft == 0) | (right < lft),
            "key_edges": w[:, 7].copy(), "key_sum_right": w[:, 8] - _BIAS * w[:, 7], "key_sum_left": w[:, 9] - _BIAS * w[:, 7],
            "arc_ring": arc_ring, "ring_arcs": [np.arange(bounds[k], bounds[k + 1], dtype=np.int64) for k in range(n_rings)],
            "ring_first": np.where(ring_first == NO_FIRST, 0, ring_first), "ring_edges": ring_words[:, 0].copy(), "rings": rings,
            "stats": {"edges": E, "arcs": A, "vertices": V, "rings": n_rings, "breaks": m[2], "twin_edges": m[3]}}
