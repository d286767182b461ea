"""Footprints as vectors: the boundary rings of the objects of an id raster, traced on the device, and the polygons a GIS reads --
what turns the id rasters of objects() and the facet ids of roofs() into GeoJSON without rasterio.features.shapes or GDAL (parity with
either is UNPINNED: neither is part of this build).  The reference has no counterpart; the spec is include/snerf_outline.h (DESIGN.md
section 5ze), the stages are the kernels of csrc/outline.hip, torch is plumbing.  The raster functions take and return device tensors.

  sides        snerf_outline_sides: which sides of every object cell are boundary edges, and their count E;
  link         snerf_outline_link: the edges in compact order, each with its successor from the 2 x 2 cells at its head;
  rank_rings   snerf_outline_rank: the rings are the cycles of the successor map; ring, rank and corner ordinal of every edge by pointer
               jumping (2 ceil(log2 E) + 4 launches, no atomics outside the two counting passes, no barrier);
  emit         snerf_outline_emit: the corners as ordered lattice vertices, and per ring the edges, the object, the doubled signed area
               and the bounding box;
  rings        the four in one call;
  polygons     per object its outer ring (positive area) followed by its holes;
  simplify     Douglas-Peucker per ring, exact in integers, on the host;
  simplify_shared  the same per ARC (eval/utils/arcs.py): a border two objects share is simplified once, so neighbours stay gap-free;
  to_map       lattice vertices -> (east, north);
  geojson      a FeatureCollection, one Polygon per object.

Everything a kernel writes is integer: the words are bit-reproducible and do not depend on launch order."""
from fractions import Fraction

import numpy as np
import torch

from ... import _lib
from . import ortho as OR

ROW_WORDS = _lib.OUTLINE_ROW_WORDS
MAX_CELLS = _lib.OUTLINE_MAX_CELLS
CORNER = _lib.OUTLINE_CORNER
_ROW_INIT = (0, 0, 0, 0, -1, 0, -1, 0)                  # int64 words: -1 holds 2^64 - 1
_POPCOUNT = tuple(bin(k).count("1") for k in range(16))


def _ids(ids):
    if not (torch.is_tensor(ids) and ids.is_cuda):
        raise ValueError("outline: ids must be a GPU tensor (the HIP path has no CPU fallback)")
    if ids.dtype != torch.int32 or ids.dim() != 2:
        raise ValueError(f"outline: ids must be a 2-D int32 raster, got {ids.dtype} {tuple(ids.shape)}")
    h, w = ids.shape
    if h * w < 1 or h * w >= MAX_CELLS:
        raise ValueError(f"outline: a raster of {h} x {w} cells: between 1 and 2^29 - 1 cells are taken")
    return ids.contiguous()


def _words(t, n, name, dtype=torch.int32):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == dtype and t.numel() == n and t.is_contiguous()):
        raise ValueError(f"outline: {name} must hold {n} contiguous {dtype} words on the GPU")
    return t


def _K(K):
    K = int(K)
    if not 0 <= K < 2 ** 31:
        raise ValueError(f"outline: K = {K} outside [0, 2^31)")
    return K


def sides(ids, K, out=None):
    """snerf_outline_sides -> (sides (H * W) uint8: the 4-bit mask of a cell's boundary sides N, E, S, W; stats (4) int64: cells with an
    id outside [0, K], object cells, boundary edges, corner edges)"""
    ids = _ids(ids)
    h, w = ids.shape
    out = torch.empty(h * w, dtype=torch.uint8, device=ids.device) if out is None else _words(out, h * w, "sides", torch.uint8)
    stats = torch.zeros(4, dtype=torch.int64, device=ids.device)
    _lib.call("snerf_outline_sides", ids, h, w, _K(K), out, stats, exc=ValueError)
    return out, stats


def offsets_of(side_bits):
    """the compact index of every cell's first edge: the exclusive cumulative sum of popcount(sides) -> (offsets (H * W) int32, E).
    Plain torch; reading E is the host synchronisation."""
    counts = torch.tensor(_POPCOUNT, dtype=torch.int32, device=side_bits.device)[side_bits.long()]
    total = torch.cumsum(counts, 0, dtype=torch.int64)
    E = int(total[-1].item()) if total.numel() else 0
    return (total - counts).to(torch.int32), E


def link(ids, side_bits, offsets, K, connectivity, E, out=None):
    """snerf_outline_link -> (slot, next, flags (E) int32, stats (2) int64: guard trips, edges written).  `out`: the three buffers to
    write into.  E == 0 launches nothing."""
    ids = _ids(ids)
    h, w = ids.shape
    if connectivity not in (4, 8):
        raise ValueError(f"outline: connectivity must be 4 or 8, got {connectivity!r}")
    E = int(E)
    if E < 0:
        raise ValueError(f"outline: E = {E} is negative")
    if out is None:
        out = tuple(torch.empty(E, dtype=torch.int32, device=ids.device) for _ in range(3))
    slot, nxt, flags = (_words(t, E, name) for t, name in zip(out, ("slot", "next", "flags")))
    stats = torch.zeros(2, dtype=torch.int64, device=ids.device)
    _lib.call("snerf_outline_link", ids, _words(side_bits, h * w, "sides", torch.uint8), _words(offsets, h * w, "offsets"), h, w, _K(K),
              connectivity, E, slot, nxt, flags, stats, exc=ValueError)
    return slot, nxt, flags, stats


def workspace_bytes(E):
    n = _lib.lib().snerf_outline_workspace_bytes(int(E))
    if n < 0:
        _lib.check(1, "snerf_outline_workspace_bytes", ValueError)
    return n


def rank_rings(nxt, flags, out=None, workspace=None):
    """snerf_outline_rank -> (ring, rank, ordinal (E) int32, totals (E, 2) int32, stats (2) int64: guard trips, the sum of the rings'
    edge counts).  On a permutation `next` the stats are (0, E); any other `next` still returns, with other stats.  `out`: the four
    buffers to write into; `workspace`: workspace_bytes(E) bytes on the GPU.  E == 0 launches nothing."""
    E = int(nxt.numel())
    nxt, flags = _words(nxt, E, "next"), _words(flags, E, "flags")
    dev = nxt.device
    if out is None:
        out = tuple(torch.empty(E, dtype=torch.int32, device=dev) for _ in range(3)) + (torch.empty((E, 2), dtype=torch.int32, device=dev),)
    ring, rank, ordinal, totals = (_words(t, n, name) for t, n, name in zip(out, (E, E, E, 2 * E), ("ring", "rank", "ordinal", "totals")))
    need = workspace_bytes(E)
    if workspace is None:
        workspace = torch.empty(need // 4, dtype=torch.int32, device=dev)
    elif not (torch.is_tensor(workspace) and workspace.is_cuda and workspace.is_contiguous()
              and workspace.numel() * workspace.element_size() >= need and workspace.data_ptr() % 4 == 0):
        raise ValueError(f"outline: workspace must be a contiguous, 4-byte aligned GPU tensor of at least {need} bytes")
    stats = torch.zeros(2, dtype=torch.int64, device=dev)
    _lib.call("snerf_outline_rank", nxt, flags, E, ring, rank, ordinal, totals, workspace, need, stats, device=dev, exc=ValueError)
    return ring, rank, ordinal, totals, stats


def new_rows(n_rings, device):
    """(n_rings, 8) int64 holding the initial u64 words of snerf_outline_emit"""
    return torch.tensor(_ROW_INIT, dtype=torch.int64, device=device).repeat(n_rings, 1)


def emit(ids, slot, flags, ring, ordinal, ring_row, vertex_offset, n_rings, V, vertices=None):
    """snerf_outline_emit -> (vertices (V, 2) int32, rows (n_rings, 8) int64 holding the u64 words, stats (2) int64: guard trips,
    vertices written).  E == 0 launches nothing."""
    ids = _ids(ids)
    h, w = ids.shape
    E, n_rings, V = int(slot.numel()), int(n_rings), int(V)
    vertices = torch.empty((V, 2), dtype=torch.int32, device=ids.device) if vertices is None else _words(vertices, 2 * V, "vertices")
    rows = new_rows(n_rings, ids.device)
    stats = torch.zeros(2, dtype=torch.int64, device=ids.device)
    _lib.call("snerf_outline_emit", ids, _words(slot, E, "slot"), _words(flags, E, "flags"), _words(ring, E, "ring"),
              _words(ordinal, E, "ordinal"), _words(ring_row, E, "ring_row"), _words(vertex_offset, n_rings, "vertex_offset", torch.int64),
              h, w, E, n_rings, V, vertices, rows, stats, exc=ValueError)
    return vertices, rows, stats


def ring_rows(ring, totals):
    """what lies between rank_rings and emit, in plain torch -> (ring_row (E) int32: the ring's row at its start, -1 elsewhere;
    vertex_offset (n_rings) int64; n_rings; V).  The rings are in ascending order of start; reading V is a host synchronisation."""
    E = ring.numel()
    starts = torch.nonzero(ring == torch.arange(E, dtype=torch.int32, device=ring.device)).reshape(-1)
    n_rings = int(starts.numel())
    ring_row = torch.full((E,), -1, dtype=torch.int32, device=ring.device)
    ring_row[starts] = torch.arange(n_rings, dtype=torch.int32, device=ring.device)
    counts = totals.reshape(-1, 2)[starts, 1].long()
    total = torch.cumsum(counts, 0)
    return ring_row, (total - counts).contiguous(), n_rings, int(total[-1].item()) if n_rings else 0


def rings(ids, K, connectivity=4):
    """The boundary rings of the objects 1..K of `ids` ((H, W) int32 on the GPU), traced at `connectivity` -- the one the ids were
    labelled with -> a dict of numpy arrays:
      vertices (V, 2) int32      the rings' corners as lattice (x, y) = (column, row), ring after ring, each in ring order
      ring_start (R + 1) int64   ring r owns vertices[ring_start[r]:ring_start[r + 1]]
      ring_object (R) int64      the id of the object on the ring's right
      ring_area2 (R) int64       the doubled signed area in cells: positive = an outer ring (clockwise on the north-up map),
                                 negative = a hole
      ring_edges (R) int64       the ring's length in unit edges
      ring_bbox (R, 4) int64     min x, max x, min y, max y
      stats                      {"bad_ids", "object_cells", "edges", "corners", "rings"} as Python ints
    Any non-zero guard word raises a RuntimeError, as does a successor map that is no permutation."""
    ids = _ids(ids)
    K = _K(K)
    side_bits, sstats = sides(ids, K)
    offsets, E = offsets_of(side_bits)
    s = [int(v) for v in sstats.cpu()]
    if s[2] != E:
        raise RuntimeError(f"outline.rings: {s[2]} edges counted but the sides hold {E}")
    slot, nxt, flags, lstats = link(ids, side_bits, offsets, K, connectivity, E)
    ring, _, ordinal, totals, rstats = rank_rings(nxt, flags)
    l, r = ([int(v) for v in t.cpu()] for t in (lstats, rstats))
    if l != [0, E] or r != [0, E]:
        raise RuntimeError(f"outline.rings: the successor map is no permutation of the {E} edges (link guard {l[0]}, written {l[1]}; "
                           f"rank guard {r[0]}, ring edges {r[1]})")
    ring_row, vertex_offset, n_rings, V = ring_rows(ring, totals)
    vertices, rows, estats = emit(ids, slot, flags, ring, ordinal, ring_row, vertex_offset, n_rings, V)
    e = [int(v) for v in estats.cpu()]
    if e != [0, V] or V != s[3]:
        raise RuntimeError(f"outline.rings: emit guard {e[0]}, {e[1]} of {V} vertices written, {s[3]} corners counted")
    rows = rows.cpu().numpy()
    return {"vertices": vertices.cpu().numpy(), "ring_start": np.concatenate([vertex_offset.cpu().numpy(), [V]]).astype(np.int64),
            "ring_object": rows[:, 2].copy(), "ring_area2": rows[:, 3].copy(), "ring_edges": rows[:, 0].copy(), "ring_bbox": rows[:, 4:8].copy(),
            "stats": {"bad_ids": s[0], "object_cells": s[1], "edges": E, "corners": V, "rings": n_rings}}


# ---- polygons: host side -----------------------------------------------------------------------------------------------------------------
def polygons(rings):
    """rings()'s result -> {object id: [outer ring, hole, ...]} in ascending id, every ring a (n, 2) int64 array of lattice (x, y), open
    (the last vertex is not the first again), the holes in ring order.  An id without a ring of positive area, or with more than one,
    is a ValueError: its cells are not one component of the connectivity the rings were traced with."""
    start, obj, area2 = rings["ring_start"], rings["ring_object"], rings["ring_area2"]
    outer, holes = {}, {}
    for r in range(len(obj)):
        n = int(obj[r])
        ring = np.asarray(rings["vertices"][int(start[r]):int(start[r + 1])], np.int64)
        if area2[r] > 0:
            outer.setdefault(n, []).append(ring)
        else:
            holes.setdefault(n, []).append(ring)
    for n in sorted(set(outer) | set(holes)):
        if len(outer.get(n, ())) != 1:
            raise ValueError(f"outline.polygons: object {n} has {len(outer.get(n, ()))} rings of positive area: the ids are not the "
                             "components of this connectivity")
    return {n: outer[n] + holes.get(n, []) for n in sorted(outer)}


def _dist2(p, a, b):
    """the squared distance of the lattice point p from the segment a b, exactly"""
    abx, aby, apx, apy = b[0] - a[0], b[1] - a[1], p[0] - a[0], p[1] - a[1]
    len2, dot = abx * abx + aby * aby, apx * abx + apy * aby
    if dot <= 0:
        return Fraction(apx * apx + apy * apy)
    if dot >= len2:
        return Fraction((p[0] - b[0]) ** 2 + (p[1] - b[1]) ** 2)
    cross = abx * apy - aby * apx
    return Fraction(cross * cross, len2)


def _simplify_ring(ring, t2):
    pts = [(int(x), int(y)) for x, y in ring]
    if len(pts) < 3:
        return ring
    return np.array([pts[k] for k in _ring_keep(pts, t2)], np.int64).reshape(-1, 2)


def _ring_keep(pts, t2):
    """the ordinals of the vertices that simplify keeps of a ring of at least 3 lattice points, ascending"""
    n = len(pts)
    far = max(range(n), key=lambda k: ((pts[k][0] - pts[0][0]) ** 2 + (pts[k][1] - pts[0][1]) ** 2, -k))
    closed = pts + [pts[0]]
    keep = {0, far}
    stack = [(0, far), (far, n)]
    while stack:
        a, b = stack.pop()
        if b - a < 2:
            continue
        d2, k = max(((_dist2(closed[k], closed[a], closed[b]), -k) for k in range(a + 1, b)))
        if d2 > t2:
            keep.add(-k)
            stack += [(a, -k), (-k, b)]
    return sorted(keep)


def _open_keep(pts, t2):
    """the same for an open polyline whose two endpoints stay"""
    keep = {0, len(pts) - 1}
    stack = [(0, len(pts) - 1)]
    while stack:
        a, b = stack.pop()
        if b - a < 2:
            continue
        d2, k = max(((_dist2(pts[k], pts[a], pts[b]), -k) for k in range(a + 1, b)))
        if d2 > t2:
            keep.add(-k)
            stack += [(a, -k), (-k, b)]
    return sorted(keep)


def simplify(polygons, tolerance_cells):
    """Douglas-Peucker on every ring, in cells: the ring is cut at its first vertex and at the vertex farthest from it (the lowest
    ordinal at a tie), each half keeps the vertex farthest from its chord while that distance exceeds the tolerance (again the lowest
    ordinal at a tie).  The distance is the one from the chord as a SEGMENT, so every dropped vertex lies within the tolerance of the
    kept ring; all comparisons are exact (cross^2 > t^2 len^2 in Python integers, t = fractions.Fraction(tolerance_cells)).  A hole left
    with fewer than 3 vertices is dropped, an outer ring left with fewer than 3 is kept unsimplified.  Rings are simplified one by one:
    neighbours may part or overlap by up to the tolerance, and a ring may come to cross itself.  tolerance_cells = 0 returns its input."""
    t = Fraction(tolerance_cells)
    if t < 0:
        raise ValueError(f"outline.simplify: tolerance_cells = {tolerance_cells!r} is negative")
    if t == 0:
        return polygons
    out = {}
    for n, ring_list in polygons.items():
        outer = _simplify_ring(ring_list[0], t * t)
        holes = [_simplify_ring(r, t * t) for r in ring_list[1:]]
        out[n] = [outer if len(outer) >= 3 else ring_list[0]] + [r for r in holes if len(r) >= 3]
    return out


def _area2(pts):
    return sum(x0 * y1 - x1 * y0 for (x0, y0), (x1, y1) in zip(pts, pts[1:] + pts[:1]))


def arc_points(arcs, a):
    """the vertices of arc `a` of arcs.arcs()'s result as a list of (x, y) Python ints"""
    start = arcs["arc_start"]
    return [(int(x), int(y)) for x, y in arcs["vertices"][int(start[a]):int(start[a + 1])]]


def simplify_shared(arcs, tolerance_cells):
    """Gap-free Douglas-Peucker: `arcs` is what arcs.arcs() returns for an id raster -> {id: [outer ring, hole, ...]} in the format of
    polygons().  Every OWNER open arc is simplified once, with the distance of simplify() and both endpoints (nodes) fixed; a closed arc
    goes through the ring rule of simplify(); an arc that is no owner takes its twin's result, reversed: a border two ids share is one
    polyline in both polygons, so neighbours neither part nor overlap.  A ring is the concatenation of its arcs.  Where a region comes
    out with an outer ring of fewer than 3 vertices or of non-positive doubled area, all the arcs of its rings (and their twins) are put
    back unsimplified and the rings are assembled again, until no region is in that state: at most as many passes as there are arcs.  A
    hole left with fewer than 3 vertices is dropped.  With a tolerance above 0 the nodes stay vertices of the rings, also where the
    ring runs straight through them: every segment of a polygon then has its reverse in the neighbour's.  tolerance_cells = 0 returns
    what polygons(rings()) returns, vertex for vertex: the rings without the nodes that are no corners, from the ring's start."""
    t = Fraction(tolerance_cells)
    if t < 0:
        raise ValueError(f"outline.simplify_shared: tolerance_cells = {tolerance_cells!r} is negative")
    t2 = t * t
    A = len(arcs["right"])
    closed, owner, twin, edges = (np.asarray(arcs[k]).tolist() for k in ("closed", "owner", "twin", "edges"))
    full = [arc_points(arcs, a) for a in range(A)]
    frozen = [t == 0] * A

    def keep_of():
        keep = [None] * A
        for a in range(A):
            if owner[a] or twin[a] < 0:
                n = len(full[a])
                if frozen[a] or n < 3:
                    keep[a] = list(range(n))
                else:
                    keep[a] = _ring_keep(full[a], t2) if closed[a] else _open_keep(full[a], t2)
        for a in range(A):
            if keep[a] is None:
                b = twin[a]
                if closed[a]:
                    kept = {full[b][k] for k in keep[b]}
                    keep[a] = [k for k, v in enumerate(full[a]) if v in kept]
                else:
                    if len(full[a]) != len(full[b]):
                        raise ValueError(f"outline.simplify_shared: arc {a} and its twin {b} differ in their vertices")
                    keep[a] = sorted(len(full[a]) - 1 - k for k in keep[b])
        return keep

    def ring_of(r, keep):
        pts, dist, d0 = [], [], 0
        for a in arcs["ring_arcs"][r].tolist():
            P = full[a]
            cum = [0]
            for (x0, y0), (x1, y1) in zip(P, P[1:]):
                cum.append(cum[-1] + abs(x1 - x0) + abs(y1 - y0))
            idx = keep[a] if closed[a] else keep[a][:-1]
            pts += [P[k] for k in idx]
            dist += [d0 + cum[k] for k in idx]
            d0 += edges[a]
        if t == 0:
            n = len(pts)
            corner = [(pts[k][0] - pts[k - 1][0]) * (pts[(k + 1) % n][1] - pts[k][1])
                      != (pts[k][1] - pts[k - 1][1]) * (pts[(k + 1) % n][0] - pts[k][0]) for k in range(n)]
            pts, dist = [v for v, c in zip(pts, corner) if c], [d for d, c in zip(dist, corner) if c]
        L = int(arcs["ring_edges"][r])
        offset = (L - int(arcs["ring_first"][r])) % L
        turn = next((k for k, d in enumerate(dist) if d >= offset), 0)
        return pts[turn:] + pts[:turn]

    rings = arcs["rings"]
    obj, area2 = np.asarray(rings["ring_object"]).tolist(), np.asarray(rings["ring_area2"]).tolist()
    R = len(obj)
    for _ in range(A + 1):
        keep = keep_of()
        out = [ring_of(r, keep) for r in range(R)]
        bad = {obj[r] for r in range(R) if area2[r] > 0 and (len(out[r]) < 3 or _area2(out[r]) <= 0)}
        thaw = [a for r in range(R) if obj[r] in bad for a in arcs["ring_arcs"][r].tolist() if not frozen[a]]
        if not thaw:
            break
        for a in thaw:
            frozen[a] = True
            if twin[a] >= 0:
                frozen[twin[a]] = True
    outer, holes = {}, {}
    for r in range(R):
        ring = np.array(out[r], np.int64).reshape(-1, 2)
        if area2[r] > 0:
            outer.setdefault(obj[r], []).append(ring)
        elif len(ring) >= 3:
            holes.setdefault(obj[r], []).append(ring)
    for n in sorted(outer):
        if len(outer[n]) != 1:
            raise ValueError(f"outline.simplify_shared: object {n} has {len(outer[n])} rings of positive area: the ids are not the "
                             "components of this connectivity")
    return {n: outer[n] + holes.get(n, []) for n in sorted(outer)}


def to_map(polygons, grid):
    """lattice vertices -> map coordinates: east = xoff + x res, north = yoff - y res in fp64, as object_table's bounding box -> the same
    structure with (n, 2) float64 arrays of (east, north).  `grid`: the raster's lattice (a DsmGrid, or a _lib.SnerfDsmGrid window)."""
    g = OR.window_grid(grid)
    xoff, yoff, res = float(g.xoff), float(g.yoff), float(g.resolution)
    return {n: [np.stack([xoff + r[:, 0].astype(np.float64) * res, yoff - r[:, 1].astype(np.float64) * res], 1) for r in ring_list]
            for n, ring_list in polygons.items()}


def geojson(polygons, grid, zone_string=None, properties=None):
    """a GeoJSON FeatureCollection (a dict, ready for json.dump): one Polygon feature per object, its rings closed, the exterior ring
    first.  The rings are traced clockwise on a north-up map (holes the other way); the right-hand rule wants the exterior
    counter-clockwise in (east, north), so every ring is written from its first vertex in REVERSE order.  With `zone_string` a named `crs` member
    urn:ogc:def:crs:EPSG::<utm_epsg(zone_string)> (the coordinates are UTM metres, not RFC 7946's WGS 84 degrees).  `properties`: a list of
    records with an "id" (objects.table_records / roofs.table_records): a feature takes the record of its id, else {"id": n}."""
    from ...framework.util.img_utils import utm_epsg
    by_id = {int(rec["id"]): rec for rec in (properties or [])}
    features = []
    for n, ring_list in to_map(polygons, grid).items():
        coords = [[[float(e), float(nn)] for e, nn in np.concatenate([r[:1], r[:0:-1], r[:1]])] for r in ring_list]
        features.append({"type": "Feature", "id": int(n), "properties": dict(by_id.get(int(n), {"id": int(n)})),
                         "geometry": {"type": "Polygon", "coordinates": coords}})
    doc = {"type": "FeatureCollection", "features": features}
    if zone_string is not None:
        doc["crs"] = {"type": "name", "properties": {"name": f"urn:ogc:def:crs:EPSG::{utm_epsg(zone_string)}"}}
    return doc


def footprints(ids, K, grid, connectivity=4, simplify_m=0.0, zone_string=None, properties=None):
    """rings, polygons, simplify (`simplify_m` metres, 0 = none) and geojson in one call -> (FeatureCollection, rings()'s result)"""
    res = float(OR.window_grid(grid).resolution)
    r = rings(ids, K, connectivity)
    polys = simplify(polygons(r), Fraction(simplify_m) / Fraction(res))
    return geojson(polys, grid, zone_string, properties), r
