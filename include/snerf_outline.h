/* Extension of the C-ABI of libsnerf_hip.so: outlines on the map -- the boundary rings of the objects of an id raster as ordered
 * lattice vertices, what turns the footprints of objects() and the facets of roofs() into polygons.  A map product of this project
 * (the reference has no counterpart); parity with rasterio.features.shapes / gdal_polygonize is UNPINNED (neither is part of this
 * build).  DESIGN.md section 5ze, restated in numpy by tests/outline_numpy.py.
 *
 * include/snerf_hip.h is the ABI-6 surface and its list of entry points is frozen; an entry added at the same ABI version is
 * declared in a header of its own (as include/snerf_objects.h), which includes it for the error codes and the limits.  Same
 * conventions: plain pointers + sizes, device pointers unless stated, `stream` is a hipStream_t, 0 = SNERF_OK, a message for every
 * other return through snerf_last_error(); no entry allocates or synchronises with the host, and none launches anything for an
 * empty problem.  snerf_version() stays 6.
 * The Python binding is this header's group of rows in _lib.LATER_HEADER_SIGNATURES (tests/test_outline_cpu.py compares it with this
 * file).
 *
 * GEOMETRY.  A raster is (h, w), row 0 the north edge, cell c = j * w + i (row j, column i); h * w < 2^29, so that an edge slot fits
 * an int32.  ids (h, w) int32: 0 = background, n in [1, K] = object n; an id outside [0, K] counts as 0.  Vertices lie on the
 * (h + 1) x (w + 1) lattice, (x, y) = (column, row): cell (j, i) has the corners (i, j), (i + 1, j), (i + 1, j + 1), (i, j + 1).
 * A boundary EDGE belongs to a cell with an id n > 0 and to one of its sides s: 0 = N, 1 = E, 2 = S, 3 = W.  It exists where the
 * neighbour across that side carries another id or lies outside the raster.  It is directed with its own cell on its right
 * (clockwise on the screen), tail -> head:
 *     N  (i, j) -> (i + 1, j)        E  (i + 1, j) -> (i + 1, j + 1)        S  (i + 1, j + 1) -> (i, j + 1)        W  (i, j + 1) -> (i, j)
 * Its SLOT is 4 c + s; its compact index p is its position among all existing edges in ascending slot order; E is their number.
 *
 * SUCCESSOR.  With the heading d = s and the unit steps step(0..3) = E, S, W, N = (0, 1), (1, 0), (0, -1), (-1, 0) in (row, column),
 * let b = own cell + step(d) and a = b + step((d + 3) mod 4); a cell outside the raster carries no id.  The successor of the edge is
 *     id(b) == n and id(a) == n                       side (d + 3) mod 4 of a        (a left turn)
 *     id(b) == n only                                 side d of b                    (straight on)
 *     id(b) != n, id(a) == n, connectivity == 8       side (d + 3) mod 4 of a        (across the diagonal)
 *     otherwise                                       side (d + 1) mod 4 of the own cell   (a right turn)
 * The successor map is a permutation of the edges; its cycles are the RINGS.  Traced at the connectivity its ids were labelled with,
 * an object has exactly one ring of positive doubled area (below) -- the outer ring -- and one of negative area per hole.
 * CORNER.  An edge is a corner when its predecessor has another heading.  With r = own cell - step(d) and l = r + step((d + 3) mod 4)
 * -- the two cells behind the edge's tail -- the edge is NO corner exactly when id(r) == n and id(l) != n (its predecessor is then
 * side d of r); the rule does not depend on the connectivity.  The corners of a ring, in ring order, are the polygon's vertices.
 *
 * Everything is integer arithmetic; the ranking uses no atomics outside its two counting passes (which add to stats), the reductions
 * integer atomics only: no word depends on launch order or on the grid shape.  Every loop has a trip count fixed on the host: no content of any buffer can turn a launch into a
 * hang, and an index read from a buffer is checked before it is used as one. */
#ifndef SNERF_OUTLINE_H
#define SNERF_OUTLINE_H

#include "snerf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SNERF_OUTLINE_ROW_WORDS 8
#define SNERF_OUTLINE_MAX_CELLS 536870912 /* 2^29: a raster has FEWER cells */
#define SNERF_OUTLINE_CORNER 1            /* flags: bit 0 = the edge is a corner; bits 1-2 = its side */

/* snerf_outline_sides: which sides of every cell are boundary edges, one launch.
 *   ids (h, w) int32;  K: the largest id;
 *   sides (h * w) u8: EVERY byte is written: bit s set = side s of the cell is an edge (0 for a cell without an id);
 *   stats[4] u64, zeroed by the caller:  [0] cells whose id lies outside [0, K],  [1] object cells,  [2] boundary edges E,
 *     [3] corner edges.
 * The host then forms offsets = the exclusive cumulative sum of popcount(sides) and reads E.
 * Refused without touching the device: a null ids, sides or stats; h or w < 1; h * w >= 2^29; K outside [0, 2^31). */
int snerf_outline_sides(const int* ids, int h, int w, long long K, unsigned char* sides, unsigned long long* stats, void* stream);

/* snerf_outline_link: the edges in compact order with their successors, one launch, one thread per cell.
 *   ids, K as above;  sides (h * w) u8 as snerf_outline_sides wrote them;  offsets (h * w) int32: the compact index of a cell's first
 *   edge;  connectivity: 4 or 8;  E: the number of edges;
 *   slot, next, flags (E) int32: for the edge of side s of cell c, at p = offsets[c] + popcount(sides[c] & ((1 << s) - 1)):
 *     slot[p] = 4 c + s;  next[p] = the compact index of its successor, formed the same way from the successor's cell and side;
 *     flags[p] = (corner ? 1 : 0) | s << 1.
 *   stats[2] u64, zeroed by the caller:  [0] guard trips,  [1] edges written.
 * Only the set bits of an OBJECT cell (id in [1, K]) are edges.  An edge whose p or whose successor's index lies outside [0, E) adds
 * 1 to stats[0] and writes none of its three words: the offsets then do not belong to these sides, and nothing lands out of place.
 * Refused without touching the device: a null pointer (with E > 0); sizes and K as snerf_outline_sides; a connectivity other than 4
 * or 8; E outside [0, 4 h w].  E == 0 launches nothing. */
int snerf_outline_link(const int* ids, const unsigned char* sides, const int* offsets, int h, int w, long long K, int connectivity,
                       long long E, int* slot, int* next, int* flags, unsigned long long* stats, void* stream);

/* snerf_outline_workspace_bytes: the bytes snerf_outline_rank needs for E edges (24 E: six int32 arrays), 0 for E == 0; -1 for a
 * refusal: E outside [0, 2^31). */
long long snerf_outline_workspace_bytes(long long E);

/* snerf_outline_rank: ring, rank and corner ordinal of every edge by pointer jumping.
 *   next, flags (E) int32 as snerf_outline_link wrote them (of flags only bit 0 is read);
 *   ring (E) int32:     the lowest compact index on the edge's cycle -- the ring's START;
 *   rank (E) int32:     the steps along `next` from ring[p] to p;
 *   ordinal (E) int32:  the number of corner edges of the ring whose rank is below rank[p];
 *   totals (E, 2) int32: at a ring's start (edges, corners) of the ring, (0, 0) at every other edge;
 *   workspace: snerf_outline_workspace_bytes(E) bytes at least, 4-byte aligned;
 *   stats[2] u64, zeroed by the caller:  [0] guard trips,  [1] the sum of the rings' edge counts.
 * With R = ceil(log2(max(E, 2))) rounds fixed by the entry, 2 R + 4 launches of one thread per edge, double-buffered in the workspace:
 *   1. minimum  m[p] = p, t[p] = next[p];  R times  m'[p] = min(m[p], m[t[p]]), t'[p] = t[t[p]]:  ring[p] = m[p];
 *   2. cut      q[p] = NIL where ring[next[p]] == next[p] (the successor is a start), else next[p];  with the weights (1, corner bit)
 *               of the successor  u[p] = (q[p] == NIL ? 0 : 1),  v[p] = (q[p] == NIL ? 0 : corner(q[p]));
 *   3. ranking  R times, where q[p] != NIL:  u'[p] = u[p] + u[q[p]], v'[p] = v[p] + v[q[p]], q'[p] = q[q[p]]  (Wyllie): u[p] is then
 *               the number of edges behind p up to its ring's end, v[p] the corners among them;
 *   4. finish   with s = ring[p], L = u[s] + 1, C = v[s] + corner(s):  rank[p] = L - 1 - u[p], ordinal[p] = C - v[p] - corner(p),
 *               totals[p] = (L, C) where p == s, else (0, 0);
 *   5. check    stats[0] += the edges with ring[next[p]] != ring[p], and the edges with rank[next[p]] != rank[p] + 1 while
 *               next[p] != ring[p];  stats[1] += totals[p][0].
 * A next[p] outside [0, E) is read as p in every pass and adds 1 to stats[0] (once, in the first).  The sums are unsigned 32-bit and
 * wrap.  On a permutation stats[0] == 0 and stats[1] == E; whatever `next` holds, every index used lies in [0, E) and the launches
 * are the same 2 R + 4.
 * Refused without touching the device: a null pointer (with E > 0); E outside [0, 2^31); a workspace that is not 4-byte aligned;
 * workspace_bytes below snerf_outline_workspace_bytes(E).  E == 0 launches nothing. */
int snerf_outline_rank(const int* next, const int* flags, long long E, int* ring, int* rank, int* ordinal, int* totals, void* workspace,
                       long long workspace_bytes, unsigned long long* stats, void* stream);

/* snerf_outline_emit: the polygon vertices and the per-ring reductions, one launch, one thread per edge.
 *   ids (h, w) int32;  slot, flags, ring, ordinal (E) int32 as written above;
 *   ring_row (E) int32, read at ring starts only: the row r of the ring that starts there (the rings in ascending order of start);
 *   vertex_offset (n_rings) int64: the first vertex of ring r -- the exclusive cumulative sum of the rings' corner counts;
 *   vertices (V, 2) int32: a corner edge writes its tail (x, y) to vertices[vertex_offset[r] + ordinal[p]]; nothing else is written;
 *   rows (n_rings, 8) u64, INITIALISED by the caller to the pattern below and only accumulated:
 *     word  content                                                                         init
 *      0    edges                                                                           0
 *      1    corner edges                                                                    0
 *      2    the object id (an atomic max; the edges of a ring agree; a negative id as 0)    0
 *      3    the doubled signed area: the sum of x0 y1 - x1 y0 over the ring's unit edges (tail 0, head 1), two's complement     0
 *      4, 5 min x, max x of the tails                                                       2^64 - 1, 0
 *      6, 7 min y, max y of the tails                                                       2^64 - 1, 0
 *   stats[2] u64, zeroed by the caller:  [0] guard trips,  [1] vertices written.
 * A ring of positive area (in these lattice coordinates, y growing south) is an outer ring; it runs clockwise on the screen and, the
 * raster being north-up, clockwise on the map as well: in (east, north) its shoelace sum is negative, and a writer that follows
 * GeoJSON's right-hand rule reverses it (eval/utils/outline.py geojson).  A ring of negative area is a hole.
 * The lanes of a wave that share a ring reduce their values inside the wave, and the wave holds the result while its next edges
 * belong to the same ring, before one lane issues the row's atomics: the words are integer sums and extremes, so the grouping does not
 * show in them.
 * Guards, each adding 1 to stats[0]: a slot outside [0, 4 h w), a ring[p] outside [0, E) or a ring_row outside [0, n_rings) -- the
 * edge then writes and folds nothing; a vertex_offset[r] outside [0, V] (tested before anything is added to it) or a vertex position outside [0, V) -- the vertex is
 * not written, the edge is still folded.
 * Refused without touching the device: a null pointer (with E > 0); sizes as snerf_outline_sides; E, V or n_rings outside [0, 4 h w].
 * E == 0 launches nothing. */
int snerf_outline_emit(const int* ids, const int* slot, const int* flags, const int* ring, const int* ordinal, const int* ring_row,
                       const long long* vertex_offset, int h, int w, long long E, long long n_rings, long long V, int* vertices,
                       unsigned long long* rows, unsigned long long* stats, void* stream);

#ifdef __cplusplus
}
#endif
#endif
