/* Extension of the C-ABI of libsnerf_hip.so: roof lines as vectors -- facets grown over the cells the facet filter dropped, so that
 * neighbouring facets touch, and the ARCS of a partition: the maximal runs of boundary edges between two NODES, each with the id on its
 * right and on its left and paired with the same run in the neighbour's ring.  What turns the facets of roofs() into ridge, hip, eave
 * and step lines and into polygons that share their borders.  A map product of this project (the reference has no counterpart).
 * DESIGN.md section 5zf, restated in numpy by tests/rooflines_numpy.py.
 *
 * Conventions as include/snerf_outline.h, which this header builds on: plain pointers + sizes, device pointers unless stated, `stream`
 * is a hipStream_t, 0 = SNERF_OK, a message for every other return through snerf_last_error(); no entry allocates or synchronises with
 * the host, and none launches anything for an empty problem.  snerf_version() stays 6.  The Python binding is this header's group of
 * rows in _lib.LATER_HEADER_SIGNATURES (tests/test_rooflines_cpu.py compares it with this file).
 *
 * GEOMETRY, EDGES, RINGS: include/snerf_outline.h.  The arcs sit on what snerf_outline_sides / _link / _rank wrote for the same ids at
 * the same K: sides, offsets, slot, flags, ring, rank, totals.
 *
 * LEFT.  left(p) of the edge of side s of cell (j, i) is the id of the cell across that side -- (j - 1, i), (j, i + 1), (j + 1, i),
 * (j, i - 1) for N, E, S, W -- and 0 when that cell lies outside the raster or its id lies outside [1, K].
 * TWIN.  For left(p) > 0 the same unit segment is side (s + 2) mod 4 of the cell across, t: twin(p) = offsets[t] +
 * popcount(sides[t] & ((1 << ((s + 2) mod 4)) - 1)), the index snerf_outline_link forms.  twin(p) = -1 where left(p) == 0.
 * NODE.  A lattice vertex (x, y) has the four cells NW (y - 1, x - 1), NE (y - 1, x), SE (y, x), SW (y, x - 1) round it, read on the
 * raster padded with 0 (an id outside [0, K] as 0).  It is a node when [NW != NE] + [NE != SE] + [SE != SW] + [SW != NW] >= 3: three
 * or more ids meet there, or two meet at a saddle.  The rule does not depend on the connectivity.
 * BREAK.  An edge breaks an arc when its tail is a node.
 * ARC.  A maximal run of a ring's edges from one break up to the next; a ring without a break is one CLOSED arc.  left(p) is constant
 * within an arc, and the twins of an arc's edges are an arc of the neighbour's ring in reverse order.
 * POSITION.  With L the ring's edge count, first = the lowest rank among the ring's break edges (0 when it has none) and base = the
 * exclusive cumulative sum of the rings' edge counts, the rings in ascending order of start:  pos(p) = base + (rank[p] - first) mod L.
 * Positions run ring after ring and, inside a ring, from a break: no arc wraps.
 * FLAGS.  hf(pos) = break or pos == base (the position is an arc's first);  vf(pos) = break or corner (the edge's tail is a vertex of
 * its arc).  The arc of a position is the inclusive cumulative sum of hf, minus 1: arcs are numbered in ring order.
 * VERTICES.  An OPEN arc (its first edge is a break) has the tails of its vf edges in order and then the head of its last edge:
 * sum(vf) + 1 vertices.  A closed arc has its corners from the ring's start, sum(vf) of them: the ring's vertex list of
 * snerf_outline_emit.
 * The cumulative sums between the launches are the host's (eval/utils/arcs.py forms them on the device, in plain torch).
 *
 * Integer arithmetic and integer atomics only in the three arc entries; every trip count is fixed on the host; every index read from a
 * buffer is range-checked, and counted, before it is used. */
#ifndef SNERF_ROOFLINES_H
#define SNERF_ROOFLINES_H

#include "snerf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SNERF_ARCS_ROW_WORDS 12
#define SNERF_ARCS_NO_FIRST 2147483647 /* the initial word of `first`: no break edge seen */
#define SNERF_GROW_MAX_ROUNDS 64

/* snerf_roofs_grow: the kept facets of roofs.filter_facets grown over the building cells that carry no facet, `rounds` launches.
 *   fids (h, w) int32 in [0, F]: the kept facets;  ids (h, w) int32: the objects;  key (h, w) int32: the key plane of terrain.keys;
 *   facet_root (F) int32: the linear index of every facet's root cell (facet_table's "root");
 *   planes (F, 3) f64: (gamma, alpha, beta) per facet in key units, as snerf_roofs_residuals takes them;
 *   unit: key units per residual step;  max_rq: the largest misfit, in steps, a cell may have from the facet it joins;
 *   a, b (h, w) int32: round 0 reads fids, round r > 0 what round r - 1 wrote; round r writes EVERY word of a (r even) or b (r odd):
 *     the result lies in a when `rounds` is odd, in b when it is even.  Jacobi: a round reads only what the round before wrote, so
 *     the result depends neither on the launch order nor on any banding.
 *   stats (rounds + 1) u64, zeroed by the caller:  [r] cells assigned in round r,  [rounds] guard trips.
 * In a round a cell is a TAKER when its object id is > 0, its facet id is 0 and its key is valid (neither SNERF_TERRAIN_HOLE nor
 * 2^31 - 1).  It looks at its N, E, S, W neighbours inside the raster.  The neighbour's facet n is a CANDIDATE when n lies in [1, F],
 * the neighbour has the taker's object id, the three plane words of n are finite, and the root of n lies in [0, h w) and has a valid
 * key.  The candidate's misfit is |rq| with rq exactly as snerf_roofs_residuals forms it for a cell of facet n: di, dj, dk relative to
 * the root of n, e = dk - ((gamma + alpha di) + beta dj), t = rint(e / unit), clamped at +-2^18 (one device function serves both
 * entries).  The taker takes the candidate with the smallest (|rq|, n) among those that are not clamped and have |rq| <= max_rq; it
 * stays 0 when there is none.  Every other cell keeps its word: a cell with a facet id > 0 is never changed.
 * Guards, each adding 1 to stats[rounds] in every round it is met: a cell whose own word lies outside [0, F] (the word is copied and
 * never used as an index; as a neighbour it is no candidate); a candidate whose root lies outside [0, h w) (it is no candidate).
 * Refused without touching the device: a null pointer (planes and facet_root may be null when F == 0); h or w outside
 * [1, SNERF_ROOFS_MAX_SIDE]; F outside [0, 2^27); rounds outside [1, SNERF_GROW_MAX_ROUNDS]; a unit that is not finite and > 0; a
 * negative max_rq.  F == 0 copies fids into the result buffer and launches nothing. */
int snerf_roofs_grow(const int* fids, const int* ids, const int* key, const int* facet_root, const double* planes, int h, int w,
                     long long F, double unit, long long max_rq, int rounds, int* a, int* b, unsigned long long* stats, void* stream);

/* snerf_arcs_first: the node bit of every edge's tail and the first break of every ring, one launch, one thread per edge.
 *   ids (h, w) int32, K;  slot, ring, rank (E) int32 as snerf_outline_link / _rank wrote them;
 *   node (E) int32: 1 where the edge's tail is a node, else 0;
 *   first (E) int32, INITIALISED by the caller to SNERF_ARCS_NO_FIRST: a break edge folds its rank into first[ring[p]] by an integer
 *     atomicMin; only the words at ring starts are touched;
 *   stats[2] u64, zeroed by the caller:  [0] guard trips,  [1] break edges.
 * Guards, each adding 1 to stats[0]: a slot outside [0, 4 h w) -- the edge writes nothing; a ring[p] outside [0, E) -- the node word
 * is written, nothing is folded.
 * Refused without touching the device: a null pointer (with E > 0; ids and stats always); h or w < 1; h * w >= 2^29; K outside
 * [0, 2^31); E outside [0, 4 h w].  E == 0 launches nothing. */
int snerf_arcs_first(const int* ids, const int* slot, const int* ring, const int* rank, int h, int w, long long K, long long E, int* node,
                     int* first, unsigned long long* stats, void* stream);

/* snerf_arcs_mark: left, twin and the ring-ordered position of every edge, one launch, one thread per edge.
 *   ids, K;  sides (h * w) u8 and offsets (h * w) int32 as for snerf_outline_link;  slot, flags, ring, rank (E), totals (E, 2) int32;
 *   node, first (E) int32 as snerf_arcs_first left them;
 *   ring_row (E) int32, read at ring starts only: the row r of the ring (outline.ring_rows);
 *   ring_base (n_rings) int64: the exclusive cumulative sum of the rings' edge counts;
 *   left, twin, pos_of (E) int32 by edge;  order, hf, vf (E) int32 by position:  order[pos(p)] = p, hf and vf as defined above.
 *   stats[4] u64, zeroed by the caller:  [0] guard trips,  [1] edges written,  [2] break edges,  [3] edges with a twin.
 * first[s] == SNERF_ARCS_NO_FIRST is read as 0.
 * Guards, each adding 1 to stats[0]: a slot outside [0, 4 h w), a ring[p] outside [0, E), a ring_row outside [0, n_rings), an edge
 * count L outside [1, E], a first or a rank outside [0, L), a ring_base outside [0, E] (tested before anything is added to it) or a
 * position outside [0, E) -- the edge writes none of its words; an unset side bit at the twin or a twin index outside [0, E) --
 * twin[p] = -1, the other words are written.
 * Refused without touching the device: a null pointer (with E > 0; ids, sides, offsets and stats always); sizes and K as above; E or
 * n_rings outside [0, 4 h w].  E == 0 launches nothing. */
int snerf_arcs_mark(const int* ids, const unsigned char* sides, const int* offsets, const int* slot, const int* flags, const int* ring,
                    const int* rank, const int* totals, const int* node, const int* first, const int* ring_row, const long long* ring_base,
                    int h, int w, long long K, long long E, long long n_rings, int* left, int* twin, int* pos_of, int* order, int* hf,
                    int* vf, unsigned long long* stats, void* stream);

/* snerf_arcs_fold: the arcs' vertices and the per-arc reductions, one launch, one thread per POSITION: the lanes of a wave share arcs.
 *   ids (h, w) int32;  key (h, w) int32 or NULL: the key plane (words 7 to 9 stay 0 without it);
 *   slot, ring, left, twin, pos_of, node (E) int32 by edge;  ring_row (E) int32 as above;
 *   order, hf, vf (E) int32 by position;  arc_of (E) int32: the arc of every position (the inclusive cumulative sum of hf, minus 1);
 *   ordinal (E) int32: the number of vf positions of the same arc in front of the position;
 *   last (E) int32: 1 where the position is the last of an OPEN arc;
 *   vertex_offset (A) int64: the first vertex of arc a -- the exclusive cumulative sum of the arcs' vertex counts;
 *   vertices (V, 2) int32: a vf position writes the tail (x, y) of its edge to vertices[vertex_offset[a] + ordinal[pos]], a `last`
 *     position also the head of its edge to vertices[vertex_offset[a] + ordinal[pos] + vf[pos]]; nothing else is written;
 *   rows (A, 12) u64, INITIALISED by the caller to 0 and only accumulated:
 *     word  content
 *      0    edges
 *      1    the sum of vf
 *      2    the id on the right (an atomic max; a negative id as 0)
 *      3    the id on the left (max)
 *      4    the ring's row + 1 (max)
 *      5    1 + the arc of pos_of[twin], from the arc's first edge only (max); 0 = no twin
 *      6    the sum over the edges of 1 + the arc of pos_of[twin] (0 for an edge without a twin)
 *      7    the edges whose own cell and whose cell across (inside the raster, whatever its id) both have valid keys
 *      8    the sum of (key of the own cell + 2^31) over the edges of word 7
 *      9    the sum of (key of the cell across + 2^31) over the edges of word 7
 *     10    1 when the arc's first edge is a break: the arc is open (max)
 *     11    0
 *   stats[2] u64, zeroed by the caller:  [0] guard trips,  [1] vertices written.
 * The lanes of a wave that share an arc reduce inside the wave, and the wave holds the result while its next positions belong to the
 * same arc, as snerf_outline_emit does for rings: the words are integer sums and maxima, so the grouping does not show in them.
 * Guards, each adding 1 to stats[0]: an order[pos] outside [0, E), a slot outside [0, 4 h w) or an arc_of outside [0, A) -- the
 * position writes and folds nothing; a ring[p] outside [0, E) or a ring_row outside [0, n_rings) -- word 4 gets nothing; a twin below
 * -1 or beyond E - 1, a pos_of[twin] outside [0, E) or its arc outside [0, A) -- words 5 and 6 get nothing; a vertex_offset[a]
 * outside [0, V] (tested before anything is added to it) or a vertex position outside [0, V), once per vertex -- that vertex is not
 * written, the position is still folded.
 * Refused without touching the device: a null pointer (with E > 0; ids and stats always; key may be null); sizes as above; E, A or
 * n_rings outside [0, 4 h w]; V outside [0, 8 h w] (an arc of one edge has two vertices).  E == 0 launches nothing. */
int snerf_arcs_fold(const int* ids, const int* key, const int* slot, const int* ring, const int* left, const int* twin, const int* pos_of,
                    const int* node, const int* ring_row, const int* order, const int* hf, const int* vf, const int* arc_of,
                    const int* ordinal, const int* last, const long long* vertex_offset, int h, int w, long long E, long long A,
                    long long n_rings, long long V, int* vertices, unsigned long long* rows, unsigned long long* stats, void* stream);

#ifdef __cplusplus
}
#endif
#endif
