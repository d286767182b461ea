/* Extension of the C-ABI of libsnerf_hip.so: per-cell altitude quantiles over all views -- the median surface on the map and the
 * spread of the views' altitudes.  A map product of this project (the reference has no counterpart); DESIGN.md section 5w, restated
 * in numpy by tests/fuse_numpy.py.
 *
 * include/snerf_hip.h is the ABI-6 surface and its list of entry points is frozen; an entry added at the same ABI version is
 * declared in a header of its own (as include/snerf_orthorect.h and include/snerf_raycast.h), which includes it for the error codes,
 * SnerfDsmGrid and the limits.  Same conventions: plain pointers + sizes, device pointers unless stated, `stream` is a hipStream_t,
 * 0 = SNERF_OK, a message for every other return through snerf_last_error(); no entry allocates or synchronises with the host, and
 * none launches anything for n == 0.  snerf_version() stays 6.
 * The Python binding is this header's group of rows in _lib.HEADER_SIGNATURES (tests/test_fuse_cpu.py compares it with this file).
 *
 * An order statistic cannot be folded with one atomic per cell: it needs the cell's list.  Three entries build the lists and read
 * them: count the offers per cell, (the caller's exclusive prefix sums turn the counts into the segments of one key buffer,)
 * scatter the keys into the segments, select exact ranks inside each segment.  Everything is integer arithmetic on integer atomics:
 * the words do not depend on launch order, on how a cloud is cut into calls or on the order of the clouds.
 *
 * The key and the cells are snerf_ortho_top's, bit for bit (include/snerf_hip.h, the ortho section): point p of a call offers
 *   key = (u64)(k + 2^31) << 32 | (0xFFFFFFFF - (index0 + p)),  k = llrint((z - z0) / q) in [-2^31, 2^31),
 * to every cell of its (2 radius + 1)^2 window that lies in the lattice extent and in the output window (cell c = jj * out_w + ii,
 * row 0 = the north edge).  A point whose k is not finite or out of range offers nothing and is counted in stats[0]; a point whose
 * window is empty offers nothing.  Keys are unique within a cell; ascending u64 order is ascending altitude and, at equal k,
 * descending point index; no valid key is 0.
 *
 * stats[4] (u64, zeroed by the caller, shared by the three entries; each adds):
 *   [0] points that offer nothing because of their altitude (snerf_fuse_count and snerf_fuse_scatter each count their own walk);
 *   [1] points that reached at least one cell (likewise);  [2] offers snerf_fuse_scatter could not store;
 *   [3] cells snerf_fuse_select refused to read. */
#ifndef SNERF_FUSE_H
#define SNERF_FUSE_H

#include "snerf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SNERF_FUSE_MAX_QUANTILES 8

/* snerf_fuse_count: one thread per point (grid-stride).  count (cells) u32, ZEROED by the caller before the first call and
 * accumulated over calls: count[c] += 1 for every cell c a valid point offers itself to (it wraps beyond 2^32 - 1 offers).
 *   xyz (n, 3) fp64 (east, north, alt); grid: the lattice and the window; radius in [0, SNERF_ORTHO_MAX_RADIUS].
 * Refused without touching the device: a null grid, count or stats, a null xyz with n > 0; n outside [0, 2^31]; radius outside
 * [0, 7]; a grid without res > 0 and positive sizes; a window beyond int32 cell indices; q not positive and finite, z0 not finite. */
int snerf_fuse_count(const double* xyz, long long n, const SnerfDsmGrid* grid, int radius, double z0, double q, unsigned* count,
                     unsigned long long* stats, void* stream);

/* snerf_fuse_scatter: the same walk; every offer takes a slot of its cell's segment and stores its key there.
 *   offsets (cells + 1) int64: the exclusive prefix sums of count (offsets[0] = 0, offsets[cells] = the total of the offers);
 *   capacity: the number of u64 words `keys` holds;  cursor (cells) u32, ZEROED before the first call and carried across calls.
 * Per offer to cell c:  t = atomicAdd(&cursor[c], 1) (always),  slot = offsets[c] + t;  the key is stored at keys[slot] only when
 *   0 <= offsets[c] <= slot < offsets[c + 1]  and  slot < capacity
 * (evaluated without overflow).  Otherwise stats[2] += 1 and nothing is written: a cloud that differs between the count walk and the
 * scatter walk, or a garbage offsets table, ends in a count, never in a write outside keys[0, capacity).  The order of the keys inside
 * a segment depends on arrival; the set does not.
 * Refused without touching the device: as snerf_fuse_count, and a null offsets, cursor or keys; index0 < 0 or
 * index0 + n > 2^32 - 1; capacity < 0. */
int snerf_fuse_scatter(const double* xyz, long long n, long long index0, const SnerfDsmGrid* grid, int radius, double z0, double q,
                       const long long* offsets, long long capacity, unsigned* cursor, unsigned long long* keys,
                       unsigned long long* stats, void* stream);

/* snerf_fuse_select: exact order statistics of every cell's segment; one wave64 owns a cell.
 *   quantiles_host (n_quantiles, 2) int: a HOST array of (num, den), 0 <= num <= den, 1 <= den <= 65536; it goes to the kernel by
 *   value.  words (n_quantiles, cells) u64: EVERY word of every cell is written.
 * Per cell c, with lo = offsets[c], hi = offsets[c + 1], m = hi - lo:
 *   m == 0: every word is 0, nothing is read or counted (offers the scatter walk made to such a cell stand in stats[2]);
 *   m < 0, lo < 0, hi > capacity, or cursor[c] != m (compared as 64-bit integers, so an m beyond 2^32 - 1 fails): every word is 0,
 *     stats[3] += 1, and no key of that cell is read;
 *   else, per quantile k:  r_k = ((m - 1) * num_k) / den_k  in 64-bit integer arithmetic (numpy's method="lower"), and
 *     words[k][c] = the r_k-th smallest key (0-based) of keys[lo, hi).
 * (0, 1) is the lowest point of a cell, (1, 1) the highest -- snerf_ortho_top's word --, (1, 2) the LOWER median: an actual point,
 * whose index exists for snerf_ortho_gather, which reads a plane of words as it reads `top`.
 * The selection reads the keys and never moves them: m <= 64 ranks one key per lane by counting; longer segments take an MSB-first
 * radix select, 8 passes of 8 bits, O(m) per pass for all quantiles together, exact for any m up to 2^32 - 1 (and for equal keys,
 * should a caller's buffer hold any: the result is the r_k-th word of the sorted segment).
 * Refused without touching the device: a null keys, offsets, cursor, quantiles_host, words or stats; capacity < 0; cells outside
 * [1, 2^31); n_quantiles outside [1, SNERF_FUSE_MAX_QUANTILES]; a (num, den) outside the ranges above. */
int snerf_fuse_select(const unsigned long long* keys, const long long* offsets, long long capacity, const unsigned* cursor,
                      long long cells, const int* quantiles_host, int n_quantiles, unsigned long long* words,
                      unsigned long long* stats, void* stream);

#ifdef __cplusplus
}
#endif
#endif
