/* Extension of the C-ABI of libsnerf_hip.so: objects on the map -- the connected components of a class raster and per-object
 * reductions (area, footprint, roof altitude, the ground round the object, perimeter).  A map product of this project (the reference
 * has no counterpart); DESIGN.md section 5x, restated in numpy by tests/objects_numpy.py.
 *
 * include/snerf_hip.h is the ABI-6 surface and its list of entry points is frozen; an entry added at the same ABI version is
 * declared in a header of its own (as include/snerf_fuse.h), which includes it for the error codes and the limits.  Same
 * conventions: plain pointers + sizes, device pointers unless stated, `stream` is a hipStream_t, 0 = SNERF_OK, a message for every
 * other return through snerf_last_error(); no entry allocates or synchronises with the host, and none launches anything for an
 * empty problem.  snerf_version() stays 6.
 * The Python binding is this header's group of rows in _lib.HEADER_SIGNATURES (tests/test_objects_cpu.py compares it with this file).
 *
 * A raster is (h, w), row 0 the north edge, cell c = j * w + i (row j, column i); h * w < 2^31.  A class table is a HOST array of
 * 256 bytes, entry c non-zero = class c is in the set; it goes to the kernel by value.  Class 255 (SNERF_ORTHO_NO_LABEL) is in no
 * set: a table that names it is refused.
 * Everything is integer arithmetic on integer atomics: no word depends on launch order, on the grid shape or on how a raster is cut
 * into row bands. */
#ifndef SNERF_OBJECTS_H
#define SNERF_OBJECTS_H

#include "snerf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SNERF_OBJECTS_ROW_WORDS 16

/* snerf_objects_link: the connected components of the cells whose class takes part.
 *   label (h, w) u8;  member_host: the classes that take part;  connectivity: 4 or 8.
 *   parent (h * w) int32: EVERY word is written: -1 for a cell whose class takes no part, else the root of the cell's component =
 *     the smallest linear index among the component's cells.
 *   stats[2] u64, zeroed by the caller:  [0] guard trips (below; 0 unless `parent` was written by someone else during the call),
 *     [1] member cells.
 * Two member cells are linked when they are 4- (W, E, N, S) or 8-neighbours (also NW, NE, SW, SE) AND carry the same class: a
 * building beside a car is two objects even where both classes take part.
 * Three launches, no host round trip:  init  parent[c] = c for a member cell, else -1;  merge  every member cell unites with its W
 * and N neighbours (and NW, NE at connectivity 8) of its own class;  flatten  parent[c] = find(c).  The union is lock-free
 * (csrc/objects_walk.h):
 *   find(a):      while ((p = load(parent[a])) != a) a = p;
 *   unite(a, b):  for (;;) { a = find(a); b = find(b); if (a == b) break; if (a < b) swap(a, b);
 *                            old = atomicMin(&parent[a], b); if (old == a) break; a = old; }
 * A link only ever points to a lower index of the same component (init gives parent[c] = c, atomicMin only lowers), so every step of
 * both loops strictly lowers a non-negative integer, and the lowest cell of a component is never hooked under anything: the result
 * does not depend on the order of arrival.  The loops also ENFORCE it: a loaded parent that is negative, or not below its cell while
 * different from it, ends the walk, adds 1 to stats[0] and leaves the cell alone -- no input can turn a launch into a hang.
 * Refused without touching the device: a null label, member_host, parent or stats; h or w < 1; h * w >= 2^31; a connectivity other
 * than 4 or 8; member_host[255] != 0. */
int snerf_objects_link(const unsigned char* label, int h, int w, const unsigned char* member_host, int connectivity, int* parent,
                       unsigned long long* stats, void* stream);

/* snerf_objects_stats: per-object reductions over the cells of the rows [row0, row1) of a raster, one launch.
 *   ids (h, w) int32 in [0, K]: 0 = background, n = object n;  label (h, w) u8;  alt (h, w) f32 (NaN = a hole);
 *   ground_host: the classes that count as ground round an object;  ring in [0, SNERF_ORTHO_MAX_RADIUS];
 *   z0, q: the quantisation of the altitudes, k = rint((alt - z0) / q), valid in [-2^31, 2^31), as the lattice's keys quantise;
 *   [row0, row1): the band of rows whose cells are folded; neighbours and ring windows read the WHOLE raster, so bands that
 *     partition [0, h), accumulated into one `rows` in any order, give the words of one call over [0, h).
 *   rows (K, 16) u64, INITIALISED by the caller to the pattern below and only accumulated;
 *   stats[4] u64, zeroed by the caller:  [0] object cells whose altitude is finite but out of key range,  [1] object cells with a
 *     non-finite altitude,  [2] cells whose id lies outside [0, K] (ignored: they add to no row),  [3] ring pairs counted.
 * Row n - 1 belongs to object n.  Signed sums are two's complement in the u64; altitude minima / maxima are stored as k + 2^31.
 *   word  content                                                         init
 *    0    area (cells)                                                    0
 *    1, 2 sum of i, sum of j (column, row of the raster)                  0
 *    3, 4 min i, max i                                                    2^64 - 1, 0
 *    5, 6 min j, max j                                                    2^64 - 1, 0
 *    7    cells with a valid k                                            0
 *    8    sum of k over those                                             0
 *    9,10 min, max of k + 2^31 over those                                 2^64 - 1, 0
 *   11    ring pairs                                                      0
 *   12    sum of k over the ring pairs                                    0
 *   13    min of k + 2^31 over the ring pairs                             2^64 - 1
 *   14    perimeter: the 4-neighbour edges of the object's cells to a cell of another id or to the raster's edge     0
 *   15    the object's class (an atomic max; the cells of a component agree)                                        0
 * The ring: for every cell c of object n (c in the band), every cell g of c's (2 ring + 1)^2 window, clipped to the raster, counts
 * when ids[g] == 0, ground_host[label[g]] != 0 and alt[g] has a valid k; the pair (c, g) adds 1 to word 11 and k(g) to word 12 of
 * row n - 1 and folds k(g) + 2^31 into word 13.  A ground cell beside a long wall is counted once per object cell that sees it: the
 * ring mean is weighted toward the ground next to the footprint and needs no de-duplication.  ring = 0 counts nothing.  With
 * h * w * (2 ring + 1)^2 < 2^32 (anything else is refused) and |k| <= 2^31 no sum leaves 63 bits.
 * Refused without touching the device: a null ids, label, alt, ground_host, rows (with K > 0) or stats; sizes as snerf_objects_link;
 * K outside [0, 2^31); ring outside [0, SNERF_ORTHO_MAX_RADIUS]; the pair-count bound; row0 < 0, row1 > h or row0 > row1; q not
 * positive and finite, z0 not finite; ground_host[255] != 0.  K == 0 or row0 == row1 launches nothing. */
int snerf_objects_stats(const int* ids, const unsigned char* label, const float* alt, int h, int w, long long K,
                        const unsigned char* ground_host, int ring, double z0, double q, int row0, int row1,
                        unsigned long long* rows, unsigned long long* stats, void* stream);

#ifdef __cplusplus
}
#endif
#endif
