/* Extension of the C-ABI of libsnerf_hip.so: a 3-D segment against the prism height field of a DSM -- where a ray of a view meets
 * the surface.  A map-to-view primitive of this project (the reference has no counterpart); DESIGN.md section 5v, restated in numpy
 * by tests/raycast_numpy.py.
 *
 * include/snerf_hip.h is the ABI-6 surface and its list of entry points is frozen; an entry added at the same ABI version is
 * declared in a header of its own (as include/snerf_orthorect.h), which includes it for the error codes and SnerfDsmGrid.  Same
 * conventions: plain pointers + sizes, device pointers unless stated, `stream` is a hipStream_t, 0 = SNERF_OK, a message for every
 * other return through snerf_last_error().  snerf_version() stays 6.
 * The Python binding is this header's group of rows in _lib.HEADER_SIGNATURES (tests/test_raycast_cpu.py compares it with this file). */
#ifndef SNERF_RAYCAST_H
#define SNERF_RAYCAST_H

#include "snerf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* snerf_dsm_segment_hit: one thread per segment walks the cells of the window the segment crosses (Amanatides-Woo) and reports
 * the first contact with the height field, each cell being a prism of its own height.  Every operation is fp64 with one rounding
 * each (no contraction); only + - * /, floor, comparisons and integer work.
 *   p0, p1 (n, 3) fp64: the end points (east, north, alt) of the segments, in the lattice's frame.
 *   grid: the lattice and the window (SnerfDsmGrid); dsm (out_h, out_w) fp32: the altitude of every cell of the window, row 0 = the
 *     north edge, NaN = a hole; bias (metres) is added to every cell's height.
 *   s_out (n) fp64: the parameter s in [0, 1] of the first contact on p0 + s (p1 - p0), NaN when there is none.
 *   state_out (n) u8: SNERF_HIT_*.  cell_out (n) int32 or NULL: the contact cell  j * out_w + i  of the window, -1 without a contact.
 * Every output is written for every segment.  Per segment, with W = out_w and H = out_h as doubles:
 *   1. an end point with a coordinate that is not finite: BAD (s NaN, cell -1), nothing is read;
 *   2. window cell coordinates of both ends, x = (east - xoff) / res - ioff, y = (yoff - north) / res - joff; dx = x1 - x0,
 *      dy = y1 - y0, da = a1 - a0; the altitude on the segment is a(s) = a0 + da * s (two roundings);
 *   3. entry.  With 0 <= x0 < W and 0 <= y0 < H the walk starts at s_in = 0 in the cell (floor x0, floor y0).  Otherwise the
 *      segment is clipped against [0, W] x [0, H] by slabs: t0 = 0, t1 = 1; for x, then for y: a zero delta with the coordinate
 *      outside [0, size) is OUTSIDE, a zero delta inside leaves t0, t1 alone, else ta = (0 - c0) / dc, tb = (size - c0) / dc,
 *      lo = min(ta, tb), hi = max(ta, tb), t0 = lo where lo > t0, t1 = hi where hi < t1.  t0 > t1: OUTSIDE.  Else s_in = t0 and
 *      the entry cell is (floor(x0 + dx * t0), floor(y0 + dy * t0)), each clamped into [0, size - 1]: the slabs put the clipped
 *      point into the closed rectangle, and rounding (or an entry through the far edge) may leave a coordinate at or just beyond
 *      an edge;
 *   4. walk, from s_a = s_in, at most out_w + out_h + 2 cells.  The crossing parameter of the cell's next boundary is recomputed
 *      from the boundary's integer coordinate, s_x = ((i + (dx > 0 ? 1 : 0)) - x0) / dx, +inf when dx == 0, and s_y likewise:
 *      nothing is accumulated.  x steps when s_x <= s_y, else y.  The cell is crossed over [s_a, s_b], s_b = min(s_x, s_y, 1), and
 *      not below s_a (the entry cell's boundary may round to just before s_in).  With h = (double)dsm[j][i] + bias:
 *        a(s_a) <= h: contact at s_a; START in the first cell of the walk (the segment begins at or under the surface), WALL after;
 *        else a(s_b) <= h: TOP, s = (h - a0) / da clamped to [s_a, s_b] (da != 0 here);
 *        else min(s_x, s_y) >= 1: END; else the step; a cell outside the window: OUTSIDE; else s_a = s_b and on.
 *      A NaN h fails both comparisons and never blocks; neither does -inf; +inf is a wall.  A vertical segment (dx == dy == 0)
 *      stays in its cell.  A walk that used up its cells (it cannot: it is monotone) is OUTSIDE.
 * Refused without touching the device: a null p0, p1, grid, dsm, s_out or state_out; n outside [0, 2^31] (n == 0 launches
 * nothing); a grid without res > 0 and positive sizes, a window beyond int32 cell indices or of 2^31 cells or more; a bias that is
 * not finite. */
#define SNERF_HIT_TOP 0
#define SNERF_HIT_WALL 1
#define SNERF_HIT_START 2
#define SNERF_HIT_END 3
#define SNERF_HIT_OUTSIDE 4
#define SNERF_HIT_BAD 5
int snerf_dsm_segment_hit(const double* p0, const double* p1, long long n, const SnerfDsmGrid* grid, const float* dsm,
                          double bias, double* s_out, unsigned char* state_out, int* cell_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
