/* Extension of the C-ABI of libsnerf_hip.so: roof planes on the map -- per-cell surface gradients and orientation codes from a
 * least-squares plane over each cell's neighbours of the same building, facets as the connected components of equal codes, per-facet
 * moment sums for a plane fit, and every facet cell's distance from its facet's plane.  A map product of this project (the reference
 * has no counterpart); DESIGN.md section 5z, restated in numpy by tests/roofs_numpy.py.
 *
 * include/snerf_hip.h is the ABI-6 surface and its list of entry points is frozen; an entry added at the same ABI version is
 * declared in a header of its own (as include/snerf_terrain.h), which includes it for the error codes and the limits.  Same
 * conventions: plain pointers + sizes, device pointers unless stated, `stream` is a hipStream_t, 0 = SNERF_OK, a message for every
 * other return through snerf_last_error(); no entry allocates or synchronises with the host, and none launches anything for an
 * empty problem.  snerf_version() stays 6.
 * The Python binding is this header's group of rows in _lib.HEADER_SIGNATURES (tests/test_roofs_cpu.py compares it with this file).
 *
 * A raster is (h, w), row 0 the north edge, cell c = j * w + i (row j, column i); here h and w are at most SNERF_ROOFS_MAX_SIDE
 * (8192), which the sum bounds below rely on.  `key` is the int32 plane of snerf_terrain_keys (include/snerf_terrain.h):
 * k = rint((alt - z0) / q), valid in the open range (-2^31, 2^31 - 1); SNERF_TERRAIN_HOLE and 2^31 - 1 are holes.  `ids` is an
 * object-id plane as the objects of include/snerf_objects.h are numbered: 0 = background, n in [1, K] = object n; an id outside
 * [0, K] is read as 0.  K < SNERF_ROOFS_MAX_OBJECTS = 2^27, so that ids * 16 + code fits an int32.
 * Every kernel loop is counted by h, w, the radius or a fixed bound; nothing terminates on memory content except the union-find walk
 * of snerf_roofs_link, which keeps the guards of csrc/objects_walk.h.  `stats` words are zeroed by the caller and only added to.
 * All sums are integers on integer atomics, and the fp64 arithmetic behind every float is fixed operation by operation (none
 * contracted): no word depends on launch order, on the grid shape or on how a raster is cut into row bands. */
#ifndef SNERF_ROOFS_H
#define SNERF_ROOFS_H

#include "snerf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SNERF_ROOFS_MAX_RADIUS 4
#define SNERF_ROOFS_MAX_SIDE 8192
#define SNERF_ROOFS_MAX_OBJECTS 134217728
#define SNERF_ROOFS_MOMENT_WORDS 16
#define SNERF_ROOFS_RESIDUAL_WORDS 8
/* the orientation codes; 1..8 are the downslope octants N, NE, E, SE, S, SW, W, NW */
#define SNERF_ROOFS_FLAT 0
#define SNERF_ROOFS_STEEP 9
#define SNERF_ROOFS_HOLE 253
#define SNERF_ROOFS_DEGENERATE 254
#define SNERF_ROOFS_NONE 255

/* snerf_roofs_normals: per-cell surface gradient and orientation code, one launch.
 *   key, ids (h, w) int32;  radius in [1, SNERF_ROOFS_MAX_RADIUS];  q: metres per key step, res: metres per cell;
 *   (cos0, sin0): the rotation of the octant bins (aspect0), applied for the code only;
 *   tan2_flat <= tan2_wall: the squared slopes at and below which a cell is flat, above which it is steep.
 * For a cell c = (j, i) with ids[c] in [1, K] and a valid key, the support is the cells g = (j + dj, i + di), |di|, |dj| <= radius,
 * inside the raster, with ids[g] == ids[c] and a valid key (c itself among them).  With d = (long long)key[g] - key[c], in int64:
 *     n = sum 1, Sx = sum di, Sy = sum dj, Sxx = sum di^2, Sxy = sum di dj, Syy = sum dj^2, Sd = sum d, Sxd = sum di d, Syd = sum dj d
 * and the cofactors of the normal matrix [[n, Sx, Sy], [Sx, Sxx, Sxy], [Sy, Sxy, Syy]], its determinant and Cramer's numerators:
 *     C00 = Sxx Syy - Sxy^2     C01 = Sxy Sy - Sx Syy     C02 = Sx Sxy - Sxx Sy
 *     C11 = n Syy - Sy^2        C12 = Sx Sy - n Sxy       C22 = n Sxx - Sx^2
 *     D = n C00 + Sx C01 + Sy C02     Nx = C01 Sd + C11 Sxd + C12 Syd     Ny = C02 Sd + C12 Sxd + C22 Syd
 * Bounds at radius <= 4: n <= 81; sum |di| <= 9 * 20 = 180, so |Sx|, |Sy| <= 180; Sxx, Syy <= 9 * 60 = 540; |Sxy| <= 20^2 = 400;
 * hence |C00| <= 540^2 + 400^2 < 2^19, |C01|, |C02| <= 400 * 180 + 180 * 540 < 2^18, |C11|, |C22| <= 81 * 540 < 2^16,
 * |C12| <= 180^2 + 81 * 400 < 2^16: every cofactor lies below 2^20.  |d| < 2^32, so |Sd| < 81 * 2^32 < 2^39 and
 * |Sxd|, |Syd| < 180 * 2^32 < 2^40; a numerator is three products below 2^18 * 2^39, 2^16 * 2^40 and 2^16 * 2^40: below 2^58 < 2^60.
 * D is the Gram determinant of the columns (1, di, dj): 0 <= D <= n Sxx Syy <= 81 * 540^2 < 2^25 < 2^29.
 * D <= 0 (a single cell or a collinear support): code = SNERF_ROOFS_DEGENERATE, NaN gradients.  Otherwise, in fp64, one IEEE
 * operation at a time in this order:
 *     f = q / res;   a = ((double)Nx / (double)D) * f;   b = ((double)Ny / (double)D) * f;      (a: rise per metre east, b: south)
 *     ar = (a * cos0) + (b * sin0);   br = (b * cos0) - (a * sin0);   s2 = (ar * ar) + (br * br);   t = fabs(ar) + fabs(br);
 *     code = 0 if s2 <= tan2_flat;  else 9 if s2 > tan2_wall;
 *            else if (t * t) < 2.0 * (ar * ar): 7 (W) if ar > 0.0 else 3 (E);       (the surface falls against its gradient)
 *            else if (t * t) < 2.0 * (br * br): 1 (N) if br > 0.0 else 5 (S);       (row 0 is north: a rise to the south falls north)
 *            else: 8 (NW) if ar > 0.0 and br > 0.0;  6 (SW) if ar > 0.0;  2 (NE) if br > 0.0;  else 4 (SE).
 * A surface whose keys are an exact integer plane alpha i + beta j + gamma gives Nx = alpha D and Ny = beta D exactly, whatever the
 * non-collinear support.
 *   slope_e, slope_n (h, w) f32, code (h, w) u8, tag (h, w) int32: EVERY word is written:
 *     slope_e = (float)a, slope_n = (float)(-b) (unrotated); NaN on every cell without a normal;
 *     code as above; SNERF_ROOFS_HOLE on an object cell with a hole key; SNERF_ROOFS_NONE off objects;
 *     tag = ids * 16 + code for the codes 0..8, else -1;
 *   stats[4] u64:  [0] object cells,  [1] cells with a normal (codes 0..9),  [2] degenerate cells,  [3] object cells with a hole key.
 * One thread per cell, consecutive lanes on consecutive columns; a workgroup stages the keys and ids of its 64 x 8 tile and its halo
 * of `radius` cells in LDS once, and the window is read from there; the sums stay in registers; the counts are reduced in the
 * workgroup before one lane adds them.
 * Refused without touching the device: a null key, ids, slope_e, slope_n, code, tag or stats; h or w outside [1, 8192]; K outside
 * [0, 2^27); radius outside [1, 4]; q or res not positive and finite; cos0 or sin0 not finite; tan2_flat or tan2_wall not finite,
 * tan2_flat < 0 or tan2_flat > tan2_wall. */
int snerf_roofs_normals(const int* key, const int* ids, int h, int w, long long K, int radius, double q, double res, double cos0,
                        double sin0, double tan2_flat, double tan2_wall, float* slope_e, float* slope_n, unsigned char* code, int* tag,
                        unsigned long long* stats, void* stream);

/* snerf_roofs_link: facets = the connected components of equal non-negative tags; snerf_objects_link (include/snerf_objects.h) with
 * "same class" replaced by "same tag", by the same three launches (init, merge by atomicMin, flatten) over the same walk and guards.
 *   tag (h, w) int32;  connectivity: 4 or 8;
 *   parent (h * w) int32: EVERY word is written: -1 where tag < 0, else the smallest linear index of the cell's component;
 *   stats[2] u64:  [0] guard trips,  [1] member cells.
 * Refused without touching the device: a null tag, parent or stats; sizes as above; a connectivity other than 4 or 8. */
int snerf_roofs_link(const int* tag, int h, int w, int connectivity, int* parent, unsigned long long* stats, void* stream);

/* snerf_roofs_moments: per-facet moment sums over the cells of the rows [row0, row1), one launch.
 *   fids (h, w) int32 in [0, F]: 0 = no facet, n = facet n;  root (h, w) int32: the `parent` plane of snerf_roofs_link;
 *   key, tag (h, w) int32: the planes the facets came from;
 *   rows (F, 16) u64, INITIALISED by the caller to the pattern below and only accumulated: bands that partition [0, h), accumulated
 *     into one `rows` in any order, give the words of one call over [0, h).
 * Coordinates are relative to the facet's own root cell (j0, i0) = (root / w, root % w) and its key k0 = key[root]:
 *     di = i - i0, dj = j - j0, dk = (long long)key[c] - k0.
 * A cell with |dk| >= 2^24 (256 m off its root at q = 2^-16 m), or whose key or whose root's key is a hole, is left out and counted.
 *   word  content                                                         init
 *    0    n: the cells folded                                             0
 *    1..3 sum di, sum dj, sum dk                                          0
 *    4..6 sum di^2, sum di dj, sum dj^2                                   0
 *    7, 8 sum di dk, sum dj dk                                            0
 *    9,10 min i, max i over the cells folded                              2^64 - 1, 0
 *   11,12 min j, max j over the cells folded                              2^64 - 1, 0
 *   13    the facet's tag (an atomic max; the cells agree)                0
 *   14    the root's linear index (an atomic max; the cells agree)        0
 *   15    cells left out                                                  0
 * Row n - 1 belongs to facet n.  Signed sums are two's complement in the u64.  A facet has at most 2^26 cells, |di|, |dj| < 2^13 and
 * |dk| < 2^24, so |sum dk| < 2^50, the second moments of position stay below 2^52 and |sum di dk| < 2^26 * 2^13 * 2^24 = 2^63: no
 * sum leaves 63 bits.  The lanes of a wave that share a facet are folded inside the wave before one lane issues the atomics.
 *   stats[3] u64:  [0] cells folded,  [1] cells left out,  [2] cells whose fid lies outside [0, F], or with a fid > 0 and a root
 *     outside [0, h * w) (ignored: they add to no row).
 * Refused without touching the device: a null fids, root, key, tag, rows (with F > 0) or stats; sizes as above; F outside [0, 2^27);
 * row0 < 0, row1 > h or row0 > row1.  F == 0 or row0 == row1 launches nothing. */
int snerf_roofs_moments(const int* fids, const int* root, const int* key, const int* tag, int h, int w, long long F, int row0, int row1,
                        unsigned long long* rows, unsigned long long* stats, void* stream);

/* snerf_roofs_residuals: the distance of every facet cell of the rows [row0, row1) from its facet's plane, one launch.
 *   fids, root, key: as snerf_roofs_moments;  planes (F, 3) f64 on the device: row n - 1 = (gamma, alpha, beta) predicts dk of facet n
 *   in key units; a row with a non-finite word means no plane;  q: metres per key step;  unit: key units per residual step.
 * With di, dj, dk as above, in fp64, one IEEE operation at a time in this order:
 *     pred = (gamma + (alpha * (double)di)) + (beta * (double)dj);   e = (double)dk - pred;   residual = (float)(q * e);
 *     t = rint(e / unit);   rq = 2^18 if !(t < 262144.0), -2^18 if t < -262144.0 (both count as clamped), else (long long)t.
 *   residual (h, w) f32: EVERY word of the rows [row0, row1) is written: NaN off facets, on a facet without a plane, on a cell whose
 *     fid or root is out of range and where the cell's key or its root's key is a hole;
 *   rows (F, 8) u64, INITIALISED by the caller and only accumulated, over the cells that got a residual:
 *   word  content                                                         init
 *    0    n                                                               0
 *    1    sum |rq|                                                        0
 *    2    sum rq^2                                                        0
 *    3    max |rq|                                                        0
 *    4, 5 min, max of key + 2^31 (the eave and the ridge)                 2^64 - 1, 0
 *    6    clamped cells                                                   0
 *    7    0                                                               0
 *   |rq| <= 2^18 and at most 2^26 cells: sum rq^2 <= 2^62.
 *   stats[3] u64:  [0] cells with a residual,  [1] facet cells without one (no plane, or a hole key),  [2] cells whose fid or root is
 *     out of range, as snerf_roofs_moments counts them.
 * Refused without touching the device: a null fids, root, key, residual, stats, or planes or rows with F > 0; sizes, F and the band
 * as snerf_roofs_moments; q or unit not positive and finite.  row0 == row1 launches nothing; F == 0 still writes the NaNs. */
int snerf_roofs_residuals(const int* fids, const int* root, const int* key, int h, int w, long long F, const double* planes, double q,
                          double unit, int row0, int row1, float* residual, unsigned long long* rows, unsigned long long* stats,
                          void* stream);

#ifdef __cplusplus
}
#endif
#endif
