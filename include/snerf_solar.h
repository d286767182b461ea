/* Extension of the C-ABI of libsnerf_hip.so: solar potential on the map -- horizon planes of a height field (one march per cell and
 * azimuth sector, the steepest slope seen), the sky-view factor from those planes, and the direct irradiation and lit counts of a
 * table of suns tested against them.  A map product of this project (the reference has no counterpart); DESIGN.md section 5zb,
 * restated in numpy by tests/solar_numpy.py.
 *
 * include/snerf_hip.h is the ABI-6 surface and its list of entry points is frozen; an entry added at the same ABI version is
 * declared in a header of its own (as include/snerf_roofs.h), which includes it for the error codes.  Same conventions: plain
 * pointers + sizes, device pointers unless stated, `stream` is a hipStream_t, 0 = SNERF_OK, a message for every other return through
 * snerf_last_error(); no entry allocates, copies or synchronises with the host.  snerf_version() stays 6.
 * The Python binding is this header's group of rows in _lib.HEADER_SIGNATURES (tests/test_solar_cpu.py compares it with this file).
 *
 * A raster is (h, w), row 0 the north edge, cell c = j * w + i (row j, column i), h * w < 2^31.  The kernels do fp64 + - * /,
 * comparisons and integer work only, one IEEE operation at a time (none contracted): the host evaluates every transcendental and no
 * word depends on the launch order or the grid shape. */
#ifndef SNERF_SOLAR_H
#define SNERF_SOLAR_H

#include "snerf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SNERF_SOLAR_MAX_DIRS 64
#define SNERF_SOLAR_MAX_SECTORS 720
#define SNERF_SOLAR_MAX_SUNS 64

/* snerf_solar_horizon: per cell and direction the steepest slope from the cell to any cell its ground track crosses, one launch.
 *   dsm (h, w) f32: altitudes, NaN = a hole;
 *   dirs_host (n_dirs, 2) f64 in HOST memory, read before the launch and passed by value: (ux, uy), the unit step in (column, row)
 *     per cell of horizontal travel (azimuth a clockwise from north: ux = sin a, uy = -cos a); 1 <= n_dirs <= SNERF_SOLAR_MAX_DIRS;
 *   bias (metres) is added to the start altitude; max_dist (cells) > 0 bounds the march, +inf = no bound;
 *   horizon_out (n_dirs, h, w) f32: EVERY word is written.
 * The march is the walk of snerf_shadow_cast (include/snerf_hip.h) from the cell's centre: stepx = ux > 0 ? 1 : -1 (stepy alike),
 * tDeltaX = 1 / |ux| (inf for ux == 0), tMaxX = 0.5 tDeltaX; per step, if tMaxX <= tMaxY: t = tMaxX, i += stepx, tMaxX += tDeltaX,
 * else the same in y (on a tie x steps first); at most h + w + 2 steps.  With h0 = (double)dsm[cell] + bias and best = -inf, after
 * each step:  (a) (i, j) outside the raster: the march ends;  (b) t > max_dist: the march ends;
 *             (c) sl = ((double)dsm[j][i] - h0) / t;  if sl > best: best = sl   (false for a NaN cell).
 * horizon_out = (float)best: metres of rise per cell of horizontal travel, -inf when nothing was tested, NaN where the start cell is
 * NaN.  A sun at that azimuth with rise >= horizon_out is visible from the cell.
 * z_top is only an early exit: a march may end once no altitude <= z_top can raise best; any z_top at or above the largest finite
 * altitude (+inf included) gives the same bits.  The altitudes are finite or NaN.
 * One workgroup per tile of 64 x 4 cells under one direction: the direction is wave-uniform, a wave is 64 neighbouring cells of a row.
 * Refused without touching the device: a null dsm, dirs_host or horizon_out; h or w < 1 or h * w >= 2^31; n_dirs outside [1, 64];
 * a row that is not finite or with ux^2 + uy^2 further than 1e-9 from 1; a bias that is not finite; max_dist NaN or <= 0; a NaN z_top. */
int snerf_solar_horizon(const float* dsm, int h, int w, const double* dirs_host, int n_dirs, double bias, double z_top, double max_dist,
                        float* horizon_out, void* stream);

/* snerf_solar_svf: the cosine-weighted sky-view factor of a horizontal surface, mean cos^2 of the horizon angle, one launch.
 *   horizon (n_dirs, h, w) f32 of snerf_solar_horizon, 1 <= n_dirs <= SNERF_SOLAR_MAX_SECTORS;  res > 0: metres per cell;
 *   svf_out (h, w) f32: EVERY word is written.
 * One thread per cell, in the order d = 0 .. n_dirs - 1 from acc = 0:
 *     T = (double)H[d] / res;   if !(T > 0.0): T = 0.0;   acc = acc + 1.0 / (1.0 + T * T);
 * svf = (float)(acc / (double)n_dirs); NaN on a cell whose H[0] is NaN.
 * Refused without touching the device: a null horizon or svf_out; sizes as above; n_dirs outside [1, 720]; res not positive and
 * finite. */
int snerf_solar_svf(const float* horizon, int n_dirs, int h, int w, double res, float* svf_out, void* stream);

/* snerf_solar_irradiate: a table of suns against the horizon planes, one launch.
 *   horizon (n_dirs, h, w) f32, 1 <= n_dirs <= SNERF_SOLAR_MAX_SECTORS;
 *   slope_e, slope_n (h, w) f32: the surface's rise per metre east and north (snerf_roofs_normals), both NULL (horizontal) or both set;
 *   suns_host (n_suns, 7) f64 in HOST memory, read before the launch and passed by value, 1 <= n_suns <= SNERF_SOLAR_MAX_SUNS:
 *     (sector, frac, rise, east, north, up, weight): the sun stands between the sectors `sector` and sector + 1 at the share frac,
 *     rise = tan(elevation) * res, (east, north, up) its unit vector, weight what it adds per unit of cos(incidence);
 *   direct_acc (h, w) f64, lit_count (h, w) u32: ACCUMULATORS the caller zeroes; calls on one stream add up in order.
 * Per cell, with gx = (double)slope_e, gy = (double)slope_n (0.0 without slopes) and a = direct_acc, in table order:
 *     Hk = frac == 0.0 ? (double)H[sector] : ((1.0 - frac) * (double)H[sector]) + (frac * (double)H[(sector + 1) % n_dirs]);
 *     lit = rise >= Hk;   c = (up - (gx * east)) - (gy * north);   a = a + ((lit && c > 0.0) ? c * weight : 0.0);   lit_count += lit;
 * direct_acc = a, or NaN if gx or gy is NaN.  A cell whose H[0] is NaN gets direct_acc = NaN and keeps its count.  The caller divides
 * by sqrt(1 + gx^2 + gy^2) for the irradiation per unit of surface.
 * Refused without touching the device: a null horizon, suns_host, direct_acc or lit_count; one slope without the other; sizes as
 * above; n_dirs outside [1, 720]; n_suns outside [1, 64]; a row that is not finite, with a sector that is not an integer of
 * [0, n_dirs), frac outside [0, 1), rise <= 0, east^2 + north^2 + up^2 further than 1e-9 from 1, up <= 0 or weight < 0. */
int snerf_solar_irradiate(const float* horizon, int n_dirs, int h, int w, const float* slope_e, const float* slope_n,
                          const double* suns_host, int n_suns, double* direct_acc, unsigned int* lit_count, void* stream);

#ifdef __cplusplus
}
#endif
#endif
