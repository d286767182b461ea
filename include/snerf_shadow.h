/*
 * snerf_shadow.h -- the cast-shadow entries of libsnerf_hip.so: the shadow a height field casts under a sun, and the agreement
 * of a learned shadow map with it.  A map product of this project (the reference has no counterpart); DESIGN.md section 5o.
 * The conventions, the error codes and snerf_last_error() are those of snerf_hip.h; the ABI version does not change.
 */
#ifndef SNERF_SHADOW_H
#define SNERF_SHADOW_H

#include "snerf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- cast shadows on the DSM lattice ------------------------------------------------------------------------------------------
 * snerf_shadow_cast: one thread per (cell, sun) marches from the cell towards the sun over the height field.
 *   dsm (h, w) fp32, device memory, row 0 = the north edge (as everywhere on the lattice), NaN = a hole.
 *   suns_host (n_suns, 3) fp64 in HOST memory, one row (ux, uy, rise) per sun: ux = sin(azimuth) (towards the sun, east = +column),
 *     uy = -cos(azimuth) (north = -row), rise = tan(elevation) * res, the metres a ray climbs per cell of horizontal travel.  The
 *     rows are checked and go to the kernel BY VALUE in its arguments: no device table, no copy, nothing read after the call
 *     returns.  1 <= n_suns <= SNERF_SHADOW_MAX_SUNS.
 *   bias (metres) is added to the start altitude; z_top (metres, may be +inf) ends a march early.
 *   lit_out (n_suns, h, w) u8: 0 = shadowed, 1 = lit, SNERF_SHADOW_UNKNOWN = the start cell is NaN.
 *   dist_out (n_suns, h, w) fp32 or NULL: the horizontal distance to the blocking cell in CELLS; NaN where lit or unknown.
 * The march is an Amanatides-Woo walk in cell units; every step fp64 with one rounding per operation (no contraction), only
 * + - * / and comparisons -- the host evaluates every transcendental -- so an fp64 restatement reproduces it bit for bit:
 *   start at (i + 0.5, j + 0.5) with h0 = (double)dsm[j][i] + bias;
 *   stepx = ux > 0 ? 1 : -1, tDeltaX = 1 / |ux| (+inf when ux == 0), tMaxX = 0.5 * tDeltaX; the same for y;
 *   each step: if tMaxX <= tMaxY then t = tMaxX, i += stepx, tMaxX += tDeltaX, else the y analogue -- ON A TIE X STEPS FIRST and
 *     the next step takes y at the same t;
 *   after each step the first of these that holds ends the march:
 *     a. (i, j) outside [0, w) x [0, h)                -> lit;
 *     b. hr = h0 + rise * t, hr > z_top                -> lit;
 *     c. (double)dsm[j][i] > hr                        -> shadowed, dist = (float)t (a NaN cell never blocks: the comparison is false).
 *   The start cell is never tested.  At most h + w + 2 steps occur.  z_top is only an early exit: with z_top >= the largest finite
 *   altitude the result is the one under +inf.
 * Refused without touching the device: null dsm / suns_host / lit_out, h or w < 1 or h * w >= 2^31, n_suns outside
 * [1, SNERF_SHADOW_MAX_SUNS], a sun row that is not finite, whose ux^2 + uy^2 is more than 1e-9 from 1, or with rise <= 0, a bias that
 * is not finite, a NaN z_top. */
#define SNERF_SHADOW_MAX_SUNS 64
#define SNERF_SHADOW_UNKNOWN 255
int snerf_shadow_cast(const float* dsm, int h, int w, const double* suns_host, int n_suns, double bias, double z_top,
                      unsigned char* lit_out, float* dist_out, void* stream);

/* snerf_shadow_agreement: n_suns learned shadow maps against n_suns cast masks in one launch.
 *   sun (n_suns, cells) fp32; lit (n_suns, cells) u8 (snerf_shadow_cast's lit_out); valid (cells) u8 or NULL (0 = leave the cell out);
 *   a cell is predicted lit when sun >= threshold.
 *   acc (n_suns, 8) u64, ZEROED by the caller, accumulated; the words of a sun's row:
 *     [0] += lit and predicted lit       [1] += lit and predicted shadow
 *     [2] += shadow and predicted lit    [3] += shadow and predicted shadow
 *     [4] += cells left out: lit == SNERF_SHADOW_UNKNOWN (or any value other than 0 / 1), valid == 0, or sun not finite
 *     [5] += llrint(sun * 2^24) over the counted lit cells, [6] the same over the counted shadow cells -- int64 sums in two's
 *            complement (the DSM rasteriser's quantised sums); the product is exact, ties round to even, and it is clamped to
 *            +-2^62 first (a shadow map lies in [0, 1]: the clamp only keeps the conversion defined)
 *     [7] reserved, not written.
 * Integer atomics only: the words do not depend on launch order, on how a map is cut into calls, or on ranks (a SUM all-reduce
 * combines them).
 * Refused without touching the device: null sun / lit / acc, cells < 1, n_suns outside [1, SNERF_SHADOW_MAX_SUNS], a threshold that
 * is not finite. */
int snerf_shadow_agreement(const float* sun, const unsigned char* lit, const unsigned char* valid, long long cells, int n_suns,
                           double threshold, unsigned long long* acc, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SNERF_SHADOW_H */
