/* Extension of the C-ABI of libsnerf_hip.so: warping a raster from one map lattice onto another -- any resolution, any offset, the
 * two lattices north-up and axis-parallel.  What holds a lidar DSM at 1 m against a 0.5 m map, or two exports at different
 * resolutions against each other.  The reference does this implicitly through GDAL; parity with gdalwarp / Translate is UNPINNED
 * (neither GDAL nor rasterio is part of this build).  DESIGN.md section 5zd, restated in numpy by tests/warp_numpy.py.
 *
 * include/snerf_hip.h is the ABI-6 surface and its list of entry points is frozen; an entry added at the same ABI version is
 * declared in a header of its own (as include/snerf_terrain.h), which includes it for the error codes and the limits.  Same
 * conventions: plain pointers + sizes, device pointers unless stated, `stream` is a hipStream_t, 0 = SNERF_OK, a message for every
 * other return through snerf_last_error(); no entry allocates or synchronises with the host, and none launches anything for an
 * empty problem.  snerf_version() stays 6.
 * The Python binding is this header's group of rows in _lib.ADDED_HEADER_SIGNATURES (tests/test_warp_cpu.py compares it with this
 * file).
 *
 * GEOMETRY.  The entries work in index space and know no geography: a SnerfWarpMap places the destination lattice in the source's
 * cell coordinates.  Rasters are (h, w), row 0 the north edge.  On an axis, source cell k covers [k, k + 1); destination cell i covers
 * [a, b) with a = off + i * step, b = off + (i + 1) * step and the centre c = off + (i + 0.5) * step -- fp64, one multiplication then
 * one addition, never fused.  Columns use off_x / step_x (i grows east), rows off_y / step_y (j grows south).
 *
 * TAPS PER AXIS.
 *   NEAREST           the single tap floor(c), weight 1;
 *   BILINEAR          t = c - 0.5, k0 = floor(t), f = t - k0: the taps (k0, 1 - f) and (k0 + 1, f);
 *   AVERAGE, MIN, MAX k = floor(a) ... ceil(b) - 1, weight min(k + 1, b) - max(k, a).
 * A tap whose weight is not > 0 is skipped entirely (0 * inf never occurs; an integer shift reads exactly one cell).
 *
 * A DESTINATION CELL, per plane: rows are the outer loop (north to south), columns the inner one (west to east); for every pair of
 * taps w = wy * wx and tot += w; where the tap lies inside the source and its value is finite, num += w * v and den += w (num starts
 * from -0, the identity of the addition, so a single tap of weight 1 returns its value's bits, those of -0 included).  Taps outside
 * the source and values that are not finite (NaN, +-inf) are holes.  The result is (float)(num / den) when den > 0 and
 * den >= min_valid * tot, else NaN (0x7fc00000).  MIN / MAX apply the same coverage test and return the extreme valid value with its
 * input bits (a later tap replaces an earlier one only if strictly smaller / larger).  NEAREST returns the tap's bits or NaN and does
 * not read min_valid.  Plain IEEE fp64 in this order: the numpy restatement gives the same bits.
 *
 * LABELS are unsigned char; 255 (SNERF_ORTHO_NO_LABEL) is a hole.  NEAREST as above; a tap outside the source or a hole gives 255.
 * MODE: the members on an axis are the source cells whose centre lies in the destination cell, k = ceil(a - 0.5) ... ceil(b - 0.5) - 1,
 * and floor(c) alone when there is none.  The votes are integer counts over the members inside the source that are not 255; the
 * winner has the most votes, the lowest class on a tie, 255 without a vote.
 *
 * stats[3] u64 is zeroed by the caller and only added to (integer atomics):  [0] finite / labelled words written,  [1] holes
 * written,  [2] destination cells with at least one tap (member) outside the source, counted once per cell whatever the planes.
 * Every loop is counted by the map alone; nothing terminates on memory content; no result depends on the order of the launch. */
#ifndef SNERF_WARP_H
#define SNERF_WARP_H

#include "snerf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SNERF_WARP_NEAREST 0
#define SNERF_WARP_BILINEAR 1
#define SNERF_WARP_AVERAGE 2
#define SNERF_WARP_MIN 3
#define SNERF_WARP_MAX 4
#define SNERF_WARP_MODE 5
#define SNERF_WARP_MAX_STEP 64
#define SNERF_WARP_MAX_PLANES 16

typedef struct SnerfWarpMap {
  double off_x, step_x, off_y, step_y;
  int src_w, src_h, dst_w, dst_h;
} SnerfWarpMap;

/* What both entries refuse without touching the device: a null pointer; src == dst; any of the four sizes < 1, or h * w >= 2^31 on
 * either side; a step that is not finite and > 0; |off| + dst_extent * step >= 2^31 on an axis (every coordinate must convert to an
 * integer exactly); a method the entry does not take; a step above SNERF_WARP_MAX_STEP on either axis for AVERAGE, MIN, MAX and MODE
 * (at most 66 taps per axis). */

/* snerf_warp_planes: float planes, one launch.
 *   src (planes, src_h, src_w) f32;  dst (planes, dst_h, dst_w) f32: EVERY word is written;
 *   method: NEAREST, BILINEAR, AVERAGE, MIN or MAX;  min_valid in (0, 1]: the share of a cell's weight that must be valid.
 * One thread per destination cell, a wave along a row, a 64 x 4 tile per workgroup; the taps of a cell are computed once and serve
 * every plane.
 * Also refused: planes outside [1, SNERF_WARP_MAX_PLANES]; min_valid outside (0, 1] or NaN. */
int snerf_warp_planes(const float* src, int planes, const SnerfWarpMap* map, int method, double min_valid, float* dst,
                      unsigned long long* stats, void* stream);

/* snerf_warp_labels: one label plane, one launch.
 *   src (src_h, src_w) u8;  dst (dst_h, dst_w) u8: EVERY byte is written;  method: NEAREST or MODE.
 * NEAREST as the planes; MODE is one wave per destination cell: the lanes stride over the members and count them in a histogram of
 * 256 words in LDS (integer LDS atomics), then every lane scans four classes and a shuffle reduction finds the winner. */
int snerf_warp_labels(const unsigned char* src, const SnerfWarpMap* map, int method, unsigned char* dst, unsigned long long* stats,
                      void* stream);

#ifdef __cplusplus
}
#endif
#endif
