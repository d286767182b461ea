/* Extension of the C-ABI of libsnerf_hip.so: orthorectification -- the scene's own images and labels on the DSM lattice.  A map
 * product of this project (the reference has no counterpart); DESIGN.md section 5t, restated in numpy by tests/orthorect_numpy.py.
 *
 * include/snerf_hip.h is the ABI-6 surface and its list of entry points is frozen (tests/test_embed_grad_cpu.py pins it symbol by
 * symbol, tests/test_gpu_fill.py classifies every pointer of it); an entry added at the same ABI version is declared in a header
 * of its own, which includes it for the error codes, SnerfDsmGrid, SnerfRpc and the limits.  Same conventions: plain pointers +
 * sizes, device pointers unless stated, `stream` is a hipStream_t, 0 = SNERF_OK, a message for every other return through
 * snerf_last_error().  snerf_version() stays 6.
 * The Python binding is this header's group of rows in _lib.HEADER_SIGNATURES (tests/test_orthorect_cpu.py compares it with this file). */
#ifndef SNERF_ORTHORECT_H
#define SNERF_ORTHORECT_H

#include "snerf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* snerf_orthorectify: one thread per cell of the output window (cells = out_h * out_w, row-major, row 0 = the north edge) walks
 * the images of the call; a cell's accumulators have one writer per launch, so nothing is atomic but the four totals.  Every
 * operation is fp64 with one rounding each (no contraction); the transcendentals are those of the world -> scene direction of
 * snerf_geo_points.
 *   dsm (cells) fp32: the altitude of every cell of the window, NaN or infinite = a hole.
 *   grid: the lattice and the window (SnerfDsmGrid); lon0 (radians), south: the UTM zone, as in SnerfGeoParams.
 *   images_host / images_dev: the same (n_images) table in host memory (checked) and in device memory (read by the kernel).
 *     Image k is w x h pixels, pixel (ci, ri) being row  row0 + ri * w + ci  of rgbs (n_rows, 3) fp32 and labels (n_rows) u8.
 *   labels / votes: both or neither.  visible (n_images, cells) u8 or NULL: snerf_shadow_cast's lit_out under the images' view rows.
 * Per cell c = jj * out_w + ii:
 *   1. i = ioff + ii, j = joff + jj, east = xoff + (i + 0.5) res, north = yoff - (j + 0.5) res, alt = (double)dsm[c];
 *   2. alt not finite: the state is HOLE for every image and (col, row) are NaN;
 *   3. else (lat, lon) = utm.to_latlon(east, north) once, and per image k:
 *   4. (col, row) = the RPC projection of (lon, lat, alt): integer (col, row) is a pixel's centre;
 *   5. ci = floor(col + 0.5), ri = floor(row + 0.5); unless 0 <= ci < w and 0 <= ri < h (compared in fp64: NaN and infinity
 *      fail) the state is OUTSIDE;
 *   6. else, visible given and visible[k][c] != 1: HIDDEN;
 *   7. else bilinear colour: c0 = floor(col), fx = col - c0, r0 = floor(row), fy = row - r0, the neighbours c0, c0 + 1 clamped to
 *      [0, w - 1] and r0, r0 + 1 to [0, h - 1]; per channel, the fp32 pixels widened, top = (1 - fx) p00 + fx p10,
 *      bot = (1 - fx) p01 + fx p11, v = (1 - fy) top + fy bot.  A v that is not finite in any channel: OUTSIDE.  Else SEEN:
 *      sum[ch * cells + c] += llrint(v * 2^24) (clamped to +-2^62 first, ties to even), count[c] += 1, and with labels,
 *      l = labels[row0 + ri * w + ci] < n_classes: votes[l * cells + c] += 1.
 * Accumulators (ZEROED by the caller before the first call; each call adds, so a split may be cut into calls of <= 64 images, in
 * any order): sum (3, cells) int64, count (cells) u32, votes (n_classes, cells) u32 in snerf_ortho_votes' layout.  The mosaic is
 * snerf_dsm_finish(count, sum + ch * cells, cells, 0, 2^-24, ...) per channel and snerf_ortho_votes_finish(votes, ...).
 * Per-image outputs, each may be NULL: col_row (n_images, 2, cells) fp64 (plane 0 col, plane 1 row); rgb_out (n_images, 3, cells)
 * fp32, NaN where not SEEN; label_out (n_images, cells) u8: the pixel's label where SEEN and labels given, else 255; state_out
 * (n_images, cells) u8.  stats[4] (u64, zeroed by the caller): [s] += the (image, cell) pairs of state s.
 * Refused without touching the device: a null dsm, grid, images_host, images_dev, rgbs, sum, count or stats; votes and labels given
 * by halves; a grid without res > 0 and positive sizes, a window beyond int32 cell indices or of 2^31 cells or more; n_images
 * outside [1, SNERF_RECT_MAX_IMAGES]; n_classes outside [1, 255] with labels; n_rows < 1; an image with w or h < 1, w * h
 * overflowing, row0 < 0 or row0 + w * h > n_rows, or a zero or non-finite RPC scale; lon0 outside [-pi, pi]; south other than 0 / 1. */
typedef struct SnerfRectImage {
  SnerfRpc rpc;
  long long row0;
  int w, h;
} SnerfRectImage;
#define SNERF_RECT_MAX_IMAGES 64   /* = SNERF_SHADOW_MAX_SUNS: one snerf_shadow_cast call makes one call's visibility planes */
#define SNERF_RECT_SEEN 0
#define SNERF_RECT_HOLE 1
#define SNERF_RECT_OUTSIDE 2
#define SNERF_RECT_HIDDEN 3
int snerf_orthorectify(const float* dsm, const SnerfDsmGrid* grid, double lon0, int south, const SnerfRectImage* images_host,
                       const SnerfRectImage* images_dev, int n_images, const float* rgbs, const unsigned char* labels,
                       long long n_rows, int n_classes, const unsigned char* visible, long long* sum, unsigned* count,
                       unsigned* votes, double* col_row, float* rgb_out, unsigned char* label_out, unsigned char* state_out,
                       unsigned long long* stats, void* stream);

#ifdef __cplusplus
}
#endif
#endif
