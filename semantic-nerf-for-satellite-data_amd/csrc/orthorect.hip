// Orthorectification on the DSM lattice: every cell of the output window is projected into every image of the call (UTM -> lat /
// lon once per cell, the RPC projection once per cell and image), the image's colour is sampled bilinearly and its label at the
// nearest pixel, and both are fused into integer accumulators -- the true ortho-image per date, the multi-date mosaic and the
// voted ground-truth class raster.  The spec is include/snerf_orthorect.h and DESIGN.md section 5t;
// tests/orthorect_numpy.py restates it.
//   - one thread per cell (the workgroups stride over the cells), a loop over the images inside the thread: a cell's sum, count
//     and votes have exactly one writer per launch, so they are plain read-modify-writes, and a cell's (lat, lon) -- five sines, a
//     cosine and a square root -- is evaluated once for all images;
//   - the image table is read at a wave-uniform address (the 80 RPC coefficients of an image come as scalar loads);
//   - fp64, evaluated operation by operation (no fused multiply-adds in this file); utm_to_latlon and rpc_project are the device
//     functions geo.hip and satrays.hip use, so col_row carries the bits of snerf_geo_points followed by snerf_rpc_project;
//   - the four state totals are folded per wave with shuffles, per workgroup through LDS, then one 64-bit integer atomic add per
//     workgroup and word: exact and independent of the launch order.
// No allocation, no copy and no host synchronisation; the entry runs on the caller's stream.
#include "geo_dev.h"
#include "lattice.h"
#include "reduce.h"
#include "rpc_dev.h"
#include "../../include/snerf_orthorect.h"

#pragma clang fp contract(off)

namespace snerf {

constexpr int RECT_THREADS = 256;
constexpr int RECT_WAVES = RECT_THREADS / 64;
constexpr unsigned RECT_MAX_BLOCKS = 8192;             // workgroups (they stride over the cells)

static_assert(sizeof(SnerfRectImage) == 1384, "snerf_amd/_lib.py mirrors this layout");
static_assert(SNERF_RECT_MAX_IMAGES == SNERF_SHADOW_MAX_SUNS, "one cast call makes one call's visibility planes");

__device__ __forceinline__ int rect_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

__global__ __launch_bounds__(RECT_THREADS) void orthorectify_kernel(
    const float* __restrict__ dsm, SnerfDsmGrid g, double lon0, int south, const SnerfRectImage* __restrict__ images, int n_images,
    const float* __restrict__ rgbs, const unsigned char* __restrict__ labels, int n_classes, const unsigned char* __restrict__ visible,
    long long* __restrict__ sum, unsigned* __restrict__ count, unsigned* __restrict__ votes, double* __restrict__ col_row,
    float* __restrict__ rgb_out, unsigned char* __restrict__ label_out, unsigned char* __restrict__ state_out,
    unsigned long long* __restrict__ stats) {
  const long long cells = (long long)g.out_h * g.out_w;
  const double nan = __builtin_nan("");
  const float nanf = __builtin_nanf("");
  unsigned long long n_state[4] = {0, 0, 0, 0};
  for (long long c = (long long)blockIdx.x * RECT_THREADS + threadIdx.x; c < cells; c += (long long)gridDim.x * RECT_THREADS) {
    const unsigned jj = (unsigned)c / (unsigned)g.out_w, ii = (unsigned)c - jj * (unsigned)g.out_w;      // cells < 2^31
    const double east = g.xoff + ((double)((long long)g.ioff + ii) + 0.5) * g.res;
    const double north = g.yoff - ((double)((long long)g.joff + jj) + 0.5) * g.res;
    const double alt = (double)dsm[c];
    const bool hole = !__builtin_isfinite(alt);
    double lat = nan, lon = nan;
    if (!hole) utm_to_latlon(east, north, lon0, south, &lat, &lon);
    long long add[3] = {0, 0, 0};
    unsigned seen = 0;
    for (int k = 0; k < n_images; ++k) {
      const SnerfRectImage& im = images[k];
      const long long o = (long long)k * cells + c;
      double col = nan, row = nan;
      int state = SNERF_RECT_HOLE;
      float px[3] = {nanf, nanf, nanf};
      unsigned char lab = SNERF_ORTHO_NO_LABEL;
      if (!hole) {
        rpc_project(im.rpc, lon, lat, alt, &col, &row);
        const double ci = floor(col + 0.5), ri = floor(row + 0.5);
        state = SNERF_RECT_OUTSIDE;
        if (ci >= 0.0 && ci < (double)im.w && ri >= 0.0 && ri < (double)im.h) {      // false for NaN and infinity
          if (visible != nullptr && visible[o] != 1) {
            state = SNERF_RECT_HIDDEN;
          } else {
            // col lies in [-0.5, w - 0.5): floor(col) in [-1, w - 1], exact as an int; the same for row
            const double c0 = floor(col), r0 = floor(row);
            const double fx = col - c0, fy = row - r0;
            const int x0 = rect_clamp((int)c0, im.w - 1), x1 = rect_clamp((int)c0 + 1, im.w - 1);
            const int y0 = rect_clamp((int)r0, im.h - 1), y1 = rect_clamp((int)r0 + 1, im.h - 1);
            const float* p00 = rgbs + 3 * (im.row0 + (long long)y0 * im.w + x0);
            const float* p10 = rgbs + 3 * (im.row0 + (long long)y0 * im.w + x1);
            const float* p01 = rgbs + 3 * (im.row0 + (long long)y1 * im.w + x0);
            const float* p11 = rgbs + 3 * (im.row0 + (long long)y1 * im.w + x1);
            double v[3];
            bool finite = true;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
              const double top = (1.0 - fx) * (double)p00[ch] + fx * (double)p10[ch];
              const double bot = (1.0 - fx) * (double)p01[ch] + fx * (double)p11[ch];
              v[ch] = (1.0 - fy) * top + fy * bot;
              finite = finite && __builtin_isfinite(v[ch]);
            }
            if (finite) {
              state = SNERF_RECT_SEEN;
              ++seen;
#pragma unroll
              for (int ch = 0; ch < 3; ++ch) {
                px[ch] = (float)v[ch];
                double q = v[ch] * 16777216.0;
                q = q > 4611686018427387904.0 ? 4611686018427387904.0 : (q < -4611686018427387904.0 ? -4611686018427387904.0 : q);
                add[ch] += llrint(q);
              }
              if (labels != nullptr) {
                lab = labels[im.row0 + (long long)ri * im.w + (long long)ci];
                if ((int)lab < n_classes) votes[(long long)lab * cells + c] += 1u;      // this thread is the cell's only writer
              }
            }
          }
        }
      }
#pragma unroll
      for (int s = 0; s < 4; ++s) n_state[s] += state == s;       // no runtime index into a per-thread array
      if (col_row != nullptr) {
        col_row[(2LL * k) * cells + c] = col;
        col_row[(2LL * k + 1) * cells + c] = row;
      }
      if (rgb_out != nullptr) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) rgb_out[(3LL * k + ch) * cells + c] = px[ch];
      }
      if (label_out != nullptr) label_out[o] = lab;
      if (state_out != nullptr) state_out[o] = (unsigned char)state;
    }
    if (seen) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) sum[ch * cells + c] += add[ch];
      count[c] += seen;
    }
  }
  // every thread of the workgroup arrives here (the loop has ended for the whole wave)
  __shared__ unsigned long long red[4][RECT_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const unsigned long long v = wave_reduce(n_state[s], OpSum());
    if (lane == 0) red[s][wave] = v;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    unsigned long long v = 0;
#pragma unroll
    for (int w = 0; w < RECT_WAVES; ++w) v += red[threadIdx.x][w];
    if (v) atomicAdd(&stats[threadIdx.x], v);
  }
}

}  // namespace snerf

using namespace snerf;

extern "C" int snerf_orthorectify(const float* dsm, const SnerfDsmGrid* grid, double lon0, int south, const SnerfRectImage* images_host,
                                  const SnerfRectImage* images_dev, int n_images, const float* rgbs, const unsigned char* labels,
                                  long long n_rows, int n_classes, const unsigned char* visible, long long* sum, unsigned* count,
                                  unsigned* votes, double* col_row, float* rgb_out, unsigned char* label_out, unsigned char* state_out,
                                  unsigned long long* stats, void* stream) {
  const char* who = "snerf_orthorectify";
  if (!dsm || !grid || !images_host || !images_dev || !rgbs || !sum || !count || !stats) { set_error("%s: null pointer", who); return SNERF_ERR_NULL; }
  if ((labels == nullptr) != (votes == nullptr)) { set_error("%s: labels and votes go together (one of them is null)", who); return SNERF_ERR_NULL; }
  if (!lattice_grid_ok(who, grid) || !lattice_window_fits_int32(who, grid)) return SNERF_ERR_BAD_DESC;
  if (!lattice_window_cells_ok(who, grid)) return SNERF_ERR_BAD_DESC;
  if (n_images < 1 || n_images > SNERF_RECT_MAX_IMAGES) {
    set_error("%s: n_images = %d outside [1, %d]", who, n_images, SNERF_RECT_MAX_IMAGES);
    return SNERF_ERR_BAD_DESC;
  }
  if (labels && (n_classes < 1 || n_classes > SNERF_ORTHO_MAX_CLASSES)) {
    set_error("%s: n_classes = %d outside [1, %d]", who, n_classes, SNERF_ORTHO_MAX_CLASSES);
    return SNERF_ERR_BAD_DESC;
  }
  if (n_rows < 1) { set_error("%s: n_rows = %lld < 1", who, n_rows); return SNERF_ERR_BAD_DESC; }
  if (!(lon0 >= -M_PI && lon0 <= M_PI)) { set_error("%s: central meridian %g rad outside [-pi, pi]", who, lon0); return SNERF_ERR_BAD_DESC; }
  if (south != 0 && south != 1) { set_error("%s: south = %d", who, south); return SNERF_ERR_BAD_DESC; }
  for (int k = 0; k < n_images; ++k) {
    const SnerfRectImage& im = images_host[k];
    long long wh, end;
    if (im.w < 1 || im.h < 1 || __builtin_mul_overflow((long long)im.w, (long long)im.h, &wh)) {
      set_error("%s: image %d has a bad size %d x %d", who, k, im.w, im.h);
      return SNERF_ERR_BAD_DESC;
    }
    if (im.row0 < 0 || __builtin_add_overflow(im.row0, wh, &end) || end > n_rows) {
      set_error("%s: image %d: rows [%lld, %lld + %lld) do not lie in [0, %lld)", who, k, im.row0, im.row0, wh, n_rows);
      return SNERF_ERR_BAD_DESC;
    }
    if (int rc = check_rpc(im.rpc, who, k)) return rc;
  }
  const long long cells = (long long)grid->out_h * grid->out_w;
  hipLaunchKernelGGL(orthorectify_kernel, dim3(blocks_for(cells, RECT_THREADS, RECT_MAX_BLOCKS)), dim3(RECT_THREADS), 0,
                     (hipStream_t)stream, dsm, *grid, lon0, south, images_dev, n_images, rgbs, labels, n_classes, visible, sum, count,
                     votes, col_row, rgb_out, label_out, state_out, stats);
  SNERF_LAUNCH_CHECK();
  return SNERF_OK;
}
