// SSIM on the device (eval/utils/metrics.py: the kornia form with window 3 and reflect padding, and ssim_inria with a
// Gaussian window and zero padding).  The spec and the numerics are stated in include/snerf_hip.h and in
// snerf_amd/eval/utils/metrics.py.  Two launches, no atomics: the tile kernel writes one fp64 partial sum per workgroup at a
// fixed slot, and the reduce kernel sums each image's slots in a fixed order, so every result is bit-reproducible run to run
// and an image's value does not depend on the other images of the batch.
#include "reduce.h"
#include "../../include/snerf_hip.h"

#include <math.h>

namespace snerf {

constexpr int SSIM_TILE = 16;                 // output tile: 16 x 16 pixels, one per thread
constexpr int SSIM_THREADS = SSIM_TILE * SSIM_TILE;
constexpr int SSIM_MAX_WS = 31;
// LDS row pitch in float2 (x, y) pairs: >= 16 + ws - 1 for every ws <= 31, and = 16 (mod 32) pairs, so the two rows a half
// wave reads with one ds_read_b64 (16 pairs = 32 dwords each) fall on the two halves of the 64 banks (conflict-free)
constexpr int SSIM_PITCH = 48;
constexpr int SSIM_REDUCE_THREADS = 256;

__device__ __forceinline__ int ssim_src(int i, int n, int border) {
  // reflect (index -1 reads 1; the host guarantees ws // 2 < n, so one reflection lands inside for every pixel that is
  // used) or zero; -1 = a zero, also for the halo of tile pixels beyond the image, which no output reads
  if (border == SNERF_SSIM_REFLECT) {
    if (i < 0) i = -i;
    else if (i >= n) i = 2 * (n - 1) - i;
  }
  return (i >= 0 && i < n) ? i : -1;
}

// One workgroup per (image, plane, 16 x 16 output tile): stages the tile and its ws - 1 halo of both inputs in LDS with the
// border resolved at load time, takes the five window sums over the ws x ws taps in fp64 (fp32 weights and inputs, exact
// fp64 products), forms the SSIM value in fp64, optionally stores it as fp32, and writes the tile's sum (fixed-order tree)
// to partial[blockIdx.x].
__global__ __launch_bounds__(SSIM_THREADS) void ssim_tile_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                 int h, int w, int ws, int border,
                                                                 const float* __restrict__ weights, double c1, double c2,
                                                                 double eps, int tiles_x, int tiles_per_plane,
                                                                 float* __restrict__ map, double* __restrict__ partial) {
  __shared__ float2 S[(SSIM_TILE + SSIM_MAX_WS - 1) * SSIM_PITCH];
  __shared__ double red[SSIM_THREADS];
  const long long blk = blockIdx.x;
  const long long plane = blk / tiles_per_plane;
  const int t = (int)(blk - plane * tiles_per_plane);
  const int x0 = (t % tiles_x) * SSIM_TILE, y0 = (t / tiles_x) * SSIM_TILE;
  const int r = ws / 2, span = SSIM_TILE + ws - 1;
  const float* xp = x + plane * h * (long long)w;
  const float* yp = y + plane * h * (long long)w;
  for (int k = threadIdx.x; k < span * span; k += SSIM_THREADS) {
    const int ly = k / span, lx = k % span;
    const int sy = ssim_src(y0 - r + ly, h, border), sx = ssim_src(x0 - r + lx, w, border);
    float2 v = make_float2(0.f, 0.f);
    if (sy >= 0 && sx >= 0) {
      const long long o = (long long)sy * w + sx;
      v = make_float2(xp[o], yp[o]);
    }
    S[ly * SSIM_PITCH + lx] = v;
  }
  __syncthreads();
  const int tx = threadIdx.x % SSIM_TILE, ty = threadIdx.x / SSIM_TILE;
  const int ox = x0 + tx, oy = y0 + ty;
  double val = 0.0;
  if (ox < w && oy < h) {
    double m1 = 0.0, m2 = 0.0, s11 = 0.0, s22 = 0.0, s12 = 0.0;
    for (int ky = 0; ky < ws; ++ky) {
      const float2* row = S + (ty + ky) * SSIM_PITCH + tx;
      const float* wr = weights + ky * ws;
      for (int kx = 0; kx < ws; ++kx) {
        const double g = (double)wr[kx];
        const float2 v = row[kx];
        const double a = (double)v.x, b = (double)v.y;
        m1 = fma(g, a, m1);
        m2 = fma(g, b, m2);
        s11 = fma(g, a * a, s11);
        s22 = fma(g, b * b, s22);
        s12 = fma(g, a * b, s12);
      }
    }
    const double mu11 = m1 * m1, mu22 = m2 * m2, mu12 = m1 * m2;
    const double sig1 = s11 - mu11, sig2 = s22 - mu22, sig12 = s12 - mu12;
    const double num = (2.0 * mu12 + c1) * (2.0 * sig12 + c2);
    const double den = (mu11 + mu22 + c1) * (sig1 + sig2 + c2);
    val = num / (den + eps);
    if (map) map[plane * h * (long long)w + (long long)oy * w + ox] = (float)val;
  }
  block_tree<SSIM_THREADS>(red, threadIdx.x, val, OpSum());
  if (threadIdx.x == 0) partial[blk] = red[0];
}

// one workgroup per image: the sum of its per_image partials (c planes x tiles, contiguous) in the order of reduce.h
__global__ __launch_bounds__(SSIM_REDUCE_THREADS) void ssim_reduce_kernel(const double* __restrict__ partial, long long per_image,
                                                                          double* __restrict__ sums) {
  __shared__ double red[SSIM_REDUCE_THREADS];
  block_strided_sum<SSIM_REDUCE_THREADS>(red, threadIdx.x, partial + (long long)blockIdx.x * per_image, per_image, 1);
  if (threadIdx.x == 0) sums[blockIdx.x] = red[0];
}

// number of tile workgroups (= fp64 partials) of a (b, c, h, w) batch; -1 on bad sizes, with the error set
static long long ssim_tiles(const char* who, int b, int c, int h, int w, int ws) {
  if (b <= 0 || c <= 0 || h <= 0 || w <= 0) { set_error("%s: b, c, h, w must be > 0", who); return -1; }
  if (ws < 1 || ws > SSIM_MAX_WS || ws % 2 == 0) { set_error("%s: window size %d must be odd and lie in [1, %d]", who, ws, SSIM_MAX_WS); return -1; }
  const long long per_plane = (long long)((w + SSIM_TILE - 1) / SSIM_TILE) * ((h + SSIM_TILE - 1) / SSIM_TILE);
  const long long planes = (long long)b * c;
  // the tile grid is one-dimensional (< 2^31 workgroups); the element count stays far below 2^63
  if (planes > (1LL << 31) / per_plane || (long long)h * w > (1LL << 40) / planes) {
    set_error("%s: %d x %d x %d x %d is too large", who, b, c, h, w); return -1; }
  const long long n = planes * per_plane;
  if (n >= (1LL << 31)) { set_error("%s: %d x %d x %d x %d is too large", who, b, c, h, w); return -1; }
  return n;
}

}  // namespace snerf

using namespace snerf;

extern "C" size_t snerf_ssim_workspace_bytes(int b, int c, int h, int w, int ws) {
  const long long n = ssim_tiles("snerf_ssim_workspace_bytes", b, c, h, w, ws);
  return n < 0 ? 0 : (size_t)n * sizeof(double);
}

extern "C" int snerf_ssim(const float* x, const float* y, int b, int c, int h, int w, int ws, int border,
                          const float* weights2d, double c1, double c2, double eps, float* map_or_null, double* per_image_sum,
                          void* workspace, size_t workspace_bytes, void* stream) {
  if (!x || !y || !weights2d || !per_image_sum || !workspace) { set_error("snerf_ssim: null pointer"); return SNERF_ERR_NULL; }
  const long long n = ssim_tiles("snerf_ssim", b, c, h, w, ws);
  if (n < 0) return SNERF_ERR_BAD_DESC;
  if (border != SNERF_SSIM_REFLECT && border != SNERF_SSIM_ZERO) { set_error("snerf_ssim: unknown border mode %d", border); return SNERF_ERR_BAD_DESC; }
  if (border == SNERF_SSIM_REFLECT && (ws / 2 >= h || ws / 2 >= w)) {
    set_error("snerf_ssim: reflect padding of %d needs an image larger than %d x %d", ws / 2, h, w); return SNERF_ERR_BAD_DESC; }
  if (!isfinite(c1) || !isfinite(c2) || !isfinite(eps)) { set_error("snerf_ssim: c1, c2 and eps must be finite"); return SNERF_ERR_BAD_DESC; }
  if (workspace_bytes < (size_t)n * sizeof(double)) {
    set_error("snerf_ssim: workspace of %zu bytes < %zu", workspace_bytes, (size_t)n * sizeof(double)); return SNERF_ERR_WORKSPACE; }
  const int tiles_x = (w + SSIM_TILE - 1) / SSIM_TILE;
  const int per_plane = (int)(n / ((long long)b * c));
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(ssim_tile_kernel, dim3((unsigned)n), dim3(SSIM_THREADS), 0, st, x, y, h, w, ws, border, weights2d, c1, c2,
                     eps, tiles_x, per_plane, map_or_null, (double*)workspace);
  SNERF_LAUNCH_CHECK();
  hipLaunchKernelGGL(ssim_reduce_kernel, dim3((unsigned)b), dim3(SSIM_REDUCE_THREADS), 0, st, (const double*)workspace,
                     (long long)c * per_plane, per_image_sum);
  SNERF_LAUNCH_CHECK();
  return SNERF_OK;
}
