// RPC ray construction, normalisation parameters, in-place normalisation and RPC reprojection on the device (the reference's
// baseline/components/rays.py satnerf_construct, baseline/components/normalization.py, framework/util/conversions.py and
// rpcm's RPCModel).  The spec is stated in include/snerf_hip.h; DESIGN.md "Scenes on disk" gives the layout and the arithmetic
// contract.
//   - ray construction: two launches for every image of a split (rpcm's iteration count of each image and altitude, then
//     the rays).  grid.y = image, the workgroups of a row of the grid stride over that image's rays, one ray per thread.  The image's RPC is read at a workgroup-uniform address (scalar loads).
//     All geometry is fp64; the only fp32 roundings are the final stores, as the reference's `.type(FloatTensor)`;
//   - bounds: per-workgroup min / max partials of the origins and fp32 far points, then one workgroup folds them.  Min and
//     max are exact and commute, so the result does not depend on the grid;
//   - normalise: one thread per row, correctly rounded fp32 subtract and divide.
// No allocation and no host synchronisation; every entry runs on the caller's stream.
#include "geo_dev.h"
#include "reduce.h"
#include "rpc_dev.h"
#include "../../include/snerf_hip.h"

#include <stdint.h>

// numpy evaluates every expression below operation by operation: no fused multiply-adds in this file
#pragma clang fp contract(off)

namespace snerf {

constexpr int RAY_THREADS = 256;
constexpr int RAY_MAX_GRID_X = 1024;     // workgroups per image (they stride over the image's rays)
constexpr int BND_THREADS = 256;
constexpr int BND_MAX_GRID = 1024;       // partial slots per array
constexpr int NRM_THREADS = 256;

static_assert(sizeof(SnerfRpc) == 1368 && sizeof(SnerfRayImage) == 1408, "snerf_amd/_lib.py mirrors these layouts");

// the forward model (rpc_poly, rpc_rfm, rpc_project) and check_rpc live in rpc_dev.h: orthorect.hip projects with them too

// rpcm's iterative inversion runs ONE loop for all points of a call: it updates every point until the last one has met the
// tolerance, so a point that converged early keeps being updated.  The kernels reproduce that in two launches: the first
// counts, per point, the updates after which it meets the tolerance (rpcm's loop test) and folds the maximum over the call
// into a counter (an integer atomic max: exact, order-free); the second runs every point of the call for exactly that many
// updates.  A point still above the tolerance when rpcm would raise (the test at n = 101) counts as failed.
constexpr int RPC_MAX_ITERS = 101;     // rpcm: `if n > 100: raise` at the top of the loop

// rpcm RPCModel.localization_iterative in normalised units.  fixed_iters < 0: stop at the tolerance and return the number of
// updates done (RPC_MAX_ITERS + 1: no convergence); fixed_iters >= 0: do exactly that many updates.
__device__ int rpc_iterate(const SnerfRpc& r, double ncol, double nrow, double nalt, int fixed_iters, double* lon_out,
                           double* lat_out) {
  double lon = -1.0, lat = -1.0;
  double eps = 2.0;
  double x0 = rpc_rfm(r.col_num, r.col_den, lat, lon, nalt);
  double y0 = rpc_rfm(r.row_num, r.row_den, lat, lon, nalt);
  double x1 = rpc_rfm(r.col_num, r.col_den, lat, lon + eps, nalt);
  double y1 = rpc_rfm(r.row_num, r.row_den, lat, lon + eps, nalt);
  double x2 = rpc_rfm(r.col_num, r.col_den, lat + eps, lon, nalt);
  double y2 = rpc_rfm(r.row_num, r.row_den, lat + eps, lon, nalt);
  int n = 0;
  for (;;) {
    if (fixed_iters >= 0) {
      if (n >= fixed_iters) break;
    } else {
      // `!(d < tol)`: a NaN estimate keeps iterating and ends at the iteration cap
      if ((x0 - ncol) * (x0 - ncol) + (y0 - nrow) * (y0 - nrow) < 1e-18) break;
      if (n >= RPC_MAX_ITERS) { n = RPC_MAX_ITERS + 1; break; }
    }
    const double e1x = x1 - x0, e1y = y1 - y0;
    const double e2x = x2 - x0, e2y = y2 - y0;
    const double ux = ncol - x0, uy = nrow - y0;
    const double a1 = (ux * e1x + uy * e1y) / (e1x * e1x + e1y * e1y);
    const double a2 = (ux * e2x + uy * e2y) / (e2x * e2x + e2y * e2y);
    lon += a1 * eps;
    lat += a2 * eps;
    eps = 0.1;
    x0 = rpc_rfm(r.col_num, r.col_den, lat, lon, nalt);
    y0 = rpc_rfm(r.row_num, r.row_den, lat, lon, nalt);
    x1 = rpc_rfm(r.col_num, r.col_den, lat, lon + eps, nalt);
    y1 = rpc_rfm(r.row_num, r.row_den, lat, lon + eps, nalt);
    x2 = rpc_rfm(r.col_num, r.col_den, lat + eps, lon, nalt);
    y2 = rpc_rfm(r.row_num, r.row_den, lat + eps, lon, nalt);
    ++n;
  }
  *lon_out = lon;
  *lat_out = lat;
  return n;
}

__device__ __forceinline__ void rpc_normalise_pixel(const SnerfRpc& r, double col, double row, double alt, double* ncol,
                                                    double* nrow, double* nalt) {
  *ncol = (col - r.col_offset) / r.col_scale;
  *nrow = (row - r.row_offset) / r.row_scale;
  *nalt = (alt - r.alt_offset) / r.alt_scale;
}

// rpcm RPCModel.localization: (col, row, alt) -> (lon, lat), normalised when `normalized`; the iterative branch runs exactly
// `iters` updates (the call's count from the counting launch)
__device__ void rpc_localize(const SnerfRpc& r, double col, double row, double alt, int iters, bool normalized, double* lon_out,
                             double* lat_out) {
  double ncol, nrow, nalt, lon, lat;
  rpc_normalise_pixel(r, col, row, alt, &ncol, &nrow, &nalt);
  if (r.has_inverse) {
    // rpcm: apply_rfm(lon_num, lon_den, nrow, ncol, nalt)
    lon = rpc_rfm(r.lon_num, r.lon_den, nrow, ncol, nalt);
    lat = rpc_rfm(r.lat_num, r.lat_den, nrow, ncol, nalt);
  } else {
    rpc_iterate(r, ncol, nrow, nalt, iters, &lon, &lat);
  }
  if (!normalized) {
    lon = lon * r.lon_scale + r.lon_offset;
    lat = lat * r.lat_scale + r.lat_offset;
  }
  *lon_out = lon;
  *lat_out = lat;
}

// the counting launch of one point: updates to convergence; folds failures and the maximum into counters
__device__ __forceinline__ void rpc_count(const SnerfRpc& r, double col, double row, double alt, int* fails, int* max_iters) {
  if (r.has_inverse) return;
  double ncol, nrow, nalt, lon, lat;
  rpc_normalise_pixel(r, col, row, alt, &ncol, &nrow, &nalt);
  const int n = rpc_iterate(r, ncol, nrow, nalt, -1, &lon, &lat);
  if (n > RPC_MAX_ITERS) atomicAdd(fails, 1);
  else atomicMax(max_iters, n);
}

__device__ __forceinline__ void ray_pixel(const SnerfRayImage& im, const double* pixels, long long i, double* col, double* row) {
  if (pixels == nullptr) {
    *row = (double)(i / im.w);
    *col = (double)(i % im.w);
  } else {
    *col = pixels[2 * (im.row0 + i)];
    *row = pixels[2 * (im.row0 + i) + 1];
  }
}

// counters: [k] failed points of image k, [n_images + 2k] / [n_images + 2k + 1]: rpcm's update count of image k at max_alt /
// min_alt (one rpcm call per image and altitude, as satnerf_construct makes them)
__global__ __launch_bounds__(RAY_THREADS) void rpc_rays_count_kernel(const SnerfRayImage* __restrict__ images, int n_images,
                                                                     const double* __restrict__ pixels, int* __restrict__ counters) {
  const int img = blockIdx.y;
  const SnerfRayImage& im = images[img];
  if (im.rpc.has_inverse) return;
  for (long long i = (long long)blockIdx.x * RAY_THREADS + threadIdx.x; i < im.n_rays; i += (long long)gridDim.x * RAY_THREADS) {
    double col, row;
    ray_pixel(im, pixels, i, &col, &row);
    rpc_count(im.rpc, col, row, im.max_alt, &counters[img], &counters[n_images + 2 * img]);
    rpc_count(im.rpc, col, row, im.min_alt, &counters[img], &counters[n_images + 2 * img + 1]);
  }
}

__global__ __launch_bounds__(RAY_THREADS) void rpc_rays_kernel(const SnerfRayImage* __restrict__ images, int n_images,
                                                               const double* __restrict__ pixels, float* __restrict__ rays,
                                                               const int* __restrict__ counters) {
  const int img = blockIdx.y;
  const SnerfRayImage& im = images[img];
  const int it_near = counters[n_images + 2 * img], it_far = counters[n_images + 2 * img + 1];
  for (long long i = (long long)blockIdx.x * RAY_THREADS + threadIdx.x; i < im.n_rays; i += (long long)gridDim.x * RAY_THREADS) {
    double col, row;
    ray_pixel(im, pixels, i, &col, &row);
    double lon_n, lat_n, lon_f, lat_f;
    // the points of maximum altitude are the nearest to the camera
    rpc_localize(im.rpc, col, row, im.max_alt, it_near, false, &lon_n, &lat_n);
    rpc_localize(im.rpc, col, row, im.min_alt, it_far, false, &lon_f, &lat_f);
    double xn, yn, zn, xf, yf, zf;
    latlon_to_ecef(lat_n, lon_n, im.max_alt, &xn, &yn, &zn);
    latlon_to_ecef(lat_f, lon_f, im.min_alt, &xf, &yf, &zf);
    const double dx = xf - xn, dy = yf - yn, dz = zf - zn;
    const double norm = sqrt(dx * dx + dy * dy + dz * dz);
    float* o = rays + (im.row0 + i) * 8;
    o[0] = (float)xn;
    o[1] = (float)yn;
    o[2] = (float)zn;
    o[3] = (float)(dx / norm);
    o[4] = (float)(dy / norm);
    o[5] = (float)(dz / norm);
    o[6] = 0.0f;
    o[7] = (float)norm;
  }
}

// counters: [0] failed points, [1] the call's update count
__global__ __launch_bounds__(RAY_THREADS) void rpc_localize_count_kernel(const SnerfRpc* __restrict__ rpc, const double* __restrict__ col,
                                                                         const double* __restrict__ row, const double* __restrict__ alt,
                                                                         long long n, int* __restrict__ counters) {
  const long long i = (long long)blockIdx.x * RAY_THREADS + threadIdx.x;
  if (i >= n) return;
  rpc_count(*rpc, col[i], row[i], alt[i], &counters[0], &counters[1]);
}

__global__ __launch_bounds__(RAY_THREADS) void rpc_localize_kernel(const SnerfRpc* __restrict__ rpc, const double* __restrict__ col,
                                                                   const double* __restrict__ row, const double* __restrict__ alt,
                                                                   long long n, int normalized, double* __restrict__ lon,
                                                                   double* __restrict__ lat, const int* __restrict__ counters) {
  const long long i = (long long)blockIdx.x * RAY_THREADS + threadIdx.x;
  if (i >= n) return;
  double a, b;
  rpc_localize(*rpc, col[i], row[i], alt[i], counters[1], normalized != 0, &a, &b);
  lon[i] = a;
  lat[i] = b;
}

__global__ __launch_bounds__(RAY_THREADS) void rpc_project_kernel(const SnerfRpc* __restrict__ rpc, const double* __restrict__ lon,
                                                                  const double* __restrict__ lat, const double* __restrict__ alt,
                                                                  long long n, double* __restrict__ col, double* __restrict__ row) {
  const long long i = (long long)blockIdx.x * RAY_THREADS + threadIdx.x;
  if (i >= n) return;
  double c, r;
  rpc_project(*rpc, lon[i], lat[i], alt[i], &c, &r);
  col[i] = c;
  row[i] = r;
}

__global__ __launch_bounds__(RAY_THREADS) void rpc_reproject_kernel(const SnerfRpc* __restrict__ rpc, const double* __restrict__ xyz,
                                                                    const double* __restrict__ pts2d, long long n,
                                                                    double* __restrict__ col_row, double* __restrict__ err) {
  const long long i = (long long)blockIdx.x * RAY_THREADS + threadIdx.x;
  if (i >= n) return;
  double lat, lon, alt, c, r;
  ecef_to_latlon(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], &lat, &lon, &alt);
  rpc_project(*rpc, lon, lat, alt, &c, &r);
  if (col_row) {
    col_row[2 * i] = c;
    col_row[2 * i + 1] = r;
  }
  const double ec = pts2d[2 * i] - c, er = pts2d[2 * i + 1] - r;
  err[i] = sqrt(ec * ec + er * er);   // np.linalg.norm(pts2d - reprojected, axis=1)
}

// the workgroup's three minima (components 0..2, fminf) and three maxima (3..5, fmaxf): results at red[k * BND_THREADS]
__device__ __forceinline__ void bounds_tree(float* red, int t, const float* v) {
  block_tree<BND_THREADS, 6>(red, t, v, [](int k, float a, float b) { return k < 3 ? fminf(a, b) : fmaxf(a, b); });
}

// per-workgroup min (slots 0..2) and max (3..5) over the origins and the far points o + far * d (fp32, two roundings)
__global__ __launch_bounds__(BND_THREADS) void ray_bounds_partial_kernel(const float* __restrict__ rays, long long n,
                                                                         float* __restrict__ partial) {
  __shared__ float red[6 * BND_THREADS];
  float v[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
  for (long long i = (long long)blockIdx.x * BND_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * BND_THREADS) {
    const float* r = rays + i * 8;
    const float far = r[7];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float o = r[k];
      const float p = __fadd_rn(o, __fmul_rn(far, r[3 + k]));
      v[k] = fminf(v[k], fminf(o, p));
      v[3 + k] = fmaxf(v[3 + k], fmaxf(o, p));
    }
  }
  const int t = threadIdx.x;
  bounds_tree(red, t, v);
  if (t < 6) partial[(long long)blockIdx.x * 6 + t] = red[t * BND_THREADS];
}

// folds n_partials slots; out: min[3], max[3], scale[3] = (max - min) / 2, offset[3] = min + scale, range = max(scale)
__global__ __launch_bounds__(BND_THREADS) void ray_bounds_finish_kernel(const float* __restrict__ partial, int n_partials,
                                                                        float* __restrict__ out) {
  __shared__ float red[6 * BND_THREADS];
  const int t = threadIdx.x;
  float v[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
  for (int p = t; p < n_partials; p += BND_THREADS) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      v[k] = fminf(v[k], partial[6 * p + k]);
      v[3 + k] = fmaxf(v[3 + k], partial[6 * p + 3 + k]);
    }
  }
  bounds_tree(red, t, v);
  if (t == 0) {
    float range = -INFINITY;
    for (int k = 0; k < 3; ++k) {
      const float mn = red[k * BND_THREADS], mx = red[(3 + k) * BND_THREADS];
      const float scale = __fmul_rn(__fsub_rn(mx, mn), 0.5f);   // numpy float32 (max - min) / 2: the halving is exact
      out[k] = mn;
      out[3 + k] = mx;
      out[6 + k] = scale;
      out[9 + k] = __fadd_rn(mn, scale);
      range = fmaxf(range, scale);
    }
    out[12] = range;
  }
}

__global__ __launch_bounds__(NRM_THREADS) void normalize_rows_kernel(float* __restrict__ rows, long long n, int stride,
                                                                     int bounds, const float* __restrict__ center_range) {
  const long long i = (long long)blockIdx.x * NRM_THREADS + threadIdx.x;
  if (i >= n) return;
  const float range = center_range[3];
  float* r = rows + i * stride;
#pragma unroll
  for (int k = 0; k < 3; ++k) r[k] = __fdiv_rn(__fsub_rn(r[k], center_range[k]), range);
  if (bounds) {
    r[6] = __fdiv_rn(r[6], range);
    r[7] = __fdiv_rn(r[7], range);
  }
}

// one item per thread, no grid stride: n <= 2^31 at every caller
static inline long long blocks_of(long long n, int threads) { return (n + threads - 1) / threads; }

}  // namespace snerf

using namespace snerf;

extern "C" int snerf_rpc_rays(const SnerfRayImage* images_host, const SnerfRayImage* images_dev, int n_images,
                              const double* pixels, long long n_rows, float* rays, int* counters, void* stream) {
  const char* who = "snerf_rpc_rays";
  if (!images_host || !images_dev || !rays || !counters) { set_error("%s: null pointer", who); return SNERF_ERR_NULL; }
  if (n_images < 1 || n_images > 65535) { set_error("%s: n_images = %d outside [1, 65535]", who, n_images); return SNERF_ERR_BAD_DESC; }
  if (n_rows < 1) { set_error("%s: n_rows = %lld < 1", who, n_rows); return SNERF_ERR_BAD_DESC; }
  if (n_rows > (long long)1 << 40) { set_error("%s: n_rows = %lld too large", who, n_rows); return SNERF_ERR_BAD_DESC; }
  long long sum = 0, max_n = 0;
  for (int k = 0; k < n_images; ++k) {
    const SnerfRayImage& im = images_host[k];
    if (im.n_rays < 1) { set_error("%s: image %d has %lld rays", who, k, im.n_rays); return SNERF_ERR_BAD_DESC; }
    if (im.row0 != sum) { set_error("%s: image %d starts at row %lld, expected %lld", who, k, im.row0, sum); return SNERF_ERR_BAD_DESC; }
    if (pixels == nullptr) {
      long long wh;
      if (im.w < 1 || im.h < 1 || __builtin_mul_overflow((long long)im.w, (long long)im.h, &wh) || wh > (long long)1 << 40) {
        set_error("%s: image %d has a bad grid %d x %d", who, k, im.w, im.h); return SNERF_ERR_BAD_DESC; }
      if (wh != im.n_rays) { set_error("%s: image %d: w * h = %lld != n_rays = %lld", who, k, wh, im.n_rays); return SNERF_ERR_BAD_DESC; }
    }
    if (!(im.min_alt < im.max_alt)) { set_error("%s: image %d needs min_alt < max_alt", who, k); return SNERF_ERR_BAD_DESC; }
    if (int rc = check_rpc(im.rpc, who, k)) return rc;
    if (__builtin_add_overflow(sum, im.n_rays, &sum)) { set_error("%s: ray count overflows", who); return SNERF_ERR_BAD_DESC; }
    max_n = im.n_rays > max_n ? im.n_rays : max_n;
  }
  if (sum != n_rows) { set_error("%s: the images hold %lld rays, the output %lld rows", who, sum, n_rows); return SNERF_ERR_BAD_DESC; }
  const unsigned gx = blocks_for(max_n, RAY_THREADS, RAY_MAX_GRID_X);
  hipLaunchKernelGGL(rpc_rays_count_kernel, dim3(gx, (unsigned)n_images), dim3(RAY_THREADS), 0, (hipStream_t)stream,
                     images_dev, n_images, pixels, counters);
  SNERF_LAUNCH_CHECK();
  hipLaunchKernelGGL(rpc_rays_kernel, dim3(gx, (unsigned)n_images), dim3(RAY_THREADS), 0, (hipStream_t)stream,
                     images_dev, n_images, pixels, rays, (const int*)counters);
  SNERF_LAUNCH_CHECK();
  return SNERF_OK;
}

extern "C" int snerf_rpc_localize(const SnerfRpc* rpc_host, const SnerfRpc* rpc_dev, const double* col, const double* row,
                                  const double* alt, long long n, int normalized, double* lon, double* lat, int* counters,
                                  void* stream) {
  const char* who = "snerf_rpc_localize";
  if (!rpc_host || !rpc_dev || !col || !row || !alt || !lon || !lat || !counters) { set_error("%s: null pointer", who); return SNERF_ERR_NULL; }
  if (n < 0 || n > (long long)1 << 31) { set_error("%s: n = %lld outside [0, 2^31]", who, n); return SNERF_ERR_BAD_DESC; }
  if (int rc = check_rpc(*rpc_host, who, 0)) return rc;
  if (n == 0) return SNERF_OK;
  hipLaunchKernelGGL(rpc_localize_count_kernel, dim3((unsigned)blocks_of(n, RAY_THREADS)), dim3(RAY_THREADS), 0, (hipStream_t)stream,
                     rpc_dev, col, row, alt, n, counters);
  SNERF_LAUNCH_CHECK();
  hipLaunchKernelGGL(rpc_localize_kernel, dim3((unsigned)blocks_of(n, RAY_THREADS)), dim3(RAY_THREADS), 0, (hipStream_t)stream,
                     rpc_dev, col, row, alt, n, normalized, lon, lat, (const int*)counters);
  SNERF_LAUNCH_CHECK();
  return SNERF_OK;
}

extern "C" int snerf_rpc_project(const SnerfRpc* rpc_host, const SnerfRpc* rpc_dev, const double* lon, const double* lat,
                                 const double* alt, long long n, double* col, double* row, void* stream) {
  const char* who = "snerf_rpc_project";
  if (!rpc_host || !rpc_dev || !lon || !lat || !alt || !col || !row) { set_error("%s: null pointer", who); return SNERF_ERR_NULL; }
  if (n < 0 || n > (long long)1 << 31) { set_error("%s: n = %lld outside [0, 2^31]", who, n); return SNERF_ERR_BAD_DESC; }
  if (int rc = check_rpc(*rpc_host, who, 0)) return rc;
  if (n == 0) return SNERF_OK;
  hipLaunchKernelGGL(rpc_project_kernel, dim3((unsigned)blocks_of(n, RAY_THREADS)), dim3(RAY_THREADS), 0, (hipStream_t)stream,
                     rpc_dev, lon, lat, alt, n, col, row);
  SNERF_LAUNCH_CHECK();
  return SNERF_OK;
}

extern "C" int snerf_rpc_reprojection_error(const SnerfRpc* rpc_host, const SnerfRpc* rpc_dev, const double* xyz_ecef,
                                            const double* pts2d, long long n, double* col_row, double* err, void* stream) {
  const char* who = "snerf_rpc_reprojection_error";
  if (!rpc_host || !rpc_dev || !xyz_ecef || !pts2d || !err) { set_error("%s: null pointer", who); return SNERF_ERR_NULL; }
  if (n < 0 || n > (long long)1 << 31) { set_error("%s: n = %lld outside [0, 2^31]", who, n); return SNERF_ERR_BAD_DESC; }
  if (int rc = check_rpc(*rpc_host, who, 0)) return rc;
  if (n == 0) return SNERF_OK;
  hipLaunchKernelGGL(rpc_reproject_kernel, dim3((unsigned)blocks_of(n, RAY_THREADS)), dim3(RAY_THREADS), 0, (hipStream_t)stream,
                     rpc_dev, xyz_ecef, pts2d, n, col_row, err);
  SNERF_LAUNCH_CHECK();
  return SNERF_OK;
}

extern "C" size_t snerf_ray_bounds_workspace_bytes(const long long* n_rows, int n_arrays) {
  if (!n_rows || n_arrays < 1) { set_error("snerf_ray_bounds_workspace_bytes: need at least one array"); return 0; }
  long long slots = 0;
  for (int a = 0; a < n_arrays; ++a) {
    if (n_rows[a] < 1 || n_rows[a] > (long long)1 << 40) { set_error("snerf_ray_bounds_workspace_bytes: array %d has %lld rows", a, n_rows[a]); return 0; }
    slots += blocks_for(n_rows[a], BND_THREADS, BND_MAX_GRID);
  }
  return (size_t)slots * 6 * sizeof(float);
}

extern "C" int snerf_ray_bounds(const float* const* rays, const long long* n_rows, int n_arrays, float* out, void* workspace,
                                size_t workspace_bytes, void* stream) {
  const char* who = "snerf_ray_bounds";
  if (!rays || !n_rows || !out || !workspace) { set_error("%s: null pointer", who); return SNERF_ERR_NULL; }
  if (n_arrays < 1 || n_arrays > 64) { set_error("%s: n_arrays = %d outside [1, 64]", who, n_arrays); return SNERF_ERR_BAD_DESC; }
  long long slots = 0;
  for (int a = 0; a < n_arrays; ++a) {
    if (!rays[a]) { set_error("%s: array %d is null", who, a); return SNERF_ERR_NULL; }
    if (n_rows[a] < 1 || n_rows[a] > (long long)1 << 40) { set_error("%s: array %d has %lld rows", who, a, n_rows[a]); return SNERF_ERR_BAD_DESC; }
    slots += blocks_for(n_rows[a], BND_THREADS, BND_MAX_GRID);
  }
  if (workspace_bytes < (size_t)slots * 6 * sizeof(float)) {
    set_error("%s: workspace of %zu bytes < %zu", who, workspace_bytes, (size_t)slots * 6 * sizeof(float)); return SNERF_ERR_WORKSPACE; }
  if (slots > (long long)1 << 30) { set_error("%s: too many partial slots", who); return SNERF_ERR_BAD_DESC; }
  hipStream_t st = (hipStream_t)stream;
  float* part = (float*)workspace;
  long long at = 0;
  for (int a = 0; a < n_arrays; ++a) {
    const unsigned g = blocks_for(n_rows[a], BND_THREADS, BND_MAX_GRID);
    hipLaunchKernelGGL(ray_bounds_partial_kernel, dim3(g), dim3(BND_THREADS), 0, st, rays[a], n_rows[a], part + at * 6);
    SNERF_LAUNCH_CHECK();
    at += g;
  }
  hipLaunchKernelGGL(ray_bounds_finish_kernel, dim3(1), dim3(BND_THREADS), 0, st, (const float*)part, (int)slots, out);
  SNERF_LAUNCH_CHECK();
  return SNERF_OK;
}

extern "C" int snerf_normalize_rows(float* rows, long long n, int stride, int bounds, const float* center_range, void* stream) {
  const char* who = "snerf_normalize_rows";
  if (!rows || !center_range) { set_error("%s: null pointer", who); return SNERF_ERR_NULL; }
  if (n < 0 || n > (long long)1 << 31) { set_error("%s: n = %lld outside [0, 2^31]", who, n); return SNERF_ERR_BAD_DESC; }
  if (bounds != 0 && bounds != 1) { set_error("%s: bounds = %d", who, bounds); return SNERF_ERR_BAD_DESC; }
  if (stride < (bounds ? 8 : 3)) { set_error("%s: stride %d < %d", who, stride, bounds ? 8 : 3); return SNERF_ERR_BAD_DESC; }
  if (n == 0) return SNERF_OK;
  hipLaunchKernelGGL(normalize_rows_kernel, dim3((unsigned)blocks_of(n, NRM_THREADS)), dim3(NRM_THREADS), 0, (hipStream_t)stream,
                     rows, n, stride, bounds, center_range);
  SNERF_LAUNCH_CHECK();
  return SNERF_OK;
}
