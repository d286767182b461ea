// World clouds on the device: a frame's rays and depth (or normalised end points) to metric (east, north, alt) UTM points and,
// optionally, (lat, lon, alt) -- the reference's get_xyz_from_nerf_prediction, StandardNormalization.denormalize,
// ecef_to_latlon_custom and utm.from_latlon (its eval/utils/dsm.py get_utm_cloud path), which it runs in numpy on the host.
// The way back (SnerfGeoParams.direction = 1, snerf_geo_points only): UTM (east, north, alt) -> lat / lon (utm.to_latlon) -> custom
// ECEF -> normalised scene coordinates, the reference's convert_utm_to_local, for casting a vertical ray per map cell.
// The spec is stated in include/snerf_hip.h; DESIGN.md sections 5h and 5l give the arithmetic contracts.
//   - one launch, one point per thread (the workgroups stride over the points), every step fp64 and evaluated operation by
//     operation as torch / numpy do: no fused multiply-adds in this file;
//   - the east / north bounds the DSM grid needs (direction 1: the bounds of scene x / y) are folded in the same launch: per wave
//     with shuffles, per workgroup through LDS, then ONE 64-bit integer atomic min / max per workgroup and bound on an
//     order-preserving integer key of the double.
//     Min and max are exact and commute, so the bounds do not depend on the grid or on the order the workgroups arrive in;
//   - a point that is not finite is written as it comes, left out of the bounds and counted.
// No allocation and no host synchronisation; both entries run on the caller's stream.
#include "geo_dev.h"
#include "reduce.h"
#include "../../include/snerf_hip.h"

#include <stdint.h>

#pragma clang fp contract(off)

namespace snerf {

constexpr int GEO_THREADS = 256;
constexpr int GEO_WAVES = GEO_THREADS / 64;
constexpr int GEO_MAX_GRID = 4096;       // workgroups (they stride over the points)

static_assert(sizeof(SnerfGeoParams) == 48, "snerf_amd/_lib.py mirrors this layout");

// the two UTM series (latlon_to_utm, utm_to_latlon) and their constants live in geo_dev.h: orthorect.hip evaluates the inverse too

constexpr unsigned long long KEY_MIN_IDENTITY = ~0ull;   // what the host writes into the two minimum words
constexpr unsigned long long KEY_MAX_IDENTITY = 0ull;    // ... and into the two maximum words

// The bounds of a launch's output, shared by both directions: every thread offers its points' first two components (east /
// north, or scene x / y), then finish() folds them per wave, per workgroup and into the caller's stats words.
struct GeoFold {
  unsigned long long k_amin = KEY_MIN_IDENTITY, k_amax = KEY_MAX_IDENTITY, k_bmin = KEY_MIN_IDENTITY, k_bmax = KEY_MAX_IDENTITY;
  unsigned int bad = 0;

  __device__ __forceinline__ void add(double a, double b, double c) {
    if (__builtin_isfinite(a) && __builtin_isfinite(b) && __builtin_isfinite(c)) {
      const unsigned long long ka = order_key(a), kb = order_key(b);
      k_amin = OpMin()(k_amin, ka);
      k_amax = OpMax()(k_amax, ka);
      k_bmin = OpMin()(k_bmin, kb);
      k_bmax = OpMax()(k_bmax, kb);
    } else {
      ++bad;
    }
  }

  // every thread of the workgroup calls this once, after its loop has ended
  __device__ __forceinline__ void finish(unsigned long long* __restrict__ stats) {
    __shared__ unsigned long long red[4][GEO_WAVES];
    __shared__ unsigned int red_bad[GEO_WAVES];
    // wave64 butterflies (every lane takes part: the loop has ended for the whole wave)
    k_amin = wave_reduce(k_amin, OpMin());
    k_amax = wave_reduce(k_amax, OpMax());
    k_bmin = wave_reduce(k_bmin, OpMin());
    k_bmax = wave_reduce(k_bmax, OpMax());
    bad = wave_reduce(bad, OpSum());
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
      red[0][wave] = k_amin;
      red[1][wave] = k_amax;
      red[2][wave] = k_bmin;
      red[3][wave] = k_bmax;
      red_bad[wave] = bad;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
      for (int w = 1; w < GEO_WAVES; ++w) {
        k_amin = OpMin()(k_amin, red[0][w]);
        k_amax = OpMax()(k_amax, red[1][w]);
        k_bmin = OpMin()(k_bmin, red[2][w]);
        k_bmax = OpMax()(k_bmax, red[3][w]);
        bad += red_bad[w];
      }
      // a workgroup without a finite point holds the identities: nothing to fold
      if (k_amin != KEY_MIN_IDENTITY) {
        atomicMin(&stats[0], k_amin);
        atomicMax(&stats[1], k_amax);
        atomicMin(&stats[2], k_bmin);
        atomicMax(&stats[3], k_bmax);
      }
      if (bad) atomicAdd(&stats[4], (unsigned long long)bad);
    }
  }
};

// direction 0, scene -> world.  rays != nullptr: step 1 (end points from the rays) first; else the points come in as xyz_n
__global__ __launch_bounds__(GEO_THREADS) void geo_cloud_kernel(const float* __restrict__ rays, int ray_stride,
                                                                const float* __restrict__ depth, const double* __restrict__ xyz_n,
                                                                long long n, SnerfGeoParams p, double* __restrict__ enu_out,
                                                                double* __restrict__ lla_out, unsigned long long* __restrict__ stats) {
  GeoFold fold;
  for (long long i = (long long)blockIdx.x * GEO_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * GEO_THREADS) {
    double q[3];
    if (rays != nullptr) {
      // 1. rays.double(): o + d * depth, one rounding for the product and one for the sum
      const float* r = rays + i * ray_stride;
      const double dep = (double)depth[i];
#pragma unroll
      for (int k = 0; k < 3; ++k) q[k] = __dadd_rn((double)r[k], __dmul_rn((double)r[3 + k], dep));
    } else {
#pragma unroll
      for (int k = 0; k < 3; ++k) q[k] = xyz_n[3 * i + k];
    }
    // 2. denormalize: xyz * range + centre, two roundings per component
    double x[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) x[k] = __dadd_rn(__dmul_rn(q[k], p.range), p.centre[k]);
    // 3. custom ECEF -> geodetic (degrees), 4. -> UTM
    double lat, lon, alt, east, north;
    ecef_to_latlon(x[0], x[1], x[2], &lat, &lon, &alt);
    latlon_to_utm(lat, lon, p.lon0, p.south, &east, &north);
    double* e = enu_out + 3 * i;
    e[0] = east;
    e[1] = north;
    e[2] = alt;
    if (lla_out != nullptr) {
      double* l = lla_out + 3 * i;
      l[0] = lat;
      l[1] = lon;
      l[2] = alt;
    }
    fold.add(east, north, alt);
  }
  fold.finish(stats);
}

// direction 1, world -> scene: enu (n, 3) (east, north, alt) -> lat / lon (utm.to_latlon) -> custom ECEF -> normalised points
__global__ __launch_bounds__(GEO_THREADS) void geo_scene_kernel(const double* __restrict__ enu, long long n, SnerfGeoParams p,
                                                                double* __restrict__ xyz_out, double* __restrict__ lla_out,
                                                                unsigned long long* __restrict__ stats) {
  GeoFold fold;
  for (long long i = (long long)blockIdx.x * GEO_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * GEO_THREADS) {
    const double east = enu[3 * i], north = enu[3 * i + 1], alt = enu[3 * i + 2];
    double lat, lon, x[3];
    utm_to_latlon(east, north, p.lon0, p.south, &lat, &lon);
    latlon_to_ecef(lat, lon, alt, &x[0], &x[1], &x[2]);
    // normalize: (xyz - centre) / range, two roundings per component (the inverse of denormalize on an fp64 tensor)
    double q[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) q[k] = __ddiv_rn(__dsub_rn(x[k], p.centre[k]), p.range);
    double* o = xyz_out + 3 * i;
    o[0] = q[0];
    o[1] = q[1];
    o[2] = q[2];
    if (lla_out != nullptr) {
      double* l = lla_out + 3 * i;
      l[0] = lat;
      l[1] = lon;
      l[2] = alt;
    }
    fold.add(q[0], q[1], q[2]);
  }
  fold.finish(stats);
}

static int geo_launch(const char* who, const float* rays, int ray_stride, const float* depth, const double* xyz_n, long long n,
                      const SnerfGeoParams* params, double* enu_out, double* lla_out, unsigned long long* stats, void* stream) {
  if (!params || !stats) { set_error("%s: null pointer", who); return SNERF_ERR_NULL; }
  if (n < 0 || n > (long long)1 << 31) { set_error("%s: n = %lld outside [0, 2^31]", who, n); return SNERF_ERR_BAD_DESC; }
  if (!(params->range > 0.0) || !__builtin_isfinite(params->range)) { set_error("%s: range must be positive and finite", who); return SNERF_ERR_BAD_DESC; }
  for (int k = 0; k < 3; ++k)
    if (!__builtin_isfinite(params->centre[k])) { set_error("%s: centre[%d] is not finite", who, k); return SNERF_ERR_BAD_DESC; }
  if (!(params->lon0 >= -M_PI && params->lon0 <= M_PI)) { set_error("%s: central meridian %g rad outside [-pi, pi]", who, params->lon0); return SNERF_ERR_BAD_DESC; }
  if (params->south != 0 && params->south != 1) { set_error("%s: south = %d", who, params->south); return SNERF_ERR_BAD_DESC; }
  // world -> scene starts from points: only snerf_geo_points (rays == nullptr) offers it
  if (params->direction != SNERF_GEO_TO_WORLD && (params->direction != SNERF_GEO_TO_SCENE || rays != nullptr)) {
    set_error("%s: direction = %d", who, params->direction);
    return SNERF_ERR_BAD_DESC;
  }
  if (n == 0) return SNERF_OK;
  if (!enu_out) { set_error("%s: null pointer", who); return SNERF_ERR_NULL; }
  const dim3 grid(blocks_for(n, GEO_THREADS, GEO_MAX_GRID)), block(GEO_THREADS);
  if (params->direction == SNERF_GEO_TO_SCENE)
    hipLaunchKernelGGL(geo_scene_kernel, grid, block, 0, (hipStream_t)stream, xyz_n, n, *params, enu_out, lla_out, stats);
  else
    hipLaunchKernelGGL(geo_cloud_kernel, grid, block, 0, (hipStream_t)stream, rays, ray_stride, depth, xyz_n, n, *params, enu_out,
                       lla_out, stats);
  SNERF_LAUNCH_CHECK();
  return SNERF_OK;
}

}  // namespace snerf

using namespace snerf;

extern "C" int snerf_geo_cloud(const float* rays, int ray_stride, const float* depth, long long n, const SnerfGeoParams* params,
                               double* enu_out, double* lla_out, unsigned long long* stats, void* stream) {
  const char* who = "snerf_geo_cloud";
  if (ray_stride < 6) { set_error("%s: ray_stride %d < 6", who, ray_stride); return SNERF_ERR_BAD_DESC; }
  if (n > 0 && (!rays || !depth)) { set_error("%s: null pointer", who); return SNERF_ERR_NULL; }
  return geo_launch(who, rays, ray_stride, depth, nullptr, n, params, enu_out, lla_out, stats, stream);
}

extern "C" int snerf_geo_points(const double* xyz_n, long long n, const SnerfGeoParams* params, double* enu_out, double* lla_out,
                                unsigned long long* stats, void* stream) {
  const char* who = "snerf_geo_points";
  if (n > 0 && !xyz_n) { set_error("%s: null pointer", who); return SNERF_ERR_NULL; }
  return geo_launch(who, nullptr, 0, nullptr, xyz_n, n, params, enu_out, lla_out, stats, stream);
}
