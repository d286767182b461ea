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

// the utm package's constants (utm/conversion.py), evaluated in its order
constexpr double UTM_K0 = 0.9996;
constexpr double UTM_E = 0.00669438;
constexpr double UTM_E2 = UTM_E * UTM_E;
constexpr double UTM_E3 = UTM_E2 * UTM_E;
constexpr double UTM_E_P2 = UTM_E / (1.0 - UTM_E);
constexpr double UTM_R = 6378137.0;
constexpr double UTM_M1 = 1.0 - UTM_E / 4.0 - 3.0 * UTM_E2 / 64.0 - 5.0 * UTM_E3 / 256.0;
constexpr double UTM_M2 = 3.0 * UTM_E / 8.0 + 3.0 * UTM_E2 / 32.0 + 45.0 * UTM_E3 / 1024.0;
constexpr double UTM_M3 = 15.0 * UTM_E2 / 256.0 + 45.0 * UTM_E3 / 1024.0;
constexpr double UTM_M4 = 35.0 * UTM_E3 / 3072.0;

// utm's mod_angle: (v + pi) % (2 pi) - pi with Python's sign rule for %, into [-pi, pi)
__device__ __forceinline__ double utm_wrap(double v) {
  const double two_pi = 2.0 * M_PI;
  double r = fmod(v + M_PI, two_pi);
  if (r != 0.0 && r < 0.0) r += two_pi;
  return r - M_PI;
}

// utm.from_latlon's series for a point at (lat, lon) in degrees in the zone of central meridian lon0 (radians)
__device__ __forceinline__ void latlon_to_utm(double lat, double lon, double lon0, int south, double* east, double* north) {
  const double lat_rad = lat * (M_PI / 180.0);
  const double lon_rad = lon * (M_PI / 180.0);
  const double ls = sin(lat_rad), lc = cos(lat_rad);
  const double t = ls / lc;
  const double t2 = t * t;
  const double t4 = t2 * t2;
  const double n = UTM_R / sqrt(1.0 - UTM_E * (ls * ls));
  const double c = UTM_E_P2 * (lc * lc);
  const double a = lc * utm_wrap(lon_rad - lon0);
  const double a2 = a * a;
  const double a3 = a2 * a;
  const double a4 = a3 * a;
  const double a5 = a4 * a;
  const double a6 = a5 * a;
  const double m = UTM_R * (UTM_M1 * lat_rad - UTM_M2 * sin(2.0 * lat_rad) + UTM_M3 * sin(4.0 * lat_rad) - UTM_M4 * sin(6.0 * lat_rad));
  *east = UTM_K0 * n * (a + a3 / 6.0 * (1.0 - t2 + c) + a5 / 120.0 * (5.0 - 18.0 * t2 + t4 + 72.0 * c - 58.0 * UTM_E_P2)) + 500000.0;
  double nn = UTM_K0 * (m + n * t * (a2 / 2.0 + a4 / 24.0 * (5.0 - t2 + 9.0 * c + 4.0 * (c * c)) +
                                     a6 / 720.0 * (61.0 - 58.0 * t2 + t4 + 600.0 * c - 330.0 * UTM_E_P2)));
  if (south) nn += 10000000.0;
  *north = nn;
}

// utm.to_latlon's constants: _E = (1 - sqrt(1 - E)) / (1 + sqrt(1 - E)) and the footpoint-latitude coefficients P2 .. P5.
// UTM_SQRT_1ME is the double nearest sqrt(1 - E) (sqrt is not a constant expression); the rest is evaluated in the package's order
constexpr double UTM_SQRT_1ME = 0.9966471893303066;
static_assert(UTM_SQRT_1ME * UTM_SQRT_1ME > (1.0 - UTM_E) * (1.0 - 1e-15) && UTM_SQRT_1ME * UTM_SQRT_1ME < (1.0 - UTM_E) * (1.0 + 1e-15),
              "UTM_SQRT_1ME is sqrt(1 - UTM_E)");
constexpr double UTM_E1 = (1.0 - UTM_SQRT_1ME) / (1.0 + UTM_SQRT_1ME);
constexpr double UTM_E1_2 = UTM_E1 * UTM_E1;
constexpr double UTM_E1_3 = UTM_E1_2 * UTM_E1;
constexpr double UTM_E1_4 = UTM_E1_3 * UTM_E1;
constexpr double UTM_E1_5 = UTM_E1_4 * UTM_E1;
constexpr double UTM_P2 = 3.0 / 2.0 * UTM_E1 - 27.0 / 32.0 * UTM_E1_3 + 269.0 / 512.0 * UTM_E1_5;
constexpr double UTM_P3 = 21.0 / 16.0 * UTM_E1_2 - 55.0 / 32.0 * UTM_E1_4;
constexpr double UTM_P4 = 151.0 / 96.0 * UTM_E1_3 - 417.0 / 128.0 * UTM_E1_5;
constexpr double UTM_P5 = 1097.0 / 512.0 * UTM_E1_4;

// utm.to_latlon's series for a point at (east, north) metres in the zone of central meridian lon0 (radians) -> degrees
__device__ __forceinline__ void utm_to_latlon(double east, double north, double lon0, int south, double* lat, double* lon) {
  const double x = east - 500000.0;
  double y = north;
  if (south) y -= 10000000.0;
  const double m = y / UTM_K0;
  const double mu = m / (UTM_R * UTM_M1);
  const double p = mu + UTM_P2 * sin(2.0 * mu) + UTM_P3 * sin(4.0 * mu) + UTM_P4 * sin(6.0 * mu) + UTM_P5 * sin(8.0 * mu);
  const double ps = sin(p), pc = cos(p);
  const double pt = ps / pc;
  const double pt2 = pt * pt;
  const double pt4 = pt2 * pt2;
  const double eps = 1.0 - UTM_E * (ps * ps);
  const double n = UTM_R / sqrt(eps);
  const double r = (1.0 - UTM_E) / eps;
  const double c = UTM_E_P2 * (pc * pc);
  const double c2 = c * c;
  const double d = x / (n * UTM_K0);
  const double d2 = d * d;
  const double d3 = d2 * d;
  const double d4 = d3 * d;
  const double d5 = d4 * d;
  const double d6 = d5 * d;
  // the d^6 term stands outside the bracket that pt / r multiplies, as in the package
  const double lat_rad = p - (pt / r) * (d2 / 2.0 - d4 / 24.0 * (5.0 + 3.0 * pt2 + 10.0 * c - 4.0 * c2 - 9.0 * UTM_E_P2)) +
                         d6 / 720.0 * (61.0 + 90.0 * pt2 + 298.0 * c + 45.0 * pt4 - 252.0 * UTM_E_P2 - 3.0 * c2);
  const double lon_rad = (d - d3 / 6.0 * (1.0 + 2.0 * pt2 + c) +
                          d5 / 120.0 * (5.0 - 2.0 * c + 28.0 * pt2 - 3.0 * c2 + 8.0 * UTM_E_P2 + 24.0 * pt4)) / pc;
  *lat = lat_rad * (180.0 / M_PI);
  *lon = utm_wrap(lon_rad + lon0) * (180.0 / M_PI);
}

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
