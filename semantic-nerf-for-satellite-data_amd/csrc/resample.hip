// Importance resampling of the depths (the reference's sample_pdf, framework/components/rendering.py:8-51, and the sort of the
// merged depths its callers do): Ni fine samples per ray from the pdf of the proposal pass's interior weights over the midpoints
// of the coarse depths, merged with the S coarse depths.  The spec is stated at snerf_resample_z in include/snerf_hip.h and in
// DESIGN.md section 5p; tests/resample_numpy.py restates it operation for operation.
//   - every floating-point operation is fp64 and rounded on its own (no fused multiply-adds in this file: plain operators under
//     `fp contract(off)`, see the note in shadow.hip), and the cdf is a prefix sum of int64 masses: the result has no summation
//     order, so it does not depend on how the scan is spread over the lanes and equals numpy's bit for bit;
//   - one wave64 per ray, up to four rays per workgroup (ray_wave.h); a ray's midpoints b, prefix masses P and the S + Ni values to merge
//     live in LDS (16 (S - 1) + 4 (S + Ni) bytes, 20 KB at the 1024-sample limit; the host lowers the rays per workgroup so
//     that a workgroup stays within 64 KB);
//   - the scan: a lane sums a run of consecutive masses, the run totals are scanned across the wave (wave_scan_i64), the lane
//     writes its run's prefixes;
//   - a fine sample is one binary search over P; the merge position of an element is its rank among the S + Ni values, ties
//     broken by the position in concatenate([z, fine]) -- numpy's stable argsort -- counted against the values in LDS (every lane
//     reads the same word: a broadcast).  A rank is at most S + Ni - 1 whatever the values are, so no store leaves the ray's row;
//   - vector loads and stores only, no atomics, one launch, no allocation, no copy and no host synchronisation.
#include "ray_wave.h"
#include "../../include/snerf_hip.h"

#pragma clang fp contract(off)

namespace snerf {

constexpr double RESAMPLE_EPS = 1e-5;
constexpr double RESAMPLE_SCALE = 1125899906842624.0;      // 2^50

static inline size_t resample_ray_bytes(int S, int Ni) { return 16 * (size_t)(S - 1) + round_up_sz(4 * (size_t)(S + Ni), 8); }

// the mass of interior weight w: llrint((w' + 1e-5) * 2^50), w' = w where finite and > 0, else 0, at most 1
__device__ __forceinline__ long long resample_mass(float w) {
  double wd = (__builtin_isfinite(w) && w > 0.f) ? (double)w : 0.0;
  wd = wd > 1.0 ? 1.0 : wd;
  return llrint((wd + RESAMPLE_EPS) * RESAMPLE_SCALE);
}

__global__ __launch_bounds__(RAY_WAVE * RAY_WAVE_MAX_RAYS_PER_BLOCK) void resample_z_kernel(
    const float* __restrict__ z, const float* __restrict__ weights, const float* __restrict__ u, float* __restrict__ z_out,
    float* __restrict__ z_fine, int n_rays, int S, int Ni, int ray_bytes) {
  extern __shared__ __attribute__((aligned(16))) unsigned char resample_lds[];
  const auto [lane, wave, ray] = ray_wave_id();
  if (ray >= n_rays) return;                                   // wave-uniform: see ray_wave.h
  const int nb = S - 1, nm = S - 2, St = S + Ni;
  double* b = reinterpret_cast<double*>(resample_lds + (size_t)wave * ray_bytes);      // [nb] midpoints
  long long* P = reinterpret_cast<long long*>(b + nb);                                 // [nb] P[0] = 0 ... P[nm] = T
  float* v = reinterpret_cast<float*>(P + nb);                                         // [St] concatenate([z, fine])
  const float* zr = z + ray * S;
  const float* wr = weights + ray * S;

  // 1. the coarse depths and their midpoints
  for (int j = lane; j < S; j += RAY_WAVE) {
    const float z0 = zr[j];
    v[j] = z0;
    if (j < nb) b[j] = 0.5 * ((double)z0 + (double)zr[j + 1]);
  }
  // 2./3. masses and their prefix sums: lane l owns the masses [l * per, l * per + per)
  const int per = (nm + RAY_WAVE - 1) / RAY_WAVE, j0 = lane * per;
  long long run = 0;
  for (int j = j0; j < j0 + per && j < nm; ++j) run += resample_mass(wr[j + 1]);
  long long acc = wave_scan_i64(run, lane, nullptr);            // the masses before this lane's run
  if (lane == 0) P[0] = 0;
  for (int j = j0; j < j0 + per && j < nm; ++j) {
    acc += resample_mass(wr[j + 1]);
    P[j + 1] = acc;
  }
  ray_wave_sync();
  const double T = (double)P[nm];

  // 4.-6. the fine samples
  for (int i = lane; i < Ni; i += RAY_WAVE) {
    double ui;
    if (u) {
      const double g = (double)u[ray * Ni + i];
      ui = g > 0.0 ? (g > 1.0 ? 1.0 : g) : 0.0;                 // NaN -> 0
    } else {
      ui = Ni > 1 ? (double)i / (double)(Ni - 1) : 0.0;
    }
    const double t = ui * T;
    int lo = 0, hi = nm - 1;                                    // the largest k in [0, S - 3] with (double)P[k] <= t
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if ((double)P[mid] <= t) lo = mid; else hi = mid - 1;
    }
    const long long p0 = P[lo];
    const double f = (t - (double)p0) / (double)(P[lo + 1] - p0);
    const double b0 = b[lo];
    const double span = b[lo + 1] - b0;
    const double step = f * span;
    const float fine = (float)(b0 + step);
    v[S + i] = fine;
    if (z_fine) z_fine[ray * Ni + i] = fine;
  }
  ray_wave_sync();

  // 7. the stable merge: element e goes to #{values below it} + #{equal values before it}
  float* out = z_out + ray * St;
  for (int e = lane; e < St; e += RAY_WAVE) {
    const float x = v[e];
    int rank = 0;
    for (int q = 0; q < St; ++q) {
      const float y = v[q];
      rank += (y < x || (y == x && q < e)) ? 1 : 0;
    }
    out[rank] = x;
  }
}

}  // namespace snerf

using namespace snerf;

extern "C" int snerf_resample_z(const float* z, const float* weights, const float* u, float* z_out, float* z_fine, int n_rays,
                                int n_samples, int n_importance, void* stream) {
  if (!z) { set_error("snerf_resample_z: z is NULL"); return SNERF_ERR_NULL; }
  if (!weights) { set_error("snerf_resample_z: weights is NULL"); return SNERF_ERR_NULL; }
  if (!z_out) { set_error("snerf_resample_z: z_out is NULL"); return SNERF_ERR_NULL; }
  if (n_rays < 1) { set_error("snerf_resample_z: n_rays = %d must be >= 1", n_rays); return SNERF_ERR_BAD_DESC; }
  if (n_samples < 3) {
    set_error("snerf_resample_z: n_samples = %d must be >= 3 (the pdf is over the interior weights)", n_samples);
    return SNERF_ERR_BAD_DESC;
  }
  if (n_importance < 1) { set_error("snerf_resample_z: n_importance = %d must be >= 1", n_importance); return SNERF_ERR_BAD_DESC; }
  if ((long long)n_samples + n_importance > SNERF_VIS_MAX_SAMPLES) {
    set_error("snerf_resample_z: n_samples + n_importance = %lld exceeds %d", (long long)n_samples + n_importance, SNERF_VIS_MAX_SAMPLES);
    return SNERF_ERR_BAD_DESC;
  }
  const size_t ray_bytes = resample_ray_bytes(n_samples, n_importance);          // <= 16 * 1022 + 4096: at least 3 rays fit
  const RayWaveLaunch l = ray_wave_launch(n_rays, ray_bytes);
  hipLaunchKernelGGL(resample_z_kernel, l.grid, l.block, l.lds_bytes, (hipStream_t)stream,
                     z, weights, u, z_out, z_fine, n_rays, n_samples, n_importance, (int)ray_bytes);
  SNERF_LAUNCH_CHECK();
  return SNERF_OK;
}
