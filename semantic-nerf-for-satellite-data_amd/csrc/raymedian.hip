// The median depth of a ray: the depth at which half of the ray's weight lies in front (SNERF_FLAG_DEPTH_MEDIAN).  One launch behind
// an inference pass's composite, O(S) per ray.  The spec is stated at the flag in include/snerf_hip.h and in DESIGN.md section 5s;
// tests/raymedian_numpy.py restates it operation for operation.
//   - every floating-point operation is fp64 and rounded on its own (no fused multiply-adds in this file: plain operators under
//     `fp contract(off)`, see the note in shadow.hip), and every sum is over int64 masses: the result has no summation order, so
//     it does not depend on how the runs are spread over the lanes and equals numpy's bit for bit;
//   - one wave64 per ray, up to four rays per workgroup (ray_wave.h), NO LDS: a lane sums the run of ceil(S / 64) consecutive
//     masses it owns, the run totals are scanned across the wave (wave_scan_i64, once), and the ONE lane whose run holds the
//     crossing of half the total walks its run again and stores the ray's depth;
//   - a pass maps a density that is not finite (a ray whose origin or direction is a NaN) to ZERO weights -- the composite takes
//     fmaxf(sigma, 0) -- so such a ray would read as empty; where the caller hands over the sigmas the pass wrote, a sigma that is not
//     finite makes the ray bad like a weight that is not finite (12 instead of 8 bytes read per sample);
//   - wave barriers only (none is needed: nothing is shared but through the shuffles): a ragged last workgroup retires its idle
//     waves at once;
//   - vector loads and stores only, no atomics, one launch, no allocation, no copy and no host synchronisation.
#include "ray_wave.h"
#include "composite.h"
#include "../../include/snerf_hip.h"

#pragma clang fp contract(off)

namespace snerf {

constexpr double RAYMEDIAN_Q = 1125899906842624.0;           // 2^50

// a = llrint(min(max((double)w, 0), 1) * 2^50); a zero of either sign gives +0 (the ray is bad when w is not finite: never used with a NaN)
__device__ __forceinline__ long long raymedian_mass(float w) {
  const double wd = (double)w;
  const double wc = wd > 0.0 ? (wd > 1.0 ? 1.0 : wd) : 0.0;
  return llrint(wc * RAYMEDIAN_Q);
}

__global__ __launch_bounds__(RAY_WAVE * RAY_WAVE_MAX_RAYS_PER_BLOCK) void ray_median_kernel(
    const float* __restrict__ weights, const float* __restrict__ z_vals, const float* __restrict__ sigmas, int n_rays, int S,
    float* __restrict__ depth) {
  const auto [lane, wave, ray] = ray_wave_id();
  if (ray >= n_rays) return;                                   // wave-uniform: see ray_wave.h
  const float* wr = weights + ray * S;
  const float* zr = z_vals + ray * S;
  const float* sr = sigmas ? sigmas + ray * S : nullptr;      // (kernel argument: wave-uniform)

  // 1. - 4. whether the ray is bad, and the masses: lane l owns the samples [l * per, l * per + per)
  const int per = (S + RAY_WAVE - 1) / RAY_WAVE, j0 = lane * per;
  const int j1 = j0 + per < S ? j0 + per : S;                   // (j0 >= S: an empty run)
  bool bad = false;
  long long run = 0;
  for (int j = j0; j < j1; ++j) {
    const float w = wr[j], z0 = zr[j];
    bad = bad || !__builtin_isfinite(w) || !__builtin_isfinite(z0);
    if (j < S - 1) bad = bad || zr[j + 1] < z0;
    if (sr) bad = bad || !__builtin_isfinite(sr[j]);
    run += raymedian_mass(w);
  }
  if (__builtin_amdgcn_ballot_w64(bad) != 0ull) {               // wave-uniform
    if (lane == 0) depth[ray] = __builtin_nanf("");
    return;
  }
  long long AT;
  const long long pa = wave_scan_i64(run, lane, &AT);           // the mass in front of this lane's run; AT <= 2^60
  // 5. nothing on the ray: the far end
  if (AT == 0) {                                                // wave-uniform
    if (lane == 0) depth[ray] = zr[S - 1];
    return;
  }
  // 6. the first j with 2 (A_j + a_j) >= AT lies in the run of the one lane with 2 pa < AT <= 2 (pa + run): the lanes before it
  //    end short of half, the lanes behind it start at or past it (an empty run starts at AT)
  if (!(2 * pa < AT && 2 * (pa + run) >= AT)) return;
  long long A = pa, a = 0;
  int j = j0;
  for (; j < j1; ++j) {
    a = raymedian_mass(wr[j]);
    if (2 * (A + a) >= AT) break;
    A += a;
  }
  // 7. the last interval is open-ended: its mass sits at its near edge
  if (j >= S - 1) {                                             // (j == S - 1; j < j1 <= S always: the run holds the crossing)
    depth[ray] = zr[S - 1];
    return;
  }
  // 8. w_j spread uniformly over [z_j, z_{j+1}]; a tie gives frac = 1
  const double frac = (double)(AT - 2 * A) / (double)(2 * a);
  const double zj = (double)zr[j];
  const double span = (double)zr[j + 1] - zj;
  const double fs = frac * span;
  depth[ray] = (float)(zj + fs);
}

// composite.h.  The caller (snerf_forward) has checked the pointers and S in [1, SNERF_VIS_MAX_SAMPLES]; n_rays * S <= 2^30 (make_plan).
int launch_ray_median(const float* weights, const float* z_vals, const float* sigmas, float* depth, int n_rays, int S, hipStream_t st) {
  const RayWaveLaunch l = ray_wave_launch(n_rays, 0);           // no LDS: four rays per workgroup
  hipLaunchKernelGGL(ray_median_kernel, l.grid, l.block, l.lds_bytes, st, weights, z_vals, sigmas, n_rays, S, depth);
  SNERF_LAUNCH_CHECK();
  return SNERF_OK;
}

}  // namespace snerf
