// The distortion loss on a ray's weights (mip-NeRF 360's regulariser), value and d / d weights in one launch and O(S) per ray.
// The spec is stated at snerf_ray_distortion in include/snerf_hip.h and in DESIGN.md section 5r; tests/raydist_numpy.py
// restates it operation for operation.
//   - every floating-point operation is fp64 and rounded on its own (no fused multiply-adds in this file: plain operators under
//     `fp contract(off)`, see the note in shadow.hip), and every sum is over int64 masses: the result has no summation order, so
//     it does not depend on how the scan is spread over the lanes and equals numpy's bit for bit;
//   - one wave64 per ray, up to four rays per workgroup (ray_wave.h); a ray's midpoints m and the exclusive prefixes A, B of its masses live in
//     LDS (24 S bytes, 24 KB at the 1024-sample limit; the host lowers the rays per workgroup so that a workgroup stays within
//     64 KB);
//   - the scan: a lane sums a run of consecutive masses, the run totals are scanned across the wave (wave_scan_i64, once per sequence),
//     the lane writes its run's prefixes;
//   - wave barriers only: a ragged last workgroup retires its idle waves at once;
//   - a ray's integer sums are reduced in the wave and lane 0 adds them to the caller's accumulator words with integer atomics;
//   - vector loads and stores only, one launch, no allocation, no copy and no host synchronisation.
#include "ray_wave.h"
#include "../../include/snerf_hip.h"

#pragma clang fp contract(off)

namespace snerf {

constexpr int RAYDIST_MAX_RAYS = 1 << 22;
constexpr double RAYDIST_Q = 1125899906842624.0;           // 2^50
constexpr double RAYDIST_ACC_SCALE = 1099511627776.0;      // 2^40
constexpr double RAYDIST_TWO_THIRDS = 2.0 / 3.0;

static inline size_t raydist_ray_bytes(int S) { return 24 * (size_t)S; }

// w' = min(max((double)w, 0), 1); a zero of either sign gives +0 (the ray is bad when w is not finite: never reached with a NaN)
__device__ __forceinline__ double raydist_clamp(float w) {
  const double wd = (double)w;
  return wd > 0.0 ? (wd > 1.0 ? 1.0 : wd) : 0.0;
}

__global__ __launch_bounds__(RAY_WAVE * RAY_WAVE_MAX_RAYS_PER_BLOCK) void ray_distortion_kernel(
    const float* __restrict__ weights, const float* __restrict__ z_vals, const float* __restrict__ rays, int ray_stride, int n_rays,
    int S, float* __restrict__ d_weights, double* __restrict__ per_ray, unsigned long long* __restrict__ acc, int ray_bytes) {
  extern __shared__ __attribute__((aligned(16))) unsigned char raydist_lds[];
  const auto [lane, wave, ray] = ray_wave_id();
  if (ray >= n_rays) return;                                   // wave-uniform: see ray_wave.h
  double* m = reinterpret_cast<double*>(raydist_lds + (size_t)wave * ray_bytes);       // [S] midpoints
  long long* A = reinterpret_cast<long long*>(m + S);                                  // [S] exclusive prefixes of a
  long long* B = A + S;                                                                // [S] exclusive prefixes of b
  const float* wr = weights + ray * S;
  const float* zr = z_vals + ray * S;
  float* gr = d_weights + ray * S;
  const float near_f = rays[ray * ray_stride + 6], far_f = rays[ray * ray_stride + 7];
  const double near = (double)near_f, span = (double)far_f - (double)near_f;

  // 1. / 6. the midpoints, and whether the ray is bad
  bool bad = !(__builtin_isfinite(near_f) && __builtin_isfinite(far_f) && far_f > near_f);
  for (int i = lane; i < S; i += RAY_WAVE) {
    const float w = wr[i], z0 = zr[i];
    const double t0 = ((double)z0 - near) / span;
    double delta = 0.0;
    bad = bad || !__builtin_isfinite(w) || !__builtin_isfinite(z0) || !(t0 >= -1.0 && t0 <= 2.0);
    if (i < S - 1) {
      const float z1 = zr[i + 1];
      bad = bad || z1 < z0;
      delta = ((double)z1 - near) / span - t0;
    }
    const double half = 0.5 * delta;
    m[i] = t0 + half;
  }
  if (__builtin_amdgcn_ballot_w64(bad) != 0ull) {               // wave-uniform from here on
    for (int i = lane; i < S; i += RAY_WAVE) gr[i] = 0.f;
    if (lane == 0) {
      if (per_ray) per_ray[ray] = __builtin_nan("");
      atomicAdd(&acc[1], 1ull);
      atomicAdd(&acc[2], 1ull);
    }
    return;
  }
  ray_wave_sync();

  // 2. / 3. the masses and their exclusive prefixes: lane l owns the samples [l * per, l * per + per)
  const int per = (S + RAY_WAVE - 1) / RAY_WAVE, j0 = lane * per;
  long long run_a = 0, run_b = 0;
  for (int j = j0; j < j0 + per && j < S; ++j) {
    const double wc = raydist_clamp(wr[j]);
    const double wm = wc * m[j];
    run_a += llrint(wc * RAYDIST_Q);
    run_b += llrint(wm * RAYDIST_Q);
  }
  long long AT, BT;
  long long pa = wave_scan_i64(run_a, lane, &AT), pb = wave_scan_i64(run_b, lane, &BT);     // the masses before this lane's run
  for (int j = j0; j < j0 + per && j < S; ++j) {
    const double wc = raydist_clamp(wr[j]);
    const double wm = wc * m[j];
    A[j] = pa;
    B[j] = pb;
    pa += llrint(wc * RAYDIST_Q);
    pb += llrint(wm * RAYDIST_Q);
  }
  ray_wave_sync();

  // 4. / 5. the per-sample terms and the gradient
  unsigned long long qsum = 0ull;                               // two's complement: the sum of the spec's int64 q
  for (int i = lane; i < S; i += RAY_WAVE) {
    const float w = wr[i];
    const double wc = raydist_clamp(w);
    const double mi = m[i];
    double delta = 0.0;
    if (i < S - 1) {
      const double t0 = ((double)zr[i] - near) / span;
      delta = ((double)zr[i + 1] - near) / span - t0;
    }
    const long long Ai = A[i], Bi = B[i];
    const long long ai = llrint(wc * RAYDIST_Q);
    const double wm = wc * mi;
    const long long bi = llrint(wm * RAYDIST_Q);
    const double Ab = (double)Ai / RAYDIST_Q, Bb = (double)Bi / RAYDIST_Q;
    const double Ap = (double)(AT - Ai - ai) / RAYDIST_Q, Bp = (double)(BT - Bi - bi) / RAYDIST_Q;
    const double mA = mi * Ab;
    const double x = mA - Bb;                                   // the mass in front of sample i, times its distance
    const double wx = wc * x;
    const double ww = wc * wc;
    const double wwd = ww * delta;
    const double third = wwd / 3.0;
    const double e = 2.0 * wx + third;
    qsum += (unsigned long long)llrint(e * RAYDIST_Q);
    const double mAp = mi * Ap;
    const double y = Bp - mAp;                                  // the mass behind it, times its distance
    const double xy = x + y;
    const double c = RAYDIST_TWO_THIRDS * wc;
    const double cd = c * delta;
    const double g = 2.0 * xy + cd;
    gr[i] = (w < 0.f || w > 1.f) ? 0.f : (float)g;
  }
#pragma unroll
  for (int o = RAY_WAVE / 2; o > 0; o >>= 1) qsum += __shfl_xor(qsum, o, RAY_WAVE);
  if (lane == 0) {
    const double Lr = (double)(long long)qsum / RAYDIST_Q;
    if (per_ray) per_ray[ray] = Lr;
    atomicAdd(&acc[0], (unsigned long long)llrint(Lr * RAYDIST_ACC_SCALE));
    atomicAdd(&acc[1], 1ull);
  }
}

}  // namespace snerf

using namespace snerf;

extern "C" int snerf_ray_distortion(const float* weights, const float* z_vals, const float* rays, int ray_stride, int n_rays,
                                    int n_samples, float* d_weights, double* per_ray, unsigned long long* acc, void* stream) {
  if (!weights) { set_error("snerf_ray_distortion: weights is NULL"); return SNERF_ERR_NULL; }
  if (!z_vals) { set_error("snerf_ray_distortion: z_vals is NULL"); return SNERF_ERR_NULL; }
  if (!rays) { set_error("snerf_ray_distortion: rays is NULL"); return SNERF_ERR_NULL; }
  if (!d_weights) { set_error("snerf_ray_distortion: d_weights is NULL"); return SNERF_ERR_NULL; }
  if (!acc) { set_error("snerf_ray_distortion: acc is NULL"); return SNERF_ERR_NULL; }
  if (n_rays < 1 || n_rays > RAYDIST_MAX_RAYS) {
    set_error("snerf_ray_distortion: n_rays = %d must be in [1, %d]", n_rays, RAYDIST_MAX_RAYS);
    return SNERF_ERR_BAD_DESC;
  }
  if (n_samples < 1 || n_samples > SNERF_VIS_MAX_SAMPLES) {
    set_error("snerf_ray_distortion: n_samples = %d must be in [1, %d]", n_samples, SNERF_VIS_MAX_SAMPLES);
    return SNERF_ERR_BAD_DESC;
  }
  if (ray_stride < 8) {
    set_error("snerf_ray_distortion: ray_stride = %d must be >= 8 (near and far are columns 6 and 7)", ray_stride);
    return SNERF_ERR_BAD_DESC;
  }
  const size_t ray_bytes = raydist_ray_bytes(n_samples);                         // <= 24 KB: at least 2 rays fit
  const RayWaveLaunch l = ray_wave_launch(n_rays, ray_bytes);
  hipLaunchKernelGGL(ray_distortion_kernel, l.grid, l.block, l.lds_bytes, (hipStream_t)stream,
                     weights, z_vals, rays, ray_stride, n_rays, n_samples, d_weights, per_ray, acc, (int)ray_bytes);
  SNERF_LAUNCH_CHECK();
  return SNERF_OK;
}
