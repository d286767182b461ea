// Per-image visualisation maps on the device (snerf_amd/eval/utils/vismaps.py, framework/visualize.py; the reference's
// framework/visualize.py, baseline/components/visualize.py, semantic/components/visualize.py and framework/util/other.py
// visualize_image_numpy).  The spec is stated in include/snerf_hip.h.
//   vis_fold_kernel: one wave per ray.  The ray's weights row goes to LDS once; every per-sample tensor of the ray is then read
//     once as one flat contiguous row (lane l on floats l, l + 64, ...), each fp32 product w * f is rounded to fp32, widened and
//     accumulated in fp64 per lane in ascending element order, and the 64 lane sums meet in a fixed xor butterfly (fp64 addition
//     commutes, so every lane ends with the same bits).  The order depends on S alone: a ray gives the same bits wherever it sits.
//     The per-ray products (differences, palette lookups, the label error) are computed wave-uniformly and stored by lane 0.
//     Minimum and maximum of the scalar planes stay in registers over the wave's rays, meet in LDS per workgroup and enter the
//     stats block as one integer atomic max per workgroup, slot and bound on order-preserving keys: exact, order-independent.
//   vis_minmax_kernel: the same bounds of a plane that was not made by the fold (the fp64 altitude plane).
//   vis_colormap_kernel: nan_to_num, normalise by the bounds, * 255, truncate, look up a (256, 3) table held in LDS.
// No float atomics, no allocation, no synchronisation; everything on the caller's stream.
#include "reduce.h"
#include "../../include/snerf_hip.h"

#include <float.h>
#include <stdint.h>

namespace snerf {

constexpr int VIS_WAVE = 64;
constexpr int VIS_WAVES = 4;                         // rays per workgroup and iteration
constexpr int VIS_THREADS = VIS_WAVE * VIS_WAVES;
constexpr int VIS_MAX_GRID = 4096;
constexpr int VIS_EW_THREADS = 256;                  // element-wise kernels (bounds of a plane, colormap)
constexpr int VIS_EW_MAX_GRID = 2048;
constexpr int VIS_FOLD_SLOTS = 6;                    // depth, sun, beta, beta_semantic, rgb_diff_distance, sem_error

static_assert(SNERF_VIS_SLOT_SEM_ERROR + 1 == VIS_FOLD_SLOTS && VIS_FOLD_SLOTS <= SNERF_VIS_SLOTS, "slot numbering");

// the order-preserving key (reduce.h) of a double that is not NaN, with -0.0 -> +0.0
__device__ __forceinline__ unsigned long long vis_key(double v) { return order_key(v + 0.0); }
// numpy.nan_to_num in the plane's own precision
__device__ __forceinline__ float vis_n2n(float x) {
  if (x != x) return 0.0f;
  return x > FLT_MAX ? FLT_MAX : (x < -FLT_MAX ? -FLT_MAX : x);
}
__device__ __forceinline__ double vis_n2n(double x) {
  if (x != x) return 0.0;
  return x > DBL_MAX ? DBL_MAX : (x < -DBL_MAX ? -DBL_MAX : x);
}
// float -> uint8 as a conversion through int32 keeps it: truncate, low eight bits (in [0, 256) plain truncation)
__device__ __forceinline__ unsigned char vis_u8(float v) {
  if (v != v) return 0;
  const float c = v > 2147483520.0f ? 2147483520.0f : (v < -2147483648.0f ? -2147483648.0f : v);
  return (unsigned char)((int)c & 255);
}
__device__ __forceinline__ unsigned char vis_u8(double v) {
  if (v != v) return 0;
  const double c = v > 2147483647.0 ? 2147483647.0 : (v < -2147483648.0 ? -2147483648.0 : v);
  return (unsigned char)((int)c & 255);
}

// sum_s fl32(w_s f_s) of a one-band row: lane l takes samples l, l + 64, ... in ascending order
__device__ __forceinline__ double vis_sum1(const float* __restrict__ f, const float* wl, int S, int lane) {
  double a = 0.0;
  for (int s = lane; s < S; s += VIS_WAVE) a += (double)__fmul_rn(wl[s], f[s]);
  return wave_reduce(a, OpSum());
}

// the three band sums of a (S, 3) row read flat: lane l takes floats l, l + 64, ... ; float e is sample e / 3, band e % 3
__device__ __forceinline__ void vis_sum3(const float* __restrict__ f, const float* wl, int S, int lane, double out[3]) {
  double a0 = 0.0, a1 = 0.0, a2 = 0.0;
  int s = lane / 3, c = lane % 3;                        // 64 = 21 * 3 + 1: a step moves 21 samples and one band on
  for (int e = lane; e < 3 * S; e += VIS_WAVE) {
    const double p = (double)__fmul_rn(wl[s], f[e]);
    a0 += c == 0 ? p : 0.0;
    a1 += c == 1 ? p : 0.0;
    a2 += c == 2 ? p : 0.0;
    s += 21;
    if (++c == 3) { c = 0; ++s; }
  }
  out[0] = wave_reduce(a0, OpSum());
  out[1] = wave_reduce(a1, OpSum());
  out[2] = wave_reduce(a2, OpSum());
}

struct VisBounds {
  double lo, hi;
  __device__ __forceinline__ void add(float v) {
    const double d = (double)vis_n2n(v);
    lo = d < lo ? d : lo;
    hi = d > hi ? d : hi;
  }
};

template <typename L>
__global__ __launch_bounds__(VIS_THREADS) void vis_fold_kernel(SnerfVisIn in, SnerfVisOut out, int m, int S, long long row0,
                                                              long long n, SnerfVisStats* __restrict__ stats) {
  __shared__ float w_lds[VIS_WAVES][SNERF_VIS_MAX_SAMPLES];
  __shared__ double b_lds[VIS_WAVES][VIS_FOLD_SLOTS][2];
  __shared__ unsigned bad_lds[VIS_WAVES];
  const int lane = threadIdx.x % VIS_WAVE, wave = threadIdx.x / VIS_WAVE;
  float* wl = w_lds[wave];
  const L* gt = (const L*)in.semantic_gt;
  VisBounds bd[VIS_FOLD_SLOTS];
#pragma unroll
  for (int k = 0; k < VIS_FOLD_SLOTS; ++k) { bd[k].lo = DBL_MAX; bd[k].hi = -DBL_MAX; }
  unsigned bad = 0;
  for (long long r = (long long)blockIdx.x * VIS_WAVES + wave; r < m; r += (long long)gridDim.x * VIS_WAVES) {
    const long long g = row0 + r;                        // the ray's column of the frame's planes
    float sun = 0.0f;
    if (in.weights) {
      const float* w = in.weights + r * S;
      for (int s = lane; s < S; s += VIS_WAVE) wl[s] = w[s];
      // the wave reads only what it wrote itself, and LDS serves a wave in program order: a wave-scope fence, no barrier
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      if (in.sun) {
        sun = (float)vis_sum1(in.sun + r * S, wl, S, lane);
        if (lane == 0 && out.sun_map) out.sun_map[g] = sun;
        bd[SNERF_VIS_SLOT_SUN].add(sun);
      }
      if (in.beta) {
        const float v = (float)vis_sum1(in.beta + r * S, wl, S, lane);
        if (lane == 0 && out.beta_map) out.beta_map[g] = v;
        bd[SNERF_VIS_SLOT_BETA].add(v);
      }
      if (in.beta_semantic) {
        const float v = (float)vis_sum1(in.beta_semantic + r * S, wl, S, lane);
        if (lane == 0 && out.beta_semantic_map) out.beta_semantic_map[g] = v;
        bd[SNERF_VIS_SLOT_BETA_SEMANTIC].add(v);
      }
      if (in.albedo && out.albedo_map) {
        double a[3];
        vis_sum3(in.albedo + r * S * 3, wl, S, lane, a);
        if (lane < 3) out.albedo_map[lane * n + g] = (float)(lane == 0 ? a[0] : lane == 1 ? a[1] : a[2]);
      }
      if (in.sky && out.sky_map) {
        double a[3];
        vis_sum3(in.sky + r * S * 3, wl, S, lane, a);
        if (lane < 3) out.sky_map[lane * n + g] = (float)(lane == 0 ? a[0] : lane == 1 ? a[1] : a[2]);
      }
    }
    if (in.depth) {
      const float v = in.depth[r];
      if (lane == 0 && out.depth_map) out.depth_map[g] = v;
      bd[SNERF_VIS_SLOT_DEPTH].add(v);
    }
    if (in.rgb && in.rgbs_gt) {
      const float d0 = fabsf(__fsub_rn(in.rgbs_gt[r * 3 + 0], in.rgb[r * 3 + 0]));
      const float d1 = fabsf(__fsub_rn(in.rgbs_gt[r * 3 + 1], in.rgb[r * 3 + 1]));
      const float d2 = fabsf(__fsub_rn(in.rgbs_gt[r * 3 + 2], in.rgb[r * 3 + 2]));
      if (lane < 3 && out.rgb_diff) out.rgb_diff[lane * n + g] = lane == 0 ? d0 : lane == 1 ? d1 : d2;
      const float dist = __fsqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(d0, d0), __fmul_rn(d1, d1)), __fmul_rn(d2, d2)));
      if (lane == 0 && out.rgb_diff_distance) out.rgb_diff_distance[g] = dist;
      bd[SNERF_VIS_SLOT_RGB_DIFF_DISTANCE].add(dist);
    }
    if (in.label) {
      const long long lab = in.label[r];
      if (in.palette) {
        const bool ok = lab >= 0 && lab < in.n_palette;
        if (!ok) ++bad;
        if (lane < 3) {
          const unsigned char c = ok ? in.palette[lab * 3 + lane] : (unsigned char)0;
          if (out.sem_color) out.sem_color[lane * n + g] = c;
          if (out.sem_shaded) out.sem_shaded[lane * n + g] = vis_u8(__fmul_rn((float)c, sun));
        }
      }
      if (gt) {
        const long long d = (long long)gt[r] - lab;
        const float e = d == 0 ? 0.0f : 1.0f;             // clamp(|gt - label|, 0, 1) of integers
        if (lane == 0 && out.sem_error) out.sem_error[g] = e;
        bd[SNERF_VIS_SLOT_SEM_ERROR].add(e);
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");      // the next ray's weights overwrite the row
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < VIS_FOLD_SLOTS; ++k) { b_lds[wave][k][0] = bd[k].lo; b_lds[wave][k][1] = bd[k].hi; }
    bad_lds[wave] = bad;
  }
  __syncthreads();
  const int t = threadIdx.x;
  if (t < VIS_FOLD_SLOTS) {                      // a slot nothing was added to (null input, a wave without rays) kept lo > hi
    double lo = DBL_MAX, hi = -DBL_MAX;
    for (int w = 0; w < VIS_WAVES; ++w) {
      lo = b_lds[w][t][0] < lo ? b_lds[w][t][0] : lo;
      hi = b_lds[w][t][1] > hi ? b_lds[w][t][1] : hi;
    }
    if (lo <= hi) {
      atomicMax(&stats->minmax[t][0], ~vis_key(lo));
      atomicMax(&stats->minmax[t][1], vis_key(hi));
    }
  }
  if (t == VIS_FOLD_SLOTS) {
    unsigned b = 0;
    for (int w = 0; w < VIS_WAVES; ++w) b += bad_lds[w];
    if (b) atomicAdd(&stats->bad_labels, (unsigned long long)b);
  }
}

template <typename T>
__global__ __launch_bounds__(VIS_EW_THREADS) void vis_minmax_kernel(const T* __restrict__ x, long long n, int slot,
                                                                    SnerfVisStats* __restrict__ stats) {
  __shared__ double red[2 * VIS_EW_THREADS];           // the minima, then the maxima
  double lo = DBL_MAX, hi = -DBL_MAX;
  for (long long i = (long long)blockIdx.x * VIS_EW_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * VIS_EW_THREADS) {
    const double v = (double)vis_n2n(x[i]);
    lo = v < lo ? v : lo;
    hi = v > hi ? v : hi;
  }
  const double lh[2] = {lo, hi};
  block_tree<VIS_EW_THREADS, 2>(red, threadIdx.x, lh,
                                [](int k, double a, double b) { return k == 0 ? OpMin()(a, b) : OpMax()(a, b); });
  if (threadIdx.x == 0 && red[0] <= red[VIS_EW_THREADS]) {
    atomicMax(&stats->minmax[slot][0], ~vis_key(red[0]));
    atomicMax(&stats->minmax[slot][1], vis_key(red[VIS_EW_THREADS]));
  }
}

// T = the plane's type: every step in that precision, one rounding per operation, as numpy computes
//   x = nan_to_num(x); x = (x - mi) / (ma - mi + 1e-8); (255 * x).astype(uint8)
// with NEP 50 promotion (numpy >= 2): the Python float 1e-8 takes the array scalars' type, so with the plane's own bounds the
// denominator is fl(fl(ma - mi) + fl(1e-8)) in T; explicit bounds are Python floats: ma - mi + 1e-8 is formed in fp64 and
// rounded once to T, and mi is rounded to T.
template <typename T>
__global__ __launch_bounds__(VIS_EW_THREADS) void vis_colormap_kernel(const T* __restrict__ x, long long n,
                                                                      const SnerfVisStats* __restrict__ stats, int slot,
                                                                      double lo, double hi,
                                                                      const unsigned char* __restrict__ table,
                                                                      unsigned char* __restrict__ out) {
  __shared__ unsigned char tab[256 * 3];
  for (int k = threadIdx.x; k < 256 * 3; k += VIS_EW_THREADS) tab[k] = table[k];
  __syncthreads();
  T mi, den;
  if (slot >= 0) {
    const unsigned long long klo = stats->minmax[slot][0], khi = stats->minmax[slot][1];
    // an untouched slot (no element was folded): bounds 0, 0
    const T a = klo ? (T)order_unkey(~klo) : (T)0, b = khi ? (T)order_unkey(khi) : (T)0;
    mi = a;
    den = (T)(b - a) + (T)1e-8;
  } else {
    mi = (T)lo;
    den = (T)(hi - lo + 1e-8);
  }
  for (long long i = (long long)blockIdx.x * VIS_EW_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * VIS_EW_THREADS) {
    const T q = (T)(vis_n2n(x[i]) - mi) / den;
    const T v = (T)255 * q;
    const int idx = vis_u8(v);
    out[i] = tab[idx * 3 + 0];
    out[n + i] = tab[idx * 3 + 1];
    out[2 * n + i] = tab[idx * 3 + 2];
  }
}

}  // namespace snerf

using namespace snerf;

extern "C" int snerf_vis_fold(const SnerfVisIn* in, const SnerfVisOut* out, int m, int n_samples, long long row0, long long n,
                              SnerfVisStats* stats, void* stream) {
  if (!in || !out || !stats) { set_error("snerf_vis_fold: null pointer"); return SNERF_ERR_NULL; }
  if (m < 0 || row0 < 0 || n < 0 || row0 + (long long)m > n) {
    set_error("snerf_vis_fold: rows [%lld, %lld + %d) outside a frame of %lld rays", row0, row0, m, n); return SNERF_ERR_BAD_DESC; }
  const bool per_sample = in->albedo || in->sun || in->sky || in->beta || in->beta_semantic;
  if (per_sample && !in->weights) { set_error("snerf_vis_fold: per-sample inputs need weights"); return SNERF_ERR_NULL; }
  if (in->weights && (n_samples < 1 || n_samples > SNERF_VIS_MAX_SAMPLES)) {
    set_error("snerf_vis_fold: n_samples = %d outside [1, %d]", n_samples, SNERF_VIS_MAX_SAMPLES); return SNERF_ERR_BAD_DESC; }
  if ((in->rgb == nullptr) != (in->rgbs_gt == nullptr)) {
    set_error("snerf_vis_fold: rgb and rgbs_gt are given together or not at all"); return SNERF_ERR_NULL; }
  if ((in->semantic_gt || in->palette) && !in->label) { set_error("snerf_vis_fold: semantic_gt and palette need label"); return SNERF_ERR_NULL; }
  if (in->palette && in->n_palette < 1) { set_error("snerf_vis_fold: n_palette = %d < 1", in->n_palette); return SNERF_ERR_BAD_DESC; }
  if (in->semantic_gt && in->gt_dtype != SNERF_VIS_U8 && in->gt_dtype != SNERF_VIS_I64) {
    set_error("snerf_vis_fold: unknown label dtype %d", in->gt_dtype); return SNERF_ERR_BAD_DESC; }
  if (out->sem_shaded && !(in->sun && in->palette)) {
    set_error("snerf_vis_fold: sem_shaded needs sun and palette"); return SNERF_ERR_NULL; }
  if ((out->albedo_map && !in->albedo) || (out->sun_map && !in->sun) || (out->sky_map && !in->sky) || (out->beta_map && !in->beta) ||
      (out->beta_semantic_map && !in->beta_semantic) || (out->depth_map && !in->depth) ||
      ((out->rgb_diff || out->rgb_diff_distance) && !in->rgb) || (out->sem_color && !in->palette) ||
      (out->sem_error && !in->semantic_gt)) {
    set_error("snerf_vis_fold: an output plane is given without the input it is made from"); return SNERF_ERR_NULL; }
  if (m == 0) return SNERF_OK;
  const unsigned grid = blocks_for(m, VIS_WAVES, VIS_MAX_GRID);      // one wave per ray
  hipStream_t st = (hipStream_t)stream;
  const int S = in->weights ? n_samples : 1;
  if (in->semantic_gt && in->gt_dtype == SNERF_VIS_I64)
    hipLaunchKernelGGL(vis_fold_kernel<long long>, dim3(grid), dim3(VIS_THREADS), 0, st, *in, *out, m, S, row0, n, stats);
  else
    hipLaunchKernelGGL(vis_fold_kernel<uint8_t>, dim3(grid), dim3(VIS_THREADS), 0, st, *in, *out, m, S, row0, n, stats);
  SNERF_LAUNCH_CHECK();
  return SNERF_OK;
}

static int vis_plane_args(const char* what, const void* plane, int dtype, long long n) {
  if (!plane) { set_error("%s: null pointer", what); return SNERF_ERR_NULL; }
  if (dtype != SNERF_VIS_F32 && dtype != SNERF_VIS_F64) { set_error("%s: unknown plane dtype %d", what, dtype); return SNERF_ERR_BAD_DESC; }
  if (n < 0) { set_error("%s: n = %lld < 0", what, n); return SNERF_ERR_BAD_DESC; }
  return SNERF_OK;
}

extern "C" int snerf_vis_minmax(const void* plane, int plane_dtype, long long n, SnerfVisStats* stats, int slot, void* stream) {
  if (int rc = vis_plane_args("snerf_vis_minmax", plane, plane_dtype, n)) return rc;
  if (!stats) { set_error("snerf_vis_minmax: null pointer"); return SNERF_ERR_NULL; }
  if (slot < 0 || slot >= SNERF_VIS_SLOTS) { set_error("snerf_vis_minmax: slot %d outside [0, %d)", slot, SNERF_VIS_SLOTS); return SNERF_ERR_BAD_DESC; }
  if (n == 0) return SNERF_OK;
  hipStream_t st = (hipStream_t)stream;
  if (plane_dtype == SNERF_VIS_F32)
    hipLaunchKernelGGL(vis_minmax_kernel<float>, dim3(blocks_for(n, VIS_EW_THREADS, VIS_EW_MAX_GRID)), dim3(VIS_EW_THREADS), 0, st, (const float*)plane, n, slot, stats);
  else
    hipLaunchKernelGGL(vis_minmax_kernel<double>, dim3(blocks_for(n, VIS_EW_THREADS, VIS_EW_MAX_GRID)), dim3(VIS_EW_THREADS), 0, st, (const double*)plane, n, slot, stats);
  SNERF_LAUNCH_CHECK();
  return SNERF_OK;
}

extern "C" int snerf_vis_colormap(const void* plane, int plane_dtype, long long n, const SnerfVisStats* stats, int slot, double lo,
                                  double hi, const unsigned char* table, unsigned char* out, void* stream) {
  if (int rc = vis_plane_args("snerf_vis_colormap", plane, plane_dtype, n)) return rc;
  if (!table || !out) { set_error("snerf_vis_colormap: null pointer"); return SNERF_ERR_NULL; }
  if (slot >= SNERF_VIS_SLOTS) { set_error("snerf_vis_colormap: slot %d outside [0, %d)", slot, SNERF_VIS_SLOTS); return SNERF_ERR_BAD_DESC; }
  if (slot >= 0 && !stats) { set_error("snerf_vis_colormap: bounds from a slot need the stats block"); return SNERF_ERR_NULL; }
  if (slot < 0 && !(lo == lo && hi == hi)) { set_error("snerf_vis_colormap: explicit bounds must not be NaN"); return SNERF_ERR_BAD_DESC; }
  if (n == 0) return SNERF_OK;
  hipStream_t st = (hipStream_t)stream;
  if (plane_dtype == SNERF_VIS_F32)
    hipLaunchKernelGGL(vis_colormap_kernel<float>, dim3(blocks_for(n, VIS_EW_THREADS, VIS_EW_MAX_GRID)), dim3(VIS_EW_THREADS), 0, st, (const float*)plane, n, stats,
                       slot, lo, hi, table, out);
  else
    hipLaunchKernelGGL(vis_colormap_kernel<double>, dim3(blocks_for(n, VIS_EW_THREADS, VIS_EW_MAX_GRID)), dim3(VIS_EW_THREADS), 0, st, (const double*)plane, n, stats,
                       slot, lo, hi, table, out);
  SNERF_LAUNCH_CHECK();
  return SNERF_OK;
}
