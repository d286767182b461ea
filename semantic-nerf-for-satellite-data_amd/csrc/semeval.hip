// Semantic evaluation on the device (snerf_amd/eval/utils/semantic.py; the reference's eval/eval_semantic.py and
// semantic/components/metrics.py).  The spec is stated in include/snerf_hip.h.  One streaming pass per render chunk folds the
// chunk's labels, targets and per-sample weights / beta into an accumulator that lives on the device across chunks:
//   - integer counts (confusion matrix, the four accuracy error counts, rays, car rays, out-of-range rows) go through one
//     LDS u32 histogram per workgroup and then one global 64-bit integer atomic add per non-zero bin: integer sums commute,
//     so the counts are exact and do not depend on arrival order;
//   - the composited beta of the car rays is summed in fp64 (the fp32 products w * beta are exact in fp64) and written as
//     one partial per workgroup at a fixed slot; a second launch sums the slots in a fixed order and adds the result into
//     the accumulator (reduce.h; no float atomics), so the sum is bit-reproducible at a fixed chunking.
// No host synchronisation, no allocation.
#include "reduce.h"
#include "../../include/snerf_hip.h"

#include <stdint.h>

namespace snerf {

constexpr int SEM_THREADS = 256;        // one ray per thread in the label phase; a workgroup's tile is SEM_THREADS rays
constexpr int SEM_MAX_GRID = 2048;      // memory-bound grid cap; the workgroups stride over the tiles
constexpr int SEM_REDUCE_THREADS = 256;
constexpr int SEM_NCOUNT = 6;           // LDS counters: errors[0..3], car rays, out-of-range rows

static_assert(SNERF_SEMEVAL_MAX_CLASSES * SNERF_SEMEVAL_MAX_CLASSES <= SEM_THREADS, "one thread per bin in the flush");

// Tile loop: the label phase reads one ray per thread (pred 8 B, targets 1 or 8 B: coalesced), bins (gt, pred) into the LDS
// histogram and marks the car rays in LDS.  If any ray of the tile is a car, the beta phase walks the tile's weights and
// beta rows as one flat, contiguous range of cnt * S floats (consecutive lanes on consecutive floats, whatever S is) and
// accumulates w * beta of the car rays' samples in fp64; rows of non-car rays are not read.
template <typename L>
__global__ __launch_bounds__(SEM_THREADS) void semeval_kernel(const long long* __restrict__ pred, const L* __restrict__ gt,
                                                              const L* __restrict__ gt_no_cars, const L* __restrict__ gt_nc,
                                                              int n, int C, int car, const float* __restrict__ weights,
                                                              const float* __restrict__ beta, int S,
                                                              SnerfSemevalAcc* __restrict__ acc, double* __restrict__ partial) {
  __shared__ unsigned hist[SNERF_SEMEVAL_MAX_CLASSES * SNERF_SEMEVAL_MAX_CLASSES];
  __shared__ unsigned cnt_lds[SEM_NCOUNT];
  __shared__ unsigned char is_car[SEM_THREADS];
  __shared__ double red[SEM_THREADS];
  const int t = threadIdx.x;
  if (t < C * C) hist[t] = 0u;
  if (t < SEM_NCOUNT) cnt_lds[t] = 0u;
  __syncthreads();
  const bool with_beta = weights != nullptr;
  // the thread's walk over a tile's flat sample range advances THREADS floats = qd rays and rm samples per step
  const int qd = with_beta ? SEM_THREADS / S : 0, rm = with_beta ? SEM_THREADS % S : 0;
  double bsum = 0.0;
  for (long long r0 = (long long)blockIdx.x * SEM_THREADS; r0 < n; r0 += (long long)gridDim.x * SEM_THREADS) {
    const long long r = r0 + t;
    bool car_ray = false;
    if (r < n) {
      const long long p = pred[r];
      const long long g = (long long)gt[r];
      if (g >= 0 && g < C && p >= 0 && p < C) atomicAdd(&hist[(int)g * C + (int)p], 1u);
      else atomicAdd(&cnt_lds[5], 1u);
      if (g != p) atomicAdd(&cnt_lds[0], 1u);
      car_ray = car >= 0 && g == car;
      if (car_ray) atomicAdd(&cnt_lds[4], 1u);
      if (gt_no_cars && (long long)gt_no_cars[r] != p) atomicAdd(&cnt_lds[1], 1u);
      if (gt_nc) {
        const long long q = (long long)gt_nc[r];
        if (q != p) {
          atomicAdd(&cnt_lds[2], 1u);
          // the reference's filter_idx: rows whose target is the car class count as correct (but stay in the denominator)
          if (!(car >= 0 && q == car)) atomicAdd(&cnt_lds[3], 1u);
        }
      }
    }
    is_car[t] = car_ray ? 1 : 0;
    const int any_car = __syncthreads_or(car_ray ? 1 : 0);
    if (with_beta && any_car) {
      const long long cnt = (n - r0) < SEM_THREADS ? (n - r0) : SEM_THREADS;
      const long long total = cnt * S;
      const float* wp = weights + r0 * S;
      const float* bp = beta + r0 * S;
      int ray = t / S, s = t % S;
      for (long long e = t; e < total; e += SEM_THREADS) {
        if (is_car[ray]) bsum = fma((double)wp[e], (double)bp[e], bsum);
        ray += qd;
        s += rm;
        if (s >= S) { s -= S; ++ray; }
      }
    }
    __syncthreads();       // is_car is rewritten by the next tile
  }
  if (t < C * C) {
    const unsigned h = hist[t];
    if (h) atomicAdd(&acc->conf[(t / C) * SNERF_SEMEVAL_MAX_CLASSES + t % C], (unsigned long long)h);
  }
  if (t < SEM_NCOUNT) {
    const unsigned c = cnt_lds[t];
    unsigned long long* dst = t < 4 ? &acc->errors[t] : t == 4 ? &acc->car_rays : &acc->out_of_range;
    if (c) atomicAdd(dst, (unsigned long long)c);
  }
  if (blockIdx.x == 0 && t == 0) atomicAdd(&acc->rays, (unsigned long long)n);
  if (with_beta) {
    block_tree<SEM_THREADS>(red, t, bsum, OpSum());
    if (t == 0) partial[blockIdx.x] = red[0];
  }
}

// one workgroup: the sum of the grid's partials in the order of reduce.h, added into the accumulator
__global__ __launch_bounds__(SEM_REDUCE_THREADS) void semeval_reduce_kernel(const double* __restrict__ partial, int count,
                                                                            SnerfSemevalAcc* __restrict__ acc) {
  __shared__ double red[SEM_REDUCE_THREADS];
  block_strided_sum<SEM_REDUCE_THREADS>(red, threadIdx.x, partial, count, 1);
  if (threadIdx.x == 0) acc->beta_car_sum += red[0];
}

}  // namespace snerf

using namespace snerf;

extern "C" size_t snerf_semeval_workspace_bytes(int n_rays, int n_samples) {
  if (n_rays < 0 || n_samples < 1) { set_error("snerf_semeval_workspace_bytes: n_rays must be >= 0 and n_samples >= 1"); return 0; }
  return (size_t)blocks_for(n_rays, SEM_THREADS, SEM_MAX_GRID) * sizeof(double);
}

extern "C" int snerf_semeval_accumulate(const long long* pred, const void* gt, const void* gt_no_cars, const void* gt_non_corrupted,
                                        int label_dtype, int n, int n_classes, int car_idx, const float* weights,
                                        const float* beta, int n_samples, SnerfSemevalAcc* acc, void* workspace,
                                        size_t workspace_bytes, void* stream) {
  if (!pred || !gt || !acc) { set_error("snerf_semeval_accumulate: null pointer"); return SNERF_ERR_NULL; }
  if (n < 0) { set_error("snerf_semeval_accumulate: n = %d < 0", n); return SNERF_ERR_BAD_DESC; }
  if (n_classes < 1 || n_classes > SNERF_SEMEVAL_MAX_CLASSES) {
    set_error("snerf_semeval_accumulate: n_classes = %d outside [1, %d]", n_classes, SNERF_SEMEVAL_MAX_CLASSES); return SNERF_ERR_BAD_DESC; }
  if (car_idx < -1 || car_idx >= n_classes) {
    set_error("snerf_semeval_accumulate: car_idx = %d outside [-1, %d)", car_idx, n_classes); return SNERF_ERR_BAD_DESC; }
  if (label_dtype != SNERF_SEMEVAL_U8 && label_dtype != SNERF_SEMEVAL_I64) {
    set_error("snerf_semeval_accumulate: unknown label dtype %d", label_dtype); return SNERF_ERR_BAD_DESC; }
  if ((weights == nullptr) != (beta == nullptr)) {
    set_error("snerf_semeval_accumulate: weights and beta are given together or not at all"); return SNERF_ERR_NULL; }
  const bool with_beta = weights != nullptr;
  if (with_beta && n_samples < 1) { set_error("snerf_semeval_accumulate: n_samples = %d < 1", n_samples); return SNERF_ERR_BAD_DESC; }
  const unsigned grid = blocks_for(n, SEM_THREADS, SEM_MAX_GRID);
  if (with_beta) {
    if (!workspace) { set_error("snerf_semeval_accumulate: null workspace"); return SNERF_ERR_NULL; }
    if (workspace_bytes < (size_t)grid * sizeof(double)) {
      set_error("snerf_semeval_accumulate: workspace of %zu bytes < %zu", workspace_bytes, (size_t)grid * sizeof(double));
      return SNERF_ERR_WORKSPACE; }
  }
  if (n == 0) return SNERF_OK;
  hipStream_t st = (hipStream_t)stream;
  double* part = (double*)workspace;
  const int S = with_beta ? n_samples : 1;
  if (label_dtype == SNERF_SEMEVAL_U8) {
    hipLaunchKernelGGL(semeval_kernel<uint8_t>, dim3(grid), dim3(SEM_THREADS), 0, st, pred, (const uint8_t*)gt,
                       (const uint8_t*)gt_no_cars, (const uint8_t*)gt_non_corrupted, n, n_classes, car_idx, weights, beta, S,
                       acc, part);
  } else {
    hipLaunchKernelGGL(semeval_kernel<long long>, dim3(grid), dim3(SEM_THREADS), 0, st, pred, (const long long*)gt,
                       (const long long*)gt_no_cars, (const long long*)gt_non_corrupted, n, n_classes, car_idx, weights,
                       beta, S, acc, part);
  }
  SNERF_LAUNCH_CHECK();
  if (with_beta) {
    hipLaunchKernelGGL(semeval_reduce_kernel, dim3(1), dim3(SEM_REDUCE_THREADS), 0, st, (const double*)part, (int)grid, acc);
    SNERF_LAUNCH_CHECK();
  }
  return SNERF_OK;
}
