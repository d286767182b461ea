// What the evaluation passes (dsm, ssim, semeval, vismaps, ortho, satrays, geo) share in reducing: the launch grid of a
// grid-stride kernel, the wave64 butterfly, the fixed-order workgroup tree over LDS, the strided sum of per-workgroup partials,
// and the order-preserving integer key of a double.  The summation order these give is part of every fp64 result's bits
// (DESIGN.md section 5k): per thread ascending, then the strided sum, then the tree, then a serial sum over the workgroups where
// a kernel has one.  The training step's kernels do not include this file.
#pragma once
#include "common.h"

namespace snerf {

// blocks of a grid-stride launch over n items: ceil(n / threads) in [1, cap]
static inline unsigned blocks_for(long long n, int threads, unsigned cap) {
  const long long want = (n + threads - 1) / threads;
  return (unsigned)(want < 1 ? 1 : (want < (long long)cap ? want : cap));
}

// The combining operations most sites use.  Min and max by comparison: the second operand wins only if it is strictly
// smaller / larger (fminf / fmaxf treat NaN differently; a site that wants them passes its own operation).
struct OpSum { template <typename V> __device__ __forceinline__ V operator()(V a, V b) const { return a + b; } };
struct OpMin { template <typename V> __device__ __forceinline__ V operator()(V a, V b) const { return b < a ? b : a; } };
struct OpMax { template <typename V> __device__ __forceinline__ V operator()(V a, V b) const { return b > a ? b : a; } };

// wave64 xor butterfly: every lane ends with op over the 64 lanes' values, combined in a fixed order
template <typename V, typename Op>
__device__ __forceinline__ V wave_reduce(V v, Op op) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o, 64));
  return v;
}

// Fixed-order tree over the T threads of a workgroup, K values at once (one barrier per level, whatever K is): thread t stores
// v[k] at lds[k * T + t], and each level o = T/2 ... 1 sets lds[k * T + t] = op(k, lds[k * T + t], lds[k * T + t + o]) for
// t < o.  After it, lds[k * T] holds the result of component k, visible to every thread.  A level reads its K pairs before it
// writes any of them: no LDS read is issued behind a write of the same level (tools/check_vgpr_hazards.py, scan 2).
template <int T, int K, typename V, typename Op>
__device__ __forceinline__ void block_tree(V* lds, int t, const V* v, Op op) {
#pragma unroll
  for (int k = 0; k < K; ++k) lds[k * T + t] = v[k];
  __syncthreads();
  for (int o = T / 2; o > 0; o >>= 1) {
    if (t < o) {
      V r[K];
#pragma unroll
      for (int k = 0; k < K; ++k) r[k] = op(k, lds[k * T + t], lds[k * T + t + o]);
#pragma unroll
      for (int k = 0; k < K; ++k) lds[k * T + t] = r[k];
    }
    __syncthreads();
  }
}

// one value per thread: the result is lds[0]
template <int T, typename V, typename Op>
__device__ __forceinline__ void block_tree(V* lds, int t, V v, Op op) {
  block_tree<T, 1>(lds, t, &v, [op](int, V a, V b) { return op(a, b); });
}

// The sum of the `count` doubles p[0], p[stride], p[2 * stride], ... by one workgroup of T threads: thread t adds elements
// t, t + T, ... in ascending order, then the tree.  The result is lds[0].
template <int T>
__device__ __forceinline__ void block_strided_sum(double* lds, int t, const double* __restrict__ p, long long count,
                                                  long long stride) {
  double a = 0.0;
  for (long long k = t; k < count; k += T) a += p[k * stride];
  block_tree<T>(lds, t, a, OpSum());
}

// order-preserving integer key of a double: a < b (as numbers) <=> key(a) < key(b) (as unsigned integers); no value has key 0
__device__ __forceinline__ unsigned long long order_key(double v) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(v);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double order_unkey(unsigned long long k) {
  const unsigned long long u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  return __longlong_as_double((long long)u);
}

}  // namespace snerf
