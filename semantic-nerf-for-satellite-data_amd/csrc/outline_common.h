// What the outline entries (outline.hip) and the arc entries (rooflines.hip) share: the launch shapes, the counters of a kernel, the
// unit steps and the id raster with its padding of 0.
#pragma once
#include "reduce.h"

namespace snerf {

constexpr int OUT_THREADS = 256;
constexpr unsigned OUT_MAX_BLOCKS = 65536;               // items beyond it are taken in a grid-stride
constexpr unsigned OUT_COUNT_BLOCKS = 1024;              // the same for a kernel that ends in atomics on its few counters: every
                                                         // workgroup adds to the SAME words, and one row takes some 125 adds per microsecond
constexpr int OUT_NIL = -1;

// the counters of a kernel: the sums over the workgroup (the waves' sums meet in LDS), added to stats[0 .. N) by one thread; a
// sum of 0 adds nothing.  Every thread of the workgroup calls it.
template <int N>
__device__ __forceinline__ void add_counts(unsigned long long (&v)[N], unsigned long long* __restrict__ stats) {
  __shared__ unsigned long long partial[N][OUT_THREADS / 64];
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const unsigned long long sum = wave_reduce(v[k], OpSum());
    if ((threadIdx.x & 63) == 0) partial[k][threadIdx.x >> 6] = sum;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < N; ++k) {
      unsigned long long sum = 0;
      for (int wave = 0; wave < OUT_THREADS / 64; ++wave) sum += partial[k][wave];
      if (sum) atomicAdd(&stats[k], sum);
    }
  }
}

// step(d) of the header: E, S, W, N in (row, column)
__device__ __forceinline__ int step_j(int d) { return d == 1 ? 1 : d == 3 ? -1 : 0; }
__device__ __forceinline__ int step_i(int d) { return d == 0 ? 1 : d == 2 ? -1 : 0; }

struct IdRaster {
  const int* ids;
  int h, w;
  long long K;
  // the id of cell (j, i): 0 outside the raster and for an id outside [0, K]
  __device__ __forceinline__ int at(int j, int i) const {
    if (j < 0 || j >= h || i < 0 || i >= w) return 0;
    const int id = ids[(long long)j * w + i];
    return (id < 0 || id > K) ? 0 : id;
  }
};

// no corner exactly when the cell behind the tail carries n and the one beside it does not
__device__ __forceinline__ bool is_corner(const IdRaster& g, int j, int i, int d, int n) {
  const int rj = j - step_j(d), ri = i - step_i(d);
  const int lj = rj + step_j((d + 3) & 3), li = ri + step_i((d + 3) & 3);
  return !(g.at(rj, ri) == n && g.at(lj, li) != n);
}

}  // namespace snerf
