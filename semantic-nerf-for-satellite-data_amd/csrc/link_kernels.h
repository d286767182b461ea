// The three launches of a connected-components labelling over the lock-free union of csrc/objects_walk.h -- init, merge, flatten --
// templated on what makes two neighbouring cells one component.  snerf_objects_link (csrc/objects.hip: same class, of a set of
// classes) and snerf_roofs_link (csrc/roofs.hip: same non-negative tag) are the two users; the walk and its guards are shared, not
// copied.  A predicate P gives
//     int  load(long long cell)     the cell's word (a class, a tag)
//     bool member(int word)         whether a cell with that word takes part
// and two member cells are linked when they are neighbours and their words are equal.
#pragma once
#include "objects_walk.h"
#include "reduce.h"

namespace snerf {

constexpr int LINK_THREADS = 256;
constexpr unsigned LINK_MAX_BLOCKS = 65536;              // cells beyond it are taken in a grid-stride

// the device side of the walk's memory policy: relaxed, agent scope
struct DeviceParents {
  int* parent;
  __device__ __forceinline__ int load(int c) { return __hip_atomic_load(parent + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  __device__ __forceinline__ int fetch_min(int c, int v) {
    return __hip_atomic_fetch_min(parent + c, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
};

// One thread per cell, consecutive lanes on consecutive cells of a row: a wave's W unions stay in lines it already holds.
template <typename P>
__global__ __launch_bounds__(LINK_THREADS) void link_init_kernel(P pred, int cells, int* __restrict__ parent,
                                                                 unsigned long long* __restrict__ stats) {
  unsigned long long members = 0;
  for (long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x; c < cells; c += (long long)gridDim.x * blockDim.x) {
    const bool in = pred.member(pred.load(c));
    parent[c] = in ? (int)c : -1;
    members += in ? 1 : 0;
  }
  members = wave_reduce(members, OpSum());
  if ((threadIdx.x & 63) == 0 && members) atomicAdd(&stats[1], members);
}

template <typename P>
__global__ __launch_bounds__(LINK_THREADS) void link_merge_kernel(P pred, int h, int w, int eight, int* parent,
                                                                  unsigned long long* __restrict__ stats) {
  DeviceParents m = {parent};
  const long long cells = (long long)h * w;
  unsigned long long trips = 0;
  for (long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x; c < cells; c += (long long)gridDim.x * blockDim.x) {
    const int l = pred.load(c);
    if (!pred.member(l)) continue;
    const int j = (int)(c / w), i = (int)(c - (long long)j * w);
    if (i > 0 && pred.load(c - 1) == l) trips += walk_unite(m, (int)c, (int)c - 1);
    if (j > 0) {
      const long long n = c - w;
      if (pred.load(n) == l) trips += walk_unite(m, (int)c, (int)n);
      if (eight && i > 0 && pred.load(n - 1) == l) trips += walk_unite(m, (int)c, (int)n - 1);
      if (eight && i + 1 < w && pred.load(n + 1) == l) trips += walk_unite(m, (int)c, (int)n + 1);
    }
  }
  if (trips) atomicAdd(&stats[0], trips);
}

static __global__ __launch_bounds__(LINK_THREADS) void link_flatten_kernel(int cells, int* parent, unsigned long long* __restrict__ stats) {
  DeviceParents m = {parent};
  unsigned long long trips = 0;
  for (long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x; c < cells; c += (long long)gridDim.x * blockDim.x) {
    if (m.load((int)c) < 0) continue;                        // not a member (init's -1)
    const int root = walk_find(m, (int)c);
    if (root < 0) { trips++; continue; }
    // a walk that passes through c meanwhile reads the old ancestor or the root: both lie below c in c's component
    __hip_atomic_store(parent + c, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (trips) atomicAdd(&stats[0], trips);
}

// init, merge, flatten on `stream`; SNERF_OK or the launch's error
template <typename P>
static int link_launch(const P& pred, int h, int w, int connectivity, int* parent, unsigned long long* stats, void* stream) {
  const int cells = h * w;
  const dim3 grid(blocks_for(cells, LINK_THREADS, LINK_MAX_BLOCKS)), block(LINK_THREADS);
  hipLaunchKernelGGL(link_init_kernel<P>, grid, block, 0, (hipStream_t)stream, pred, cells, parent, stats);
  SNERF_LAUNCH_CHECK();
  hipLaunchKernelGGL(link_merge_kernel<P>, grid, block, 0, (hipStream_t)stream, pred, h, w, connectivity == 8 ? 1 : 0, parent, stats);
  SNERF_LAUNCH_CHECK();
  hipLaunchKernelGGL(link_flatten_kernel, grid, block, 0, (hipStream_t)stream, cells, parent, stats);
  SNERF_LAUNCH_CHECK();
  return SNERF_OK;
}

}  // namespace snerf
