// What a one-wave-per-ray kernel needs (resample.hip, raydist.hip): a wave64 owns a ray, up to four rays share a workgroup, the
// ray's working set lives in the wave's own slice of LDS, and integer run totals are scanned across the lanes with shuffles.
// Primitives only: the arithmetic, what lives in LDS and the order of loads and stores are the kernel's own.
#pragma once
#include "common.h"

namespace snerf {

constexpr int RAY_WAVE = 64;
constexpr int RAY_WAVE_MAX_RAYS_PER_BLOCK = 4;
constexpr size_t RAY_WAVE_MAX_LDS = 65536;

// The launch of a kernel that keeps ray_bytes of LDS per ray: as many rays per workgroup as fit in RAY_WAVE_MAX_LDS, at most
// RAY_WAVE_MAX_RAYS_PER_BLOCK; one wave per ray; the last workgroup may be ragged.  The caller's limits keep ray_bytes within
// RAY_WAVE_MAX_LDS, so at least one ray fits.  ray_bytes = 0 (raymedian.hip: a ray kept in registers) gives the full workgroup.
struct RayWaveLaunch {
  dim3 grid, block;
  size_t lds_bytes;
};
static inline RayWaveLaunch ray_wave_launch(int n_rays, size_t ray_bytes) {
  size_t rays_per_block = ray_bytes ? RAY_WAVE_MAX_LDS / ray_bytes : (size_t)RAY_WAVE_MAX_RAYS_PER_BLOCK;
  if (rays_per_block > (size_t)RAY_WAVE_MAX_RAYS_PER_BLOCK) rays_per_block = RAY_WAVE_MAX_RAYS_PER_BLOCK;
  const unsigned blocks = (unsigned)(((long long)n_rays + (long long)rays_per_block - 1) / (long long)rays_per_block);
  return {dim3(blocks), dim3((unsigned)(RAY_WAVE * rays_per_block)), rays_per_block * ray_bytes};
}

// Which ray this wave owns.  The kernel's first statement after it is `if (ray >= n_rays) return;`: wave-uniform, it retires the
// idle waves of a ragged last workgroup at once.  Such a kernel therefore must not use a workgroup barrier (__syncthreads): the
// retired waves never arrive at it.  A wave shares its slice of LDS with no other wave; ray_wave_sync() is all it needs.
struct RayWaveId {
  int lane, wave;
  long long ray;
};
__device__ __forceinline__ RayWaveId ray_wave_id() {
  const int wave = threadIdx.x / RAY_WAVE;
  return {(int)(threadIdx.x & (RAY_WAVE - 1)), wave, (long long)blockIdx.x * (blockDim.x / RAY_WAVE) + wave};
}

// Makes what the wave's lanes wrote to its slice of LDS visible to all of its lanes.
__device__ __forceinline__ void ray_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Scan of the lanes' run totals: returns the sum of `run` over the lanes below this one (the exclusive offset of the lane's run)
// and, where total is not NULL, the sum over the whole wave through it.  Integers: the result has no summation order.
__device__ __forceinline__ long long wave_scan_i64(long long run, int lane, long long* total) {
  long long incl = run;
#pragma unroll
  for (int o = 1; o < RAY_WAVE; o <<= 1) {
    const long long up = __shfl_up(incl, o, RAY_WAVE);
    if (lane >= o) incl += up;
  }
  if (total) *total = __shfl(incl, RAY_WAVE - 1, RAY_WAVE);
  return incl - run;
}

}  // namespace snerf
