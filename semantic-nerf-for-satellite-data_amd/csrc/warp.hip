// Warping a raster from one map lattice onto another: nearest, bilinear, area average / minimum / maximum of float planes, nearest and
// majority of a label plane.  The spec is include/snerf_warp.h and DESIGN.md section 5zd.
//   - fp64, evaluated operation by operation (no fused multiply-adds in this file), only + - * /, floor / ceil, comparisons and integer
//     work: tests/warp_numpy.py reproduces every word bit for bit;
//   - the planes and the nearest label: one thread per destination cell, a workgroup is one 64 x 4 tile of cells, a wave is 64
//     neighbouring cells of a row.  At steps near 1 neighbouring lanes read neighbouring addresses; at large steps every lane walks
//     whole cache lines of its own, row by row.  Either way a source line is fetched about once; nothing is staged in LDS;
//   - the majority: one wave per destination cell, the lanes stride over the members; the wave owns a histogram of 256 words in LDS;
//   - the loops are counted by the map alone, nothing terminates on memory content; the only atomics are integer (the LDS histogram,
//     the counts of `stats`): no result depends on the order of the launch.
// No allocation, no copy and no host synchronisation; every entry runs on the caller's stream.
#include "lattice.h"
#include "reduce.h"
#include "../../include/snerf_warp.h"

#pragma clang fp contract(off)

namespace snerf {

constexpr int WARP_TILE_X = 64, WARP_TILE_Y = 4;
constexpr int WARP_THREADS = WARP_TILE_X * WARP_TILE_Y;
constexpr int WARP_WAVES = WARP_THREADS / 64;
// Tiles (cells of the majority) beyond it are strided over: four workgroups per CU.  Every workgroup ends in up to three atomics on the
// same three words, which the L2 serialises at some 6 to 9 ns each: one set per wave of 16,384 workgroups cost 1.2 ms whatever the method.
constexpr unsigned WARP_MAX_BLOCKS = 1024;
constexpr unsigned char WARP_NO_LABEL = SNERF_ORTHO_NO_LABEL;

// The taps of one destination cell on one axis: source cells k0 ... k0 + n - 1.  NEAREST and BILINEAR carry their (at most two)
// weights; the area methods compute a tap's weight from the cell's bounds [a, b).  The host has checked that every coordinate lies
// inside (-2^31, 2^31): floor(a) ... ceil(b) - 1 are int32, and a count is taken in fp64 (exact) before it becomes an integer.
struct AxisTaps {
  int k0, n;
  double a, b, w0, w1;
};

template <int METHOD>
__device__ __forceinline__ AxisTaps axis_taps(double off, double step, int i) {
  AxisTaps t;
  t.a = off + (double)i * step;
  t.b = off + ((double)i + 1.0) * step;
  t.w0 = 1.0;
  t.w1 = 0.0;
  const double c = off + ((double)i + 0.5) * step;
  if (METHOD == SNERF_WARP_NEAREST) {
    t.k0 = (int)floor(c);
    t.n = 1;
  } else if (METHOD == SNERF_WARP_BILINEAR) {
    const double u = c - 0.5, k = floor(u), f = u - k;
    t.k0 = (int)k;
    t.n = 2;
    t.w0 = 1.0 - f;
    t.w1 = f;
  } else {
    const double k = floor(t.a);
    t.k0 = (int)k;
    t.n = (int)(ceil(t.b) - k);
  }
  return t;
}

// the weight of tap k0 + s
template <int METHOD>
__device__ __forceinline__ double tap_weight(const AxisTaps& t, int s) {
  if (METHOD == SNERF_WARP_NEAREST || METHOD == SNERF_WARP_BILINEAR) return s == 0 ? t.w0 : t.w1;
  const double k = (double)(t.k0 + s);
  return fmin(k + 1.0, t.b) - fmax(k, t.a);
}

// the cell (i, j) of tile `tile`, false beyond the raster
__device__ __forceinline__ bool warp_tile_cell(long long tile, int tiles_x, int w, int h, int* i, int* j) {
  *i = (int)(tile % tiles_x) * WARP_TILE_X + (int)(threadIdx.x & 63);
  *j = (int)(tile / tiles_x) * WARP_TILE_Y + (int)(threadIdx.x >> 6);
  return *i < w && *j < h;
}

// the three counts of a workgroup: reduced inside each wave, then over the waves through LDS, then one atomic per count.  Every thread
// of the workgroup calls it.
__device__ __forceinline__ void warp_add_stats(unsigned long long written, unsigned long long holes, unsigned long long outside,
                                               unsigned long long* __restrict__ stats) {
  __shared__ unsigned long long part[WARP_WAVES][3];
  written = wave_reduce(written, OpSum());
  holes = wave_reduce(holes, OpSum());
  outside = wave_reduce(outside, OpSum());
  if ((threadIdx.x & 63) == 0) {
    part[threadIdx.x >> 6][0] = written;
    part[threadIdx.x >> 6][1] = holes;
    part[threadIdx.x >> 6][2] = outside;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    unsigned long long total = 0;
#pragma unroll
    for (int w = 0; w < WARP_WAVES; ++w) total += part[w][threadIdx.x];
    if (total) atomicAdd(&stats[threadIdx.x], total);
  }
}

template <int METHOD>
__global__ __launch_bounds__(WARP_THREADS) void warp_planes_kernel(const float* __restrict__ src, int planes, SnerfWarpMap m,
                                                                  double min_valid, int tiles_x, long long n_tiles,
                                                                  float* __restrict__ dst, unsigned long long* __restrict__ stats) {
  unsigned long long n_written = 0, n_holes = 0, n_outside = 0;
  const long long src_cells = (long long)m.src_h * m.src_w, dst_cells = (long long)m.dst_h * m.dst_w;
  for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    int i, j;
    if (!warp_tile_cell(tile, tiles_x, m.dst_w, m.dst_h, &i, &j)) continue;
    const AxisTaps tx = axis_taps<METHOD>(m.off_x, m.step_x, i), ty = axis_taps<METHOD>(m.off_y, m.step_y, j);
    const long long o = (long long)j * m.dst_w + i;
    bool outside = false;
    for (int p = 0; p < planes; ++p) {
      const float* __restrict__ plane = src + p * src_cells;
      double tot = 0.0, num = -0.0, den = 0.0;
      float best = 0.f;
      bool any = false;
      for (int sy = 0; sy < ty.n; ++sy) {
        const double wy = tap_weight<METHOD>(ty, sy);
        if (!(wy > 0.0)) continue;
        const int ky = ty.k0 + sy;
        const bool row_in = ky >= 0 && ky < m.src_h;
        for (int sx = 0; sx < tx.n; ++sx) {
          const double wx = tap_weight<METHOD>(tx, sx);
          if (!(wx > 0.0)) continue;
          const int kx = tx.k0 + sx;
          const double w = wy * wx;
          tot += w;
          if (!(row_in && kx >= 0 && kx < m.src_w)) {
            outside = true;
            continue;
          }
          const float v = plane[(long long)ky * m.src_w + kx];
          if (!(fabsf(v) < __builtin_inff())) continue;           // NaN, +-inf: a hole
          den += w;
          if (METHOD == SNERF_WARP_MIN) {
            if (!any || v < best) best = v;
          } else if (METHOD == SNERF_WARP_MAX) {
            if (!any || v > best) best = v;
          } else if (METHOD == SNERF_WARP_NEAREST) {
            best = v;
          } else {
            num += w * (double)v;
          }
          any = true;
        }
      }
      float r = __builtin_nanf("");
      if (METHOD == SNERF_WARP_NEAREST) {
        if (any) r = best;
      } else if (den > 0.0 && den >= min_valid * tot) {
        r = (METHOD == SNERF_WARP_MIN || METHOD == SNERF_WARP_MAX) ? best : (float)(num / den);
      }
      dst[p * dst_cells + o] = r;
      if (r != r) ++n_holes; else ++n_written;
    }
    n_outside += outside ? 1u : 0u;
  }
  warp_add_stats(n_written, n_holes, n_outside, stats);
}

__global__ __launch_bounds__(WARP_THREADS) void warp_labels_nearest_kernel(const unsigned char* __restrict__ src, SnerfWarpMap m, int tiles_x,
                                                                          long long n_tiles, unsigned char* __restrict__ dst,
                                                                          unsigned long long* __restrict__ stats) {
  unsigned long long n_written = 0, n_holes = 0, n_outside = 0;
  for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    int i, j;
    if (!warp_tile_cell(tile, tiles_x, m.dst_w, m.dst_h, &i, &j)) continue;
    const int kx = axis_taps<SNERF_WARP_NEAREST>(m.off_x, m.step_x, i).k0, ky = axis_taps<SNERF_WARP_NEAREST>(m.off_y, m.step_y, j).k0;
    const bool in = kx >= 0 && kx < m.src_w && ky >= 0 && ky < m.src_h;
    const unsigned char c = in ? src[(long long)ky * m.src_w + kx] : WARP_NO_LABEL;
    dst[(long long)j * m.dst_w + i] = c;
    if (c == WARP_NO_LABEL) ++n_holes; else ++n_written;
    n_outside += in ? 0u : 1u;
  }
  warp_add_stats(n_written, n_holes, n_outside, stats);
}

// the members of a destination cell on one axis: k0 ... k0 + n - 1
__device__ __forceinline__ void axis_members(double off, double step, int i, int* k0, int* n) {
  const double a = off + (double)i * step, b = off + ((double)i + 1.0) * step, c = off + ((double)i + 0.5) * step;
  const double lo = ceil(a - 0.5), hi = ceil(b - 0.5);
  *k0 = (int)(hi > lo ? lo : floor(c));
  *n = hi > lo ? (int)(hi - lo) : 1;
}

// One wave per destination cell, WARP_WAVES cells per pass of a workgroup; every wave of the workgroup takes every barrier (a wave
// beyond the last cell counts nothing and writes nothing).
__global__ __launch_bounds__(WARP_THREADS) void warp_labels_mode_kernel(const unsigned char* __restrict__ src, SnerfWarpMap m, long long cells,
                                                                       unsigned char* __restrict__ dst,
                                                                       unsigned long long* __restrict__ stats) {
  __shared__ unsigned int hist[WARP_WAVES][256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned long long n_written = 0, n_holes = 0, n_outside = 0;                 // lane 0 counts for its wave
  for (long long base = (long long)blockIdx.x * WARP_WAVES; base < cells; base += (long long)gridDim.x * WARP_WAVES) {
    const long long cell = base + wave;
    const bool active = cell < cells;                                         // wave-uniform
#pragma unroll
    for (int q = 0; q < 4; ++q) hist[wave][lane * 4 + q] = 0u;
    __syncthreads();
    bool outside = false;
    if (active) {
      const int i = (int)(cell % m.dst_w), j = (int)(cell / m.dst_w);
      int kx0, ky0, nx, ny;
      axis_members(m.off_x, m.step_x, i, &kx0, &nx);
      axis_members(m.off_y, m.step_y, j, &ky0, &ny);
      const int members = nx * ny;                                            // at most 66 * 66
      for (int t = lane; t < members; t += 64) {
        const int ky = ky0 + t / nx, kx = kx0 + t % nx;
        if (ky >= 0 && ky < m.src_h && kx >= 0 && kx < m.src_w) {
          const unsigned char c = src[(long long)ky * m.src_w + kx];
          if (c != WARP_NO_LABEL) atomicAdd(&hist[wave][c], 1u);
        } else {
          outside = true;
        }
      }
    }
    __syncthreads();
    // lane l scans the classes 4 l ... 4 l + 3; the key (count << 8) | (255 - class): the most votes, then the lowest class
    unsigned int key = 0u;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const unsigned int c = (unsigned int)(lane * 4 + q), k = (hist[wave][c] << 8) | (255u - c);
      key = k > key ? k : key;
    }
    key = wave_reduce(key, OpMax());
    const bool any_outside = __builtin_amdgcn_ballot_w64(outside) != 0ull;
    if (active && lane == 0) {
      const unsigned char winner = (key >> 8) ? (unsigned char)(255u - (key & 255u)) : WARP_NO_LABEL;
      dst[cell] = winner;
      if (winner == WARP_NO_LABEL) ++n_holes; else ++n_written;
      n_outside += any_outside ? 1u : 0u;
    }
    __syncthreads();                                                          // the scan is done before the next pass zeroes
  }
  warp_add_stats(n_written, n_holes, n_outside, stats);
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
static bool warp_axis_ok(const char* who, const char* axis, double off, double step, int extent, bool area) {
  if (!(step > 0.0) || !isfinite(step)) { set_error("%s: step_%s = %.17g must be finite and > 0", who, axis, step); return false; }
  if (!(fabs(off) + (double)extent * step < 2147483648.0)) {                   // false for a NaN or infinite offset too
    set_error("%s: |off_%s| + dst extent * step_%s = |%.17g| + %d * %.17g must stay below 2^31", who, axis, axis, off, extent, step);
    return false;
  }
  if (area && step > (double)SNERF_WARP_MAX_STEP) {
    set_error("%s: step_%s = %.17g above %d (SNERF_WARP_MAX_STEP) for this method", who, axis, step, SNERF_WARP_MAX_STEP);
    return false;
  }
  return true;
}

static bool warp_map_ok(const char* who, const SnerfWarpMap* m, bool area) {
  if (m->src_w < 1 || m->src_h < 1 || m->dst_w < 1 || m->dst_h < 1) {
    set_error("%s: every size must be >= 1 (src %d x %d, dst %d x %d)", who, m->src_h, m->src_w, m->dst_h, m->dst_w);
    return false;
  }
  return lattice_cells_ok(who, m->src_h, m->src_w) && lattice_cells_ok(who, m->dst_h, m->dst_w) &&
         warp_axis_ok(who, "x", m->off_x, m->step_x, m->dst_w, area) && warp_axis_ok(who, "y", m->off_y, m->step_y, m->dst_h, area);
}

static inline long long warp_tiles(const SnerfWarpMap* m, int* tiles_x) {
  *tiles_x = (m->dst_w + WARP_TILE_X - 1) / WARP_TILE_X;
  return (long long)*tiles_x * ((m->dst_h + WARP_TILE_Y - 1) / WARP_TILE_Y);
}

}  // namespace snerf

using namespace snerf;

extern "C" int snerf_warp_planes(const float* src, int planes, const SnerfWarpMap* map, int method, double min_valid, float* dst,
                                 unsigned long long* stats, void* stream) {
  const char* who = "snerf_warp_planes";
  if (!src || !map || !dst || !stats) { set_error("%s: null pointer", who); return SNERF_ERR_NULL; }
  if (src == dst) { set_error("%s: dst must not alias src", who); return SNERF_ERR_BAD_DESC; }
  if (method < SNERF_WARP_NEAREST || method > SNERF_WARP_MAX) {
    set_error("%s: method = %d is none of NEAREST, BILINEAR, AVERAGE, MIN, MAX (0 ... 4)", who, method);
    return SNERF_ERR_BAD_DESC;
  }
  if (planes < 1 || planes > SNERF_WARP_MAX_PLANES) {
    set_error("%s: planes = %d outside [1, %d]", who, planes, SNERF_WARP_MAX_PLANES);
    return SNERF_ERR_BAD_DESC;
  }
  if (!(min_valid > 0.0 && min_valid <= 1.0)) { set_error("%s: min_valid = %.17g outside (0, 1]", who, min_valid); return SNERF_ERR_BAD_DESC; }
  if (!warp_map_ok(who, map, method >= SNERF_WARP_AVERAGE)) return SNERF_ERR_BAD_DESC;
  int tiles_x;
  const long long n_tiles = warp_tiles(map, &tiles_x);
  const dim3 grid(blocks_for(n_tiles, 1, WARP_MAX_BLOCKS)), block(WARP_THREADS);
  const hipStream_t s = (hipStream_t)stream;
  switch (method) {
    case SNERF_WARP_NEAREST:
      hipLaunchKernelGGL(warp_planes_kernel<SNERF_WARP_NEAREST>, grid, block, 0, s, src, planes, *map, min_valid, tiles_x, n_tiles, dst, stats);
      break;
    case SNERF_WARP_BILINEAR:
      hipLaunchKernelGGL(warp_planes_kernel<SNERF_WARP_BILINEAR>, grid, block, 0, s, src, planes, *map, min_valid, tiles_x, n_tiles, dst, stats);
      break;
    case SNERF_WARP_AVERAGE:
      hipLaunchKernelGGL(warp_planes_kernel<SNERF_WARP_AVERAGE>, grid, block, 0, s, src, planes, *map, min_valid, tiles_x, n_tiles, dst, stats);
      break;
    case SNERF_WARP_MIN:
      hipLaunchKernelGGL(warp_planes_kernel<SNERF_WARP_MIN>, grid, block, 0, s, src, planes, *map, min_valid, tiles_x, n_tiles, dst, stats);
      break;
    default:
      hipLaunchKernelGGL(warp_planes_kernel<SNERF_WARP_MAX>, grid, block, 0, s, src, planes, *map, min_valid, tiles_x, n_tiles, dst, stats);
      break;
  }
  SNERF_LAUNCH_CHECK();
  return SNERF_OK;
}

extern "C" int snerf_warp_labels(const unsigned char* src, const SnerfWarpMap* map, int method, unsigned char* dst,
                                 unsigned long long* stats, void* stream) {
  const char* who = "snerf_warp_labels";
  if (!src || !map || !dst || !stats) { set_error("%s: null pointer", who); return SNERF_ERR_NULL; }
  if (src == dst) { set_error("%s: dst must not alias src", who); return SNERF_ERR_BAD_DESC; }
  if (method != SNERF_WARP_NEAREST && method != SNERF_WARP_MODE) {
    set_error("%s: method = %d is neither NEAREST (0) nor MODE (5)", who, method);
    return SNERF_ERR_BAD_DESC;
  }
  if (!warp_map_ok(who, map, method == SNERF_WARP_MODE)) return SNERF_ERR_BAD_DESC;
  const hipStream_t s = (hipStream_t)stream;
  if (method == SNERF_WARP_NEAREST) {
    int tiles_x;
    const long long n_tiles = warp_tiles(map, &tiles_x);
    hipLaunchKernelGGL(warp_labels_nearest_kernel, dim3(blocks_for(n_tiles, 1, WARP_MAX_BLOCKS)), dim3(WARP_THREADS), 0, s, src, *map, tiles_x,
                       n_tiles, dst, stats);
  } else {
    const long long cells = (long long)map->dst_h * map->dst_w;
    hipLaunchKernelGGL(warp_labels_mode_kernel, dim3(blocks_for(cells, WARP_WAVES, WARP_MAX_BLOCKS)), dim3(WARP_THREADS), 0, s, src, *map, cells,
                       dst, stats);
  }
  SNERF_LAUNCH_CHECK();
  return SNERF_OK;
}
