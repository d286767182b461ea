// A 3-D segment against the prism height field of a DSM window: one Amanatides-Woo walk per segment, reporting where it first
// touches the surface.  The spec is include/snerf_raycast.h and DESIGN.md section 5v.
//   - fp64, evaluated operation by operation (no fused multiply-adds in this file), with only + - * /, floor, comparisons and
//     integer work, so tests/raycast_numpy.py reproduces it bit for bit.  Plain operators under `fp contract(off)`, not
//     __dadd_rn / __dmul_rn: see the note at the top of shadow.hip;
//   - one thread per segment: the rays of a chunk are neighbours and read neighbouring cells of the height field, which is read
//     straight from memory (it lives in L2: 4 MB at 1024 x 1024);
//   - a crossing parameter is recomputed from the boundary's integer coordinate at every step, so the walk cannot drift.
// No allocation, no copy and no host synchronisation; the entry runs on the caller's stream.
#include "lattice.h"
#include "reduce.h"
#include "../../include/snerf_raycast.h"

#pragma clang fp contract(off)

namespace snerf {

constexpr int RAYCAST_THREADS = 256;
constexpr unsigned RAYCAST_MAX_BLOCKS = 65536;         // segments beyond it are strided over

// one axis of the slab clip of step 3; false: the segment misses the window on this axis
__device__ __forceinline__ bool clip_axis(double c0, double dc, double size, double& t0, double& t1) {
  if (dc == 0.0) return c0 >= 0.0 && c0 < size;
  const double ta = (0.0 - c0) / dc, tb = (size - c0) / dc;
  const double lo = ta < tb ? ta : tb, hi = ta < tb ? tb : ta;
  if (lo > t0) t0 = lo;
  if (hi < t1) t1 = hi;
  return true;
}

// floor(c) clamped into [0, size - 1], size >= 1
__device__ __forceinline__ int entry_cell(double c, int size) {
  const double f = floor(c);
  return f >= 0.0 ? (f <= (double)(size - 1) ? (int)f : size - 1) : 0;
}

__global__ __launch_bounds__(RAYCAST_THREADS) void dsm_segment_hit_kernel(const double* __restrict__ p0, const double* __restrict__ p1,
                                                                          long long n, SnerfDsmGrid g, const float* __restrict__ dsm,
                                                                          double bias, double* __restrict__ s_out,
                                                                          unsigned char* __restrict__ state_out, int* __restrict__ cell_out) {
  const int w = g.out_w, h = g.out_h;
  const double W = (double)w, H = (double)h, ioff = (double)g.ioff, joff = (double)g.joff;
  const long long max_steps = (long long)w + h + 2;
  const double inf = __builtin_inf(), nan = __builtin_nan("");
  for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (long long)gridDim.x * blockDim.x) {
    const double e0 = p0[3 * r], n0 = p0[3 * r + 1], a0 = p0[3 * r + 2];
    const double e1 = p1[3 * r], n1 = p1[3 * r + 1], a1 = p1[3 * r + 2];
    double s = nan;
    unsigned char state = SNERF_HIT_BAD;
    int cell = -1;
    if (__builtin_isfinite(e0) && __builtin_isfinite(n0) && __builtin_isfinite(a0) && __builtin_isfinite(e1) && __builtin_isfinite(n1) &&
        __builtin_isfinite(a1)) {
      const double x0 = (e0 - g.xoff) / g.res - ioff, y0 = (g.yoff - n0) / g.res - joff;
      const double x1 = (e1 - g.xoff) / g.res - ioff, y1 = (g.yoff - n1) / g.res - joff;
      const double dx = x1 - x0, dy = y1 - y0, da = a1 - a0;
      state = SNERF_HIT_OUTSIDE;
      double s_a = 0.0;
      int i = 0, j = 0;
      bool enters = true;
      if (x0 >= 0.0 && x0 < W && y0 >= 0.0 && y0 < H) {
        i = (int)floor(x0);
        j = (int)floor(y0);
      } else {
        double t0 = 0.0, t1 = 1.0;
        enters = clip_axis(x0, dx, W, t0, t1) && clip_axis(y0, dy, H, t0, t1) && !(t0 > t1);
        if (enters) {
          s_a = t0;
          i = entry_cell(x0 + dx * t0, w);
          j = entry_cell(y0 + dy * t0, h);
        }
      }
      if (enters) {
        const int stepx = dx > 0.0 ? 1 : -1, stepy = dy > 0.0 ? 1 : -1;
        const int aheadx = dx > 0.0 ? 1 : 0, aheady = dy > 0.0 ? 1 : 0;
        bool first = true;
        for (long long step = 0; step < max_steps; ++step) {
          const double s_x = dx == 0.0 ? inf : ((double)(i + aheadx) - x0) / dx;
          const double s_y = dy == 0.0 ? inf : ((double)(j + aheady) - y0) / dy;
          const bool x_steps = s_x <= s_y;
          const double s_next = x_steps ? s_x : s_y;
          double s_b = s_next < 1.0 ? s_next : 1.0;
          if (s_b < s_a) s_b = s_a;
          const double hc = (double)dsm[(long long)j * w + i] + bias;
          if (a0 + da * s_a <= hc) {
            s = s_a;
            state = first ? SNERF_HIT_START : SNERF_HIT_WALL;
            cell = j * w + i;
            break;
          }
          if (a0 + da * s_b <= hc) {
            const double t = (hc - a0) / da;
            s = t < s_a ? s_a : (t > s_b ? s_b : t);
            state = SNERF_HIT_TOP;
            cell = j * w + i;
            break;
          }
          if (s_next >= 1.0) {
            state = SNERF_HIT_END;
            break;
          }
          if (x_steps) i += stepx; else j += stepy;
          if (i < 0 || i >= w || j < 0 || j >= h) break;                       // left the window: OUTSIDE
          s_a = s_b;
          first = false;
        }
      }
    }
    s_out[r] = s;
    state_out[r] = state;
    if (cell_out) cell_out[r] = cell;
  }
}

}  // namespace snerf

using namespace snerf;

extern "C" int snerf_dsm_segment_hit(const double* p0, const double* p1, long long n, const SnerfDsmGrid* grid, const float* dsm,
                                     double bias, double* s_out, unsigned char* state_out, int* cell_out, void* stream) {
  const char* who = "snerf_dsm_segment_hit";
  if (!p0 || !p1 || !grid || !dsm || !s_out || !state_out) { set_error("%s: null pointer", who); return SNERF_ERR_NULL; }
  if (n < 0 || n > LATTICE_MAX_POINTS) { set_error("%s: n = %lld outside [0, 2^31]", who, n); return SNERF_ERR_BAD_DESC; }
  if (!lattice_grid_ok(who, grid) || !lattice_window_fits_int32(who, grid)) return SNERF_ERR_BAD_DESC;
  if (!lattice_window_cells_ok(who, grid)) return SNERF_ERR_BAD_DESC;
  if (!__builtin_isfinite(bias)) { set_error("%s: bias must be finite", who); return SNERF_ERR_BAD_DESC; }
  if (n == 0) return SNERF_OK;
  hipLaunchKernelGGL(dsm_segment_hit_kernel, dim3(blocks_for(n, RAYCAST_THREADS, RAYCAST_MAX_BLOCKS)), dim3(RAYCAST_THREADS), 0,
                     (hipStream_t)stream, p0, p1, n, *grid, dsm, bias, s_out, state_out, cell_out);
  SNERF_LAUNCH_CHECK();
  return SNERF_OK;
}
