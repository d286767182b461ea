// Solar potential on the DSM lattice: horizon planes (one Amanatides-Woo march per cell and azimuth sector, the steepest slope seen),
// the sky-view factor from those planes, and a table of suns tested against them (direct irradiation and lit counts).  The spec is
// include/snerf_solar.h and DESIGN.md section 5zb.
//   - fp64, evaluated operation by operation (no fused multiply-adds in this file), only + - * /, comparisons and integer work: the
//     host evaluates every transcendental, so tests/solar_numpy.py reproduces every word bit for bit (see the note in dsm_march.h);
//   - the horizon's march is the walk of dsm_march.h.  A workgroup is one 64 x 4 tile of cells under ONE direction: a wave is 64
//     neighbouring cells of a row, so the parallel marches read neighbouring addresses of the height field;
//   - the slope of a step is a division; a step skips it when a product proves that the quotient cannot exceed the best so far, and
//     a march ends when the same product proves that of every altitude up to z_top.  Neither changes a bit (solar_cannot_exceed);
//   - svf and irradiate are one thread per cell over planes read sector by sector: every load is coalesced.
// No allocation, no copy and no host synchronisation; every entry runs on the caller's stream.
#include "dsm_march.h"
#include "lattice.h"
#include "reduce.h"
#include "../../include/snerf_solar.h"

#pragma clang fp contract(off)

namespace snerf {

constexpr int SOLAR_TILE_X = 64, SOLAR_TILE_Y = 4;
constexpr int SOLAR_THREADS = SOLAR_TILE_X * SOLAR_TILE_Y;
constexpr unsigned SOLAR_MAX_BLOCKS = 65536;           // tiles beyond it are strided over (a tile's marches differ in length)
constexpr unsigned SOLAR_CELL_MAX_BLOCKS = 16384;      // svf, irradiate: cells beyond it are strided over

// the checked rows of a call, by value in the kernel arguments
struct SolarDirs {
  double row[SNERF_SOLAR_MAX_DIRS][2];
};
struct SolarSuns {
  double row[SNERF_SOLAR_MAX_SUNS][7];
};
static_assert(sizeof(SolarDirs) == 1024 && sizeof(SolarSuns) == 3584, "the kernel arguments stay below 4 KB");

// True only if fl(num / t) <= best is certain, for t > 0 and best the running maximum; false decides nothing.
//   num <= 0 <= best: the quotient is <= 0.
//   num > 0, best > 0: q = fl(num (1 + 2^-50)) >= num (1 + 2^-50)(1 - 2^-53) > num (1 + 2^-51) and p = fl(best t) <= best t (1 + 2^-53)
//   while p is normal, so q <= p gives num < best t, num / t < best, and rounding is monotone.  A NaN or infinite num fails both tests.
__device__ __forceinline__ bool solar_cannot_exceed(double num, double p, double best) {
  if (num <= 0.0) return best >= 0.0;
  return num * 1.0000000000000009 <= p && p > 1e-280;
}

__global__ __launch_bounds__(SOLAR_THREADS) void solar_horizon_kernel(const float* __restrict__ dsm, int h, int w, int tiles_x,
                                                                      long long tiles_per_dir, long long n_tiles, SolarDirs dirs,
                                                                      double bias, double z_top, double max_dist,
                                                                      float* __restrict__ horizon_out) {
  for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    int k, i0, j0;
    if (!march_tile_cell<SOLAR_TILE_X, SOLAR_TILE_Y>(tile, tiles_x, tiles_per_dir, h, w, &k, &i0, &j0)) continue;
    const long long cell = (long long)j0 * w + i0, o = ((long long)k * h + j0) * w + i0;
    const double start = (double)dsm[cell];
    if (start != start) {
      horizon_out[o] = __builtin_nanf("");
      continue;
    }
    const double h0 = start + bias;
    const double top = z_top - h0;                     // no altitude <= z_top gives a larger numerator (rounding is monotone)
    double best = -__builtin_inf();
    DsmMarch m(h, w, i0, j0, dirs.row[k][0], dirs.row[k][1]);
    while (m.next()) {                                                       // a. left the window
      const double t = m.t;
      if (t > max_dist) break;                                               // b. beyond the search distance
      const double p = best * t;                                             // -inf until something was tested: both tests then fail
      if (top >= 0.0 && solar_cannot_exceed(top, p, best)) break;            // nothing from here on can raise best (t only grows)
      const double num = (double)dsm[(long long)m.j * w + m.i] - h0;
      if (solar_cannot_exceed(num, p, best)) continue;
      const double sl = num / t;                                             // c. false for a NaN cell
      if (sl > best) best = sl;
    }
    horizon_out[o] = (float)best;
  }
}

__global__ __launch_bounds__(256) void solar_svf_kernel(const float* __restrict__ horizon, int n_dirs, long long cells, double res,
                                                        float* __restrict__ svf_out) {
  for (long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x; c < cells; c += (long long)gridDim.x * blockDim.x) {
    const float first = horizon[c];
    double acc = 0.0;
    for (int d = 0; d < n_dirs; ++d) {
      double T = (double)horizon[(long long)d * cells + c] / res;
      if (!(T > 0.0)) T = 0.0;
      acc = acc + 1.0 / (1.0 + T * T);
    }
    svf_out[c] = first != first ? __builtin_nanf("") : (float)(acc / (double)n_dirs);
  }
}

__global__ __launch_bounds__(256) void solar_irradiate_kernel(const float* __restrict__ horizon, int n_dirs, long long cells,
                                                              const float* __restrict__ slope_e, const float* __restrict__ slope_n,
                                                              SolarSuns suns, int n_suns, double* __restrict__ direct_acc,
                                                              unsigned int* __restrict__ lit_count) {
  for (long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x; c < cells; c += (long long)gridDim.x * blockDim.x) {
    const float first = horizon[c];
    if (first != first) {
      direct_acc[c] = __builtin_nan("");
      continue;
    }
    const double gx = slope_e ? (double)slope_e[c] : 0.0, gy = slope_n ? (double)slope_n[c] : 0.0;
    double a = direct_acc[c];
    unsigned int n = lit_count[c];
    for (int k = 0; k < n_suns; ++k) {
      const int sector = (int)suns.row[k][0];
      const double frac = suns.row[k][1], rise = suns.row[k][2], east = suns.row[k][3], north = suns.row[k][4], up = suns.row[k][5],
                   weight = suns.row[k][6];
      double Hk = (double)horizon[(long long)sector * cells + c];
      if (frac != 0.0) {
        const int next = sector + 1 == n_dirs ? 0 : sector + 1;
        Hk = ((1.0 - frac) * Hk) + (frac * (double)horizon[(long long)next * cells + c]);
      }
      const bool lit = rise >= Hk;
      const double ci = (up - (gx * east)) - (gy * north);
      a = a + ((lit && ci > 0.0) ? ci * weight : 0.0);
      n += lit ? 1u : 0u;
    }
    direct_acc[c] = (gx != gx || gy != gy) ? __builtin_nan("") : a;
    lit_count[c] = n;
  }
}

}  // namespace snerf

using namespace snerf;

extern "C" int snerf_solar_horizon(const float* dsm, int h, int w, const double* dirs_host, int n_dirs, double bias, double z_top,
                                   double max_dist, float* horizon_out, void* stream) {
  if (!dsm || !dirs_host || !horizon_out) { set_error("snerf_solar_horizon: null pointer"); return SNERF_ERR_NULL; }
  if (!lattice_cells_ok("snerf_solar_horizon", h, w)) return SNERF_ERR_BAD_DESC;
  if (n_dirs < 1 || n_dirs > SNERF_SOLAR_MAX_DIRS) {
    set_error("snerf_solar_horizon: n_dirs = %d outside [1, %d]", n_dirs, SNERF_SOLAR_MAX_DIRS);
    return SNERF_ERR_BAD_DESC;
  }
  if (!__builtin_isfinite(bias)) { set_error("snerf_solar_horizon: bias must be finite"); return SNERF_ERR_BAD_DESC; }
  if (z_top != z_top) { set_error("snerf_solar_horizon: z_top is NaN"); return SNERF_ERR_BAD_DESC; }
  if (!(max_dist > 0.0)) { set_error("snerf_solar_horizon: max_dist = %.17g must be > 0 (+inf: no bound)", max_dist); return SNERF_ERR_BAD_DESC; }
  SolarDirs dirs = {};
  for (int k = 0; k < n_dirs; ++k) {
    const double* r = dirs_host + 2 * k;
    if (!unit_row_ok("snerf_solar_horizon", "direction", k, r, 2, 0, 2)) return SNERF_ERR_BAD_DESC;
    dirs.row[k][0] = r[0];
    dirs.row[k][1] = r[1];
  }
  const MarchTiles m = march_tiles(h, w, SOLAR_TILE_X, SOLAR_TILE_Y, n_dirs);
  hipLaunchKernelGGL(solar_horizon_kernel, dim3(blocks_for(m.n_tiles, 1, SOLAR_MAX_BLOCKS)), dim3(SOLAR_THREADS), 0, (hipStream_t)stream,
                     dsm, h, w, m.tiles_x, m.tiles_per_plane, m.n_tiles, dirs, bias, z_top, max_dist, horizon_out);
  SNERF_LAUNCH_CHECK();
  return SNERF_OK;
}

extern "C" int snerf_solar_svf(const float* horizon, int n_dirs, int h, int w, double res, float* svf_out, void* stream) {
  if (!horizon || !svf_out) { set_error("snerf_solar_svf: null pointer"); return SNERF_ERR_NULL; }
  if (!lattice_cells_ok("snerf_solar_svf", h, w)) return SNERF_ERR_BAD_DESC;
  if (n_dirs < 1 || n_dirs > SNERF_SOLAR_MAX_SECTORS) {
    set_error("snerf_solar_svf: n_dirs = %d outside [1, %d]", n_dirs, SNERF_SOLAR_MAX_SECTORS);
    return SNERF_ERR_BAD_DESC;
  }
  if (!(res > 0.0) || !__builtin_isfinite(res)) { set_error("snerf_solar_svf: res > 0 and finite required"); return SNERF_ERR_BAD_DESC; }
  const long long cells = (long long)h * w;
  hipLaunchKernelGGL(solar_svf_kernel, dim3(blocks_for(cells, 256, SOLAR_CELL_MAX_BLOCKS)), dim3(256), 0, (hipStream_t)stream, horizon,
                     n_dirs, cells, res, svf_out);
  SNERF_LAUNCH_CHECK();
  return SNERF_OK;
}

extern "C" int snerf_solar_irradiate(const float* horizon, int n_dirs, int h, int w, const float* slope_e, const float* slope_n,
                                     const double* suns_host, int n_suns, double* direct_acc, unsigned int* lit_count, void* stream) {
  if (!horizon || !suns_host || !direct_acc || !lit_count) { set_error("snerf_solar_irradiate: null pointer"); return SNERF_ERR_NULL; }
  if ((slope_e == nullptr) != (slope_n == nullptr)) {
    set_error("snerf_solar_irradiate: slope_e and slope_n are both null or both set");
    return SNERF_ERR_NULL;
  }
  if (!lattice_cells_ok("snerf_solar_irradiate", h, w)) return SNERF_ERR_BAD_DESC;
  if (n_dirs < 1 || n_dirs > SNERF_SOLAR_MAX_SECTORS) {
    set_error("snerf_solar_irradiate: n_dirs = %d outside [1, %d]", n_dirs, SNERF_SOLAR_MAX_SECTORS);
    return SNERF_ERR_BAD_DESC;
  }
  if (n_suns < 1 || n_suns > SNERF_SOLAR_MAX_SUNS) {
    set_error("snerf_solar_irradiate: n_suns = %d outside [1, %d]", n_suns, SNERF_SOLAR_MAX_SUNS);
    return SNERF_ERR_BAD_DESC;
  }
  SolarSuns suns = {};
  for (int k = 0; k < n_suns; ++k) {
    const double* r = suns_host + 7 * k;
    if (!unit_row_ok("snerf_solar_irradiate", "sun", k, r, 7, 3, 3)) return SNERF_ERR_BAD_DESC;
    if (!(r[0] >= 0.0 && r[0] < (double)n_dirs) || r[0] != (double)(int)r[0]) {
      set_error("snerf_solar_irradiate: sun %d: sector = %.17g is no integer of [0, %d)", k, r[0], n_dirs);
      return SNERF_ERR_BAD_DESC;
    }
    if (!(r[1] >= 0.0 && r[1] < 1.0)) { set_error("snerf_solar_irradiate: sun %d: frac = %.17g outside [0, 1)", k, r[1]); return SNERF_ERR_BAD_DESC; }
    if (!(r[2] > 0.0)) { set_error("snerf_solar_irradiate: sun %d: rise = %.17g must be > 0", k, r[2]); return SNERF_ERR_BAD_DESC; }
    if (!(r[5] > 0.0)) { set_error("snerf_solar_irradiate: sun %d: up = %.17g must be > 0", k, r[5]); return SNERF_ERR_BAD_DESC; }
    if (!(r[6] >= 0.0)) { set_error("snerf_solar_irradiate: sun %d: weight = %.17g must be >= 0", k, r[6]); return SNERF_ERR_BAD_DESC; }
    for (int c = 0; c < 7; ++c) suns.row[k][c] = r[c];
  }
  const long long cells = (long long)h * w;
  hipLaunchKernelGGL(solar_irradiate_kernel, dim3(blocks_for(cells, 256, SOLAR_CELL_MAX_BLOCKS)), dim3(256), 0, (hipStream_t)stream,
                     horizon, n_dirs, cells, slope_e, slope_n, suns, n_suns, direct_acc, lit_count);
  SNERF_LAUNCH_CHECK();
  return SNERF_OK;
}
