// Cast shadows on the DSM lattice: the shadow a height field casts under a sun (one Amanatides-Woo march per cell and sun), and
// the agreement of a learned shadow map with the cast mask (integer counts and quantised integer sums).  The spec is
// the cast-shadow section of include/snerf_hip.h and DESIGN.md section 5o.
//   - the march is the walk of dsm_march.h (fp64, operation by operation, no fused multiply-add anywhere in this file: see the note
//     there), so tests/shadow_numpy.py reproduces it bit for bit; a workgroup is one 16 x 16 tile of cells under ONE sun, whose
//     height field lives in L2 (4 MB at 1024 x 1024);
//   - the agreement words are folded per wave with shuffles, then one 64-bit integer atomic add per wave and word: exact and
//     independent of the launch order.
// No allocation, no copy and no host synchronisation; both entries run on the caller's stream.
#include "dsm_march.h"
#include "lattice.h"
#include "reduce.h"
#include "../../include/snerf_hip.h"

#pragma clang fp contract(off)

namespace snerf {

constexpr int SHADOW_TILE = 16;
constexpr int SHADOW_THREADS = SHADOW_TILE * SHADOW_TILE;
constexpr unsigned SHADOW_MAX_BLOCKS = 65536;          // tiles beyond it are strided over (a tile's marches differ in length)
constexpr unsigned SHADOW_AGREE_MAX_BLOCKS = 4096;     // per sun

// the checked rows of a call, by value in the kernel arguments
struct ShadowSuns {
  double row[SNERF_SHADOW_MAX_SUNS][3];
};
static_assert(sizeof(ShadowSuns) == 1536, "the kernel arguments stay far below 4 KB");

__global__ __launch_bounds__(SHADOW_THREADS) void shadow_cast_kernel(const float* __restrict__ dsm, int h, int w, int tiles_x,
                                                                     long long tiles_per_sun, long long n_tiles, ShadowSuns suns,
                                                                     double bias, double z_top, unsigned char* __restrict__ lit_out,
                                                                     float* __restrict__ dist_out) {
  for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    int k, i0, j0;
    if (!march_tile_cell<SHADOW_TILE, SHADOW_TILE>(tile, tiles_x, tiles_per_sun, h, w, &k, &i0, &j0)) continue;
    const long long cell = (long long)j0 * w + i0, o = ((long long)k * h + j0) * w + i0;
    const double rise = suns.row[k][2];
    const double start = (double)dsm[cell];
    unsigned char lit = 1;
    float dist = __builtin_nanf("");
    if (start != start) {
      lit = SNERF_SHADOW_UNKNOWN;
    } else {
      const double h0 = start + bias;
      DsmMarch m(h, w, i0, j0, suns.row[k][0], suns.row[k][1]);
      while (m.next()) {                                                     // a. left the window: lit
        const double hr = h0 + rise * m.t;                                    // two roundings
        if (hr > z_top) break;                                               // b. above everything: lit
        if ((double)dsm[(long long)m.j * w + m.i] > hr) {                    // c. blocked (false for a NaN cell)
          lit = 0;
          dist = (float)m.t;
          break;
        }
      }
    }
    lit_out[o] = lit;
    if (dist_out) dist_out[o] = dist;
  }
}

// blockIdx.y = the sun; the workgroups of a sun stride over its cells
__global__ __launch_bounds__(SHADOW_THREADS) void shadow_agreement_kernel(const float* __restrict__ sun, const unsigned char* __restrict__ lit,
                                                                          const unsigned char* __restrict__ valid, long long cells,
                                                                          double threshold, unsigned long long* __restrict__ acc) {
  const long long base = (long long)blockIdx.y * cells;
  unsigned long long n[7] = {0, 0, 0, 0, 0, 0, 0};
  for (long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x; c < cells; c += (long long)gridDim.x * blockDim.x) {
    const unsigned char l = lit[base + c];
    const float v = sun[base + c];
    if (l > 1 || (valid && valid[c] == 0) || !__builtin_isfinite(v)) { n[4]++; continue; }
    const int pred_lit = (double)v >= threshold;
    double q = (double)v * 16777216.0;                                       // exact
    q = q > 4611686018427387904.0 ? 4611686018427387904.0 : (q < -4611686018427387904.0 ? -4611686018427387904.0 : q);
    const unsigned long long qi = (unsigned long long)llrint(q);             // two's complement: the adds wrap as int64 sums do
    const unsigned long long on = l, pl = (unsigned long long)pred_lit;      // l is 0 or 1 here
    n[0] += on & pl;
    n[1] += on & (pl ^ 1);
    n[2] += (on ^ 1) & pl;
    n[3] += (on ^ 1) & (pl ^ 1);
    n[5] += on ? qi : 0;
    n[6] += on ? 0 : qi;
  }
  unsigned long long* row = acc + (long long)blockIdx.y * 8;
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    const unsigned long long v = wave_reduce(n[k], OpSum());
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(&row[k], v);
  }
}

}  // namespace snerf

using namespace snerf;

extern "C" int snerf_shadow_cast(const float* dsm, int h, int w, const double* suns_host, int n_suns, double bias, double z_top,
                                 unsigned char* lit_out, float* dist_out, void* stream) {
  if (!dsm || !suns_host || !lit_out) { set_error("snerf_shadow_cast: null pointer"); return SNERF_ERR_NULL; }
  if (!lattice_cells_ok("snerf_shadow_cast", h, w)) return SNERF_ERR_BAD_DESC;
  if (n_suns < 1 || n_suns > SNERF_SHADOW_MAX_SUNS) {
    set_error("snerf_shadow_cast: n_suns = %d outside [1, %d]", n_suns, SNERF_SHADOW_MAX_SUNS);
    return SNERF_ERR_BAD_DESC;
  }
  if (!__builtin_isfinite(bias)) { set_error("snerf_shadow_cast: bias must be finite"); return SNERF_ERR_BAD_DESC; }
  if (z_top != z_top) { set_error("snerf_shadow_cast: z_top is NaN"); return SNERF_ERR_BAD_DESC; }
  ShadowSuns suns = {};
  for (int k = 0; k < n_suns; ++k) {
    const double* r = suns_host + 3 * k;
    if (!unit_row_ok("snerf_shadow_cast", "sun", k, r, 3, 0, 2)) return SNERF_ERR_BAD_DESC;
    const double ux = r[0], uy = r[1], rise = r[2];
    if (!(rise > 0.0)) { set_error("snerf_shadow_cast: sun %d: rise = %.17g must be > 0", k, rise); return SNERF_ERR_BAD_DESC; }
    suns.row[k][0] = ux;
    suns.row[k][1] = uy;
    suns.row[k][2] = rise;
  }
  const MarchTiles m = march_tiles(h, w, SHADOW_TILE, SHADOW_TILE, n_suns);
  hipLaunchKernelGGL(shadow_cast_kernel, dim3(blocks_for(m.n_tiles, 1, SHADOW_MAX_BLOCKS)), dim3(SHADOW_THREADS), 0, (hipStream_t)stream,
                     dsm, h, w, m.tiles_x, m.tiles_per_plane, m.n_tiles, suns, bias, z_top, lit_out, dist_out);
  SNERF_LAUNCH_CHECK();
  return SNERF_OK;
}

extern "C" int snerf_shadow_agreement(const float* sun, const unsigned char* lit, const unsigned char* valid, long long cells,
                                      int n_suns, double threshold, unsigned long long* acc, void* stream) {
  if (!sun || !lit || !acc) { set_error("snerf_shadow_agreement: null pointer"); return SNERF_ERR_NULL; }
  if (cells < 1 || cells > (1LL << 53)) { set_error("snerf_shadow_agreement: cells must be >= 1"); return SNERF_ERR_BAD_DESC; }
  if (n_suns < 1 || n_suns > SNERF_SHADOW_MAX_SUNS) {
    set_error("snerf_shadow_agreement: n_suns = %d outside [1, %d]", n_suns, SNERF_SHADOW_MAX_SUNS);
    return SNERF_ERR_BAD_DESC;
  }
  if (!__builtin_isfinite(threshold)) { set_error("snerf_shadow_agreement: threshold must be finite"); return SNERF_ERR_BAD_DESC; }
  hipLaunchKernelGGL(shadow_agreement_kernel, dim3(blocks_for(cells, SHADOW_THREADS, SHADOW_AGREE_MAX_BLOCKS), n_suns),
                     dim3(SHADOW_THREADS), 0, (hipStream_t)stream, sun, lit, valid, cells, threshold, acc);
  SNERF_LAUNCH_CHECK();
  return SNERF_OK;
}
