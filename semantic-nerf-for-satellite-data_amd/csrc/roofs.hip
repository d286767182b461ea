// Roof planes on the map: per-cell surface gradients and orientation codes (a least-squares plane over the cell's neighbours of the
// same building, integer sums and an fp64 tail), facets as the connected components of equal tags (the launches of
// csrc/link_kernels.h over the walk of csrc/objects_walk.h), per-facet moment sums and the distance of every facet cell from its
// facet's plane (a reduction inside the wave over the lanes that share a facet, then one lane's integer atomics, as
// snerf_objects_stats folds).  The spec is include/snerf_roofs.h and DESIGN.md section 5z; tests/roofs_numpy.py restates it.
// Every loop is counted by h, w, the radius or a fixed bound, except the union-find walk with its guards.
#include "lattice.h"
#include "link_kernels.h"
#include "reduce.h"
#include "roof_plane.h"
#include "../../include/snerf_roofs.h"
#include "../../include/snerf_terrain.h"

#include <limits.h>

// the fp64 tails are restated operation by operation in numpy: no fused multiply-add (as csrc/terrain.hip)
#pragma clang fp contract(off)

namespace snerf {

constexpr int ROOF_TILE_W = 64;              // one wave per tile row: consecutive lanes on consecutive columns
constexpr int ROOF_TILE_H = 8;
constexpr int ROOF_TILE_THREADS = ROOF_TILE_W * ROOF_TILE_H;
constexpr int ROOF_TILE_WAVES = ROOF_TILE_THREADS / 64;
constexpr int ROOF_THREADS = 256;            // the per-facet folds: one thread per cell of the band
constexpr unsigned ROOF_MAX_BLOCKS = 65536;
constexpr long long ROOF_DK_LIMIT = 1LL << 24;

// ---- normals -----------------------------------------------------------------------------------------------------------------------
// A workgroup of 64 x 8 threads takes a 64 x 8 tile.  It stages (key, id) pairs of the tile and its halo of R cells in LDS, a hole
// key and id -1 beyond the raster, a hole key stored as SNERF_TERRAIN_HOLE and an id outside [0, K] as 0: the window loop then needs
// no test but "same id, valid key".  The pairs are 8 bytes, so a wave's read of one window offset is one conflict-free ds_read_b64
// over consecutive addresses.  The loop bounds are compile-time constants: it unrolls, and di, dj fold into the instructions.
template <int R>
__global__ __launch_bounds__(ROOF_TILE_THREADS) void roofs_normals_kernel(const int* __restrict__ key, const int* __restrict__ ids, int h,
                                                                          int w, int K, double f, double cos0, double sin0,
                                                                          double tan2_flat, double tan2_wall, float* __restrict__ slope_e,
                                                                          float* __restrict__ slope_n, unsigned char* __restrict__ code,
                                                                          int* __restrict__ tag, unsigned long long* __restrict__ stats) {
  constexpr int TW = ROOF_TILE_W + 2 * R, TH = ROOF_TILE_H + 2 * R;
  __shared__ int2 tile[TH * TW];
  __shared__ unsigned counts[ROOF_TILE_WAVES][4];
  const int tx = threadIdx.x, ty = threadIdx.y, t = ty * ROOF_TILE_W + tx;
  const int x0 = blockIdx.x * ROOF_TILE_W, y0 = blockIdx.y * ROOF_TILE_H;
  for (int s = t; s < TH * TW; s += ROOF_TILE_THREADS) {
    const int sy = s / TW, sx = s - sy * TW;
    const int gx = x0 - R + sx, gy = y0 - R + sy;
    int2 v = make_int2(SNERF_TERRAIN_HOLE, -1);
    if (gx >= 0 && gx < w && gy >= 0 && gy < h) {
      const long long g = (long long)gy * w + gx;
      const int k = key[g], id = ids[g];
      v.x = roof_valid(k) ? k : SNERF_TERRAIN_HOLE;
      v.y = (id < 0 || id > K) ? 0 : id;
    }
    tile[s] = v;
  }
  __syncthreads();
  const int i = x0 + tx, j = y0 + ty;
  unsigned is_object = 0, has_normal = 0, degenerate = 0, hole = 0;
  if (i < w && j < h) {
    const int2 centre = tile[(ty + R) * TW + tx + R];
    const int id = centre.y;
    unsigned c = SNERF_ROOFS_NONE;
    float se = __int_as_float(0x7fc00000), sn = __int_as_float(0x7fc00000);
    if (id > 0) {
      is_object = 1;
      if (centre.x == SNERF_TERRAIN_HOLE) {
        c = SNERF_ROOFS_HOLE;
        hole = 1;
      } else {
        int n = 0, sx = 0, sy = 0, sxx = 0, sxy = 0, syy = 0;
        long long sd = 0, sxd = 0, syd = 0;
#pragma unroll
        for (int dj = -R; dj <= R; ++dj) {
#pragma unroll
          for (int di = -R; di <= R; ++di) {
            const int2 g = tile[(ty + R + dj) * TW + tx + R + di];
            if (g.y == id && g.x != SNERF_TERRAIN_HOLE) {
              const long long d = (long long)g.x - centre.x;
              n += 1;
              sx += di;
              sy += dj;
              sxx += di * di;
              sxy += di * dj;
              syy += dj * dj;
              sd += d;
              sxd += di * d;
              syd += dj * d;
            }
          }
        }
        // every cofactor lies below 2^20 and D below 2^29 (include/snerf_roofs.h): int64 holds the numerators with room to spare
        const long long N = n, Sx = sx, Sy = sy, Sxx = sxx, Sxy = sxy, Syy = syy;
        const long long c00 = Sxx * Syy - Sxy * Sxy, c01 = Sxy * Sy - Sx * Syy, c02 = Sx * Sxy - Sxx * Sy;
        const long long c11 = N * Syy - Sy * Sy, c12 = Sx * Sy - N * Sxy, c22 = N * Sxx - Sx * Sx;
        const long long D = N * c00 + Sx * c01 + Sy * c02;
        if (D <= 0) {
          c = SNERF_ROOFS_DEGENERATE;
          degenerate = 1;
        } else {
          const long long Nx = c01 * sd + c11 * sxd + c12 * syd, Ny = c02 * sd + c12 * sxd + c22 * syd;
          const double a = ((double)Nx / (double)D) * f, b = ((double)Ny / (double)D) * f;
          const double ar = (a * cos0) + (b * sin0), br = (b * cos0) - (a * sin0);
          const double ar2 = ar * ar, br2 = br * br;
          const double s2 = ar2 + br2, m = fabs(ar) + fabs(br), m2 = m * m;
          if (s2 <= tan2_flat) c = SNERF_ROOFS_FLAT;
          else if (s2 > tan2_wall) c = SNERF_ROOFS_STEEP;
          else if (m2 < 2.0 * ar2) c = ar > 0.0 ? 7 : 3;
          else if (m2 < 2.0 * br2) c = br > 0.0 ? 1 : 5;
          else c = ar > 0.0 ? (br > 0.0 ? 8 : 6) : (br > 0.0 ? 2 : 4);
          se = (float)a;
          sn = (float)(-b);
          has_normal = 1;
        }
      }
    }
    const long long cell = (long long)j * w + i;
    slope_e[cell] = se;
    slope_n[cell] = sn;
    code[cell] = (unsigned char)c;
    tag[cell] = c <= 8 ? id * 16 + (int)c : -1;
  }
  // the counts: over the wave, then over the workgroup's waves in LDS, then one lane's atomics
  is_object = wave_reduce(is_object, OpSum());
  has_normal = wave_reduce(has_normal, OpSum());
  degenerate = wave_reduce(degenerate, OpSum());
  hole = wave_reduce(hole, OpSum());
  if (tx == 0) {
    counts[ty][0] = is_object;
    counts[ty][1] = has_normal;
    counts[ty][2] = degenerate;
    counts[ty][3] = hole;
  }
  __syncthreads();
  if (t < 4) {
    unsigned long long sum = 0;
#pragma unroll
    for (int wv = 0; wv < ROOF_TILE_WAVES; ++wv) sum += counts[wv][t];
    if (sum) atomicAdd(&stats[t], sum);
  }
}

// ---- link --------------------------------------------------------------------------------------------------------------------------
// what links two cells of a tag plane: the same non-negative tag
struct TagLink {
  const int* tag;
  __device__ __forceinline__ int load(long long c) const { return tag[c]; }
  __device__ __forceinline__ bool member(int t) const { return t >= 0; }
};

// ---- the per-facet folds -------------------------------------------------------------------------------------------------------------
// What both folds read of a cell: its facet (0: none or ignored), its offsets from the facet's root and whether both keys are valid.
struct RoofCell {
  int fid, di, dj, i, j, k;
  long long dk;
  bool bad, keyed;
};
__device__ __forceinline__ RoofCell roof_cell(const int* __restrict__ fids, const int* __restrict__ root, const int* __restrict__ key,
                                              long long c, long long end, int w, long long cells, long long F) {
  RoofCell r = {0, 0, 0, 0, 0, 0, 0, false, false};
  if (c >= end) return r;
  const int fid = fids[c];
  if (fid < 0 || fid > F) { r.bad = true; return r; }
  if (fid == 0) return r;
  const int rt = root[c];
  if (rt < 0 || rt >= cells) { r.bad = true; return r; }
  r.fid = fid;
  r.j = (int)(c / w);
  r.i = (int)(c - (long long)r.j * w);
  const int j0 = rt / w, i0 = rt - j0 * w;
  r.di = r.i - i0;
  r.dj = r.j - j0;
  const int k = key[c], k0 = key[rt];
  r.keyed = roof_valid(k) && roof_valid(k0);
  r.k = k;
  r.dk = (long long)k - k0;
  return r;
}

// One thread per cell of the band.  The wave takes the first lane that still has a facet, ballots the lanes of that facet, reduces
// their values across the wave (the others hold the identities) and lets that lane issue the row's atomics: the sums are integers,
// so the grouping does not show in the words.
__global__ __launch_bounds__(ROOF_THREADS) void roofs_moments_kernel(const int* __restrict__ fids, const int* __restrict__ root,
                                                                     const int* __restrict__ key, const int* __restrict__ tag, int w,
                                                                     long long cells, long long F, long long first, long long end,
                                                                     unsigned long long* __restrict__ rows,
                                                                     unsigned long long* __restrict__ stats) {
  const int lane = threadIdx.x & 63;
  unsigned long long folded = 0, left_out = 0, bad = 0;
  // every thread of a workgroup makes the same number of trips: the wave's ballots and shuffles run with all lanes
  for (long long base = first + (long long)blockIdx.x * blockDim.x; base < end; base += (long long)gridDim.x * blockDim.x) {
    const long long c = base + threadIdx.x;
    const RoofCell r = roof_cell(fids, root, key, c, end, w, cells, F);
    bad += r.bad ? 1 : 0;
    const int id = r.fid;
    const bool take = id > 0 && r.keyed && r.dk > -ROOF_DK_LIMIT && r.dk < ROOF_DK_LIMIT;
    const unsigned n = take ? 1u : 0u, out = (id > 0 && !take) ? 1u : 0u;
    const long long di = take ? r.di : 0, dj = take ? r.dj : 0, dk = take ? r.dk : 0;
    const unsigned min_i = take ? (unsigned)r.i : 0xFFFFFFFFu, max_i = take ? (unsigned)r.i : 0u;
    const unsigned min_j = take ? (unsigned)r.j : 0xFFFFFFFFu, max_j = take ? (unsigned)r.j : 0u;
    const int tg = id > 0 ? tag[c] : 0;
    const unsigned my_tag = tg > 0 ? (unsigned)tg : 0u, my_root = id > 0 ? (unsigned)root[c] : 0u;
    folded += n;
    left_out += out;
    unsigned long long todo = __ballot(id > 0);
    while (todo) {                                           // wave-uniform: `todo` is the same word in every lane
      const int leader = __ffsll((long long)todo) - 1;
      const int group_id = __shfl(id, leader, 64);
      const bool in = id == group_id;                        // (group_id > 0: a lane of `todo`)
      todo &= ~__ballot(in);
      const unsigned r_n = wave_reduce(in ? n : 0u, OpSum());
      const long long r_di = wave_reduce(in ? di : 0ll, OpSum()), r_dj = wave_reduce(in ? dj : 0ll, OpSum());
      const long long r_dk = wave_reduce(in ? dk : 0ll, OpSum());
      const long long r_xx = wave_reduce(in ? di * di : 0ll, OpSum()), r_xy = wave_reduce(in ? di * dj : 0ll, OpSum());
      const long long r_yy = wave_reduce(in ? dj * dj : 0ll, OpSum());
      const long long r_xk = wave_reduce(in ? di * dk : 0ll, OpSum()), r_yk = wave_reduce(in ? dj * dk : 0ll, OpSum());
      const unsigned r_min_i = wave_reduce(in ? min_i : 0xFFFFFFFFu, OpMin()), r_max_i = wave_reduce(in ? max_i : 0u, OpMax());
      const unsigned r_min_j = wave_reduce(in ? min_j : 0xFFFFFFFFu, OpMin()), r_max_j = wave_reduce(in ? max_j : 0u, OpMax());
      const unsigned r_tag = wave_reduce(in ? my_tag : 0u, OpMax()), r_root = wave_reduce(in ? my_root : 0u, OpMax());
      const unsigned r_out = wave_reduce(in ? out : 0u, OpSum());
      if (lane == leader) {
        unsigned long long* row = rows + (long long)(group_id - 1) * SNERF_ROOFS_MOMENT_WORDS;
        if (r_n) {
          atomicAdd(&row[0], (unsigned long long)r_n);
          atomicAdd(&row[1], (unsigned long long)r_di);
          atomicAdd(&row[2], (unsigned long long)r_dj);
          atomicAdd(&row[3], (unsigned long long)r_dk);
          atomicAdd(&row[4], (unsigned long long)r_xx);
          atomicAdd(&row[5], (unsigned long long)r_xy);
          atomicAdd(&row[6], (unsigned long long)r_yy);
          atomicAdd(&row[7], (unsigned long long)r_xk);
          atomicAdd(&row[8], (unsigned long long)r_yk);
          atomicMin(&row[9], (unsigned long long)r_min_i);
          atomicMax(&row[10], (unsigned long long)r_max_i);
          atomicMin(&row[11], (unsigned long long)r_min_j);
          atomicMax(&row[12], (unsigned long long)r_max_j);
        }
        atomicMax(&row[13], (unsigned long long)r_tag);
        atomicMax(&row[14], (unsigned long long)r_root);
        if (r_out) atomicAdd(&row[15], (unsigned long long)r_out);
      }
    }
  }
  folded = wave_reduce(folded, OpSum());
  left_out = wave_reduce(left_out, OpSum());
  bad = wave_reduce(bad, OpSum());
  if (lane == 0) {
    if (folded) atomicAdd(&stats[0], folded);
    if (left_out) atomicAdd(&stats[1], left_out);
    if (bad) atomicAdd(&stats[2], bad);
  }
}

__global__ __launch_bounds__(ROOF_THREADS) void roofs_residuals_kernel(const int* __restrict__ fids, const int* __restrict__ root,
                                                                       const int* __restrict__ key, int w, long long cells, long long F,
                                                                       const double* __restrict__ planes, double q, double unit,
                                                                       long long first, long long end, float* __restrict__ residual,
                                                                       unsigned long long* __restrict__ rows,
                                                                       unsigned long long* __restrict__ stats) {
  const int lane = threadIdx.x & 63;
  unsigned long long with = 0, without = 0, bad = 0;
  for (long long base = first + (long long)blockIdx.x * blockDim.x; base < end; base += (long long)gridDim.x * blockDim.x) {
    const long long c = base + threadIdx.x;
    const RoofCell r = roof_cell(fids, root, key, c, end, w, cells, F);
    bad += r.bad ? 1 : 0;
    int id = 0;                                              // the facet this cell adds to: only with a residual
    float out = __int_as_float(0x7fc00000);
    long long rq = 0;
    unsigned clamped = 0;
    if (r.fid > 0) {
      const double* p = planes + (long long)(r.fid - 1) * 3;
      const double gamma = p[0], alpha = p[1], beta = p[2];
      if (r.keyed && isfinite(gamma) && isfinite(alpha) && isfinite(beta)) {
        const RoofMisfit m = roof_misfit(gamma, alpha, beta, r.di, r.dj, r.dk, unit);      // roof_plane.h: shared with the growth
        out = (float)(q * m.e);
        rq = m.rq;
        clamped = m.clamped;
        id = r.fid;
        with++;
      } else {
        without++;
      }
    }
    if (c < end) residual[c] = out;
    const unsigned long long mag = (unsigned long long)(rq < 0 ? -rq : rq);
    const unsigned biased = id > 0 ? (unsigned)((long long)r.k + 2147483648LL) : 0u;
    unsigned long long todo = __ballot(id > 0);
    while (todo) {                                           // wave-uniform, as above
      const int leader = __ffsll((long long)todo) - 1;
      const int group_id = __shfl(id, leader, 64);
      const bool in = id == group_id;
      todo &= ~__ballot(in);
      const unsigned r_n = wave_reduce(in ? 1u : 0u, OpSum());
      const unsigned long long r_abs = wave_reduce(in ? mag : 0ull, OpSum()), r_sq = wave_reduce(in ? mag * mag : 0ull, OpSum());
      const unsigned long long r_max = wave_reduce(in ? mag : 0ull, OpMax());
      const unsigned r_min_k = wave_reduce(in ? biased : 0xFFFFFFFFu, OpMin()), r_max_k = wave_reduce(in ? biased : 0u, OpMax());
      const unsigned r_clamped = wave_reduce(in ? clamped : 0u, OpSum());
      if (lane == leader) {
        unsigned long long* row = rows + (long long)(group_id - 1) * SNERF_ROOFS_RESIDUAL_WORDS;
        atomicAdd(&row[0], (unsigned long long)r_n);
        if (r_abs) atomicAdd(&row[1], r_abs);
        if (r_sq) atomicAdd(&row[2], r_sq);
        atomicMax(&row[3], r_max);
        atomicMin(&row[4], (unsigned long long)r_min_k);
        atomicMax(&row[5], (unsigned long long)r_max_k);
        if (r_clamped) atomicAdd(&row[6], (unsigned long long)r_clamped);
      }
    }
  }
  with = wave_reduce(with, OpSum());
  without = wave_reduce(without, OpSum());
  bad = wave_reduce(bad, OpSum());
  if (lane == 0) {
    if (with) atomicAdd(&stats[0], with);
    if (without) atomicAdd(&stats[1], without);
    if (bad) atomicAdd(&stats[2], bad);
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
static bool roofs_sizes_ok(const char* who, int h, int w) {
  if (h < 1 || w < 1) { set_error("%s: h and w must be >= 1 (h = %d, w = %d)", who, h, w); return false; }
  if (h > SNERF_ROOFS_MAX_SIDE || w > SNERF_ROOFS_MAX_SIDE) {
    set_error("%s: h and w must be at most %d (h = %d, w = %d)", who, SNERF_ROOFS_MAX_SIDE, h, w);
    return false;
  }
  return true;
}

static bool roofs_count_ok(const char* who, const char* what, long long n) {
  if (n >= 0 && n < SNERF_ROOFS_MAX_OBJECTS) return true;
  set_error("%s: %s must lie in [0, 2^27) (%s = %lld)", who, what, what, n);
  return false;
}

static bool roofs_band_ok(const char* who, int h, int row0, int row1) {
  if (row0 >= 0 && row1 <= h && row0 <= row1) return true;
  set_error("%s: 0 <= row0 <= row1 <= h required (row0 = %d, row1 = %d, h = %d)", who, row0, row1, h);
  return false;
}

static bool roofs_positive(const char* who, const char* what, double v) {
  if (v > 0.0 && isfinite(v)) return true;
  set_error("%s: %s > 0 and finite required (%s = %g)", who, what, what, v);
  return false;
}

static unsigned roofs_blocks(long long n) { return blocks_for(n, ROOF_THREADS, ROOF_MAX_BLOCKS); }

}  // namespace snerf

using namespace snerf;

extern "C" int snerf_roofs_normals(const int* key, const int* ids, int h, int w, long long K, int radius, double q, double res,
                                   double cos0, double sin0, double tan2_flat, double tan2_wall, float* slope_e, float* slope_n,
                                   unsigned char* code, int* tag, unsigned long long* stats, void* stream) {
  const char* who = "snerf_roofs_normals";
  if (!key || !ids || !slope_e || !slope_n || !code || !tag || !stats) { set_error("%s: null pointer", who); return SNERF_ERR_NULL; }
  if (!roofs_sizes_ok(who, h, w) || !roofs_count_ok(who, "K", K)) return SNERF_ERR_BAD_DESC;
  if (radius < 1 || radius > SNERF_ROOFS_MAX_RADIUS) {
    set_error("%s: radius must lie in [1, %d] (radius = %d)", who, SNERF_ROOFS_MAX_RADIUS, radius);
    return SNERF_ERR_BAD_DESC;
  }
  if (!roofs_positive(who, "q", q) || !roofs_positive(who, "res", res)) return SNERF_ERR_BAD_DESC;
  if (!isfinite(cos0) || !isfinite(sin0)) {
    set_error("%s: cos0 and sin0 must be finite (cos0 = %g, sin0 = %g)", who, cos0, sin0);
    return SNERF_ERR_BAD_DESC;
  }
  if (!isfinite(tan2_flat) || !isfinite(tan2_wall) || tan2_flat < 0.0 || tan2_flat > tan2_wall) {
    set_error("%s: 0 <= tan2_flat <= tan2_wall, both finite, required (tan2_flat = %g, tan2_wall = %g)", who, tan2_flat, tan2_wall);
    return SNERF_ERR_BAD_DESC;
  }
  const double f = q / res;
  const dim3 grid((w + ROOF_TILE_W - 1) / ROOF_TILE_W, (h + ROOF_TILE_H - 1) / ROOF_TILE_H), block(ROOF_TILE_W, ROOF_TILE_H);
#define SNERF_ROOFS_LAUNCH(R)                                                                                                       \
  hipLaunchKernelGGL(roofs_normals_kernel<R>, grid, block, 0, (hipStream_t)stream, key, ids, h, w, (int)K, f, cos0, sin0, tan2_flat, \
                     tan2_wall, slope_e, slope_n, code, tag, stats)
  switch (radius) {
    case 1: SNERF_ROOFS_LAUNCH(1); break;
    case 2: SNERF_ROOFS_LAUNCH(2); break;
    case 3: SNERF_ROOFS_LAUNCH(3); break;
    default: SNERF_ROOFS_LAUNCH(4); break;
  }
#undef SNERF_ROOFS_LAUNCH
  SNERF_LAUNCH_CHECK();
  return SNERF_OK;
}

extern "C" int snerf_roofs_link(const int* tag, int h, int w, int connectivity, int* parent, unsigned long long* stats, void* stream) {
  const char* who = "snerf_roofs_link";
  if (!tag || !parent || !stats) { set_error("%s: null pointer", who); return SNERF_ERR_NULL; }
  if (!roofs_sizes_ok(who, h, w)) return SNERF_ERR_BAD_DESC;
  if (connectivity != 4 && connectivity != 8) {
    set_error("%s: connectivity must be 4 or 8 (connectivity = %d)", who, connectivity);
    return SNERF_ERR_BAD_DESC;
  }
  const TagLink pred = {tag};
  return link_launch(pred, h, w, connectivity, parent, stats, stream);
}

extern "C" int snerf_roofs_moments(const int* fids, const int* root, const int* key, const int* tag, int h, int w, long long F, int row0,
                                   int row1, unsigned long long* rows, unsigned long long* stats, void* stream) {
  const char* who = "snerf_roofs_moments";
  if (!fids || !root || !key || !tag || !stats || (F > 0 && !rows)) { set_error("%s: null pointer", who); return SNERF_ERR_NULL; }
  if (!roofs_sizes_ok(who, h, w) || !roofs_count_ok(who, "F", F) || !roofs_band_ok(who, h, row0, row1)) return SNERF_ERR_BAD_DESC;
  if (F == 0 || row0 == row1) return SNERF_OK;
  const long long first = (long long)row0 * w, end = (long long)row1 * w;
  hipLaunchKernelGGL(roofs_moments_kernel, dim3(roofs_blocks(end - first)), dim3(ROOF_THREADS), 0, (hipStream_t)stream, fids, root, key,
                     tag, w, (long long)h * w, F, first, end, rows, stats);
  SNERF_LAUNCH_CHECK();
  return SNERF_OK;
}

extern "C" int snerf_roofs_residuals(const int* fids, const int* root, const int* key, int h, int w, long long F, const double* planes,
                                     double q, double unit, int row0, int row1, float* residual, unsigned long long* rows,
                                     unsigned long long* stats, void* stream) {
  const char* who = "snerf_roofs_residuals";
  if (!fids || !root || !key || !residual || !stats || (F > 0 && (!planes || !rows))) {
    set_error("%s: null pointer", who);
    return SNERF_ERR_NULL;
  }
  if (!roofs_sizes_ok(who, h, w) || !roofs_count_ok(who, "F", F) || !roofs_band_ok(who, h, row0, row1)) return SNERF_ERR_BAD_DESC;
  if (!roofs_positive(who, "q", q) || !roofs_positive(who, "unit", unit)) return SNERF_ERR_BAD_DESC;
  if (row0 == row1) return SNERF_OK;
  const long long first = (long long)row0 * w, end = (long long)row1 * w;
  hipLaunchKernelGGL(roofs_residuals_kernel, dim3(roofs_blocks(end - first)), dim3(ROOF_THREADS), 0, (hipStream_t)stream, fids, root, key,
                     w, (long long)h * w, F, planes, q, unit, first, end, residual, rows, stats);
  SNERF_LAUNCH_CHECK();
  return SNERF_OK;
}
