// DSM evaluation on the device: rasterisation of an (E, N, alt) point cloud (plyflatten with radius r, sigma = inf, as the
// reference calls it: eval/utils/dsm.py:75-77), the 2x pyramid and the NCC shift search of the registration
// (eval/utils/dsmr.py:17-144), and the shifted difference against the ground truth (dsm.py:235-266).  The spec and the
// numerics are stated in include/snerf_hip.h and in snerf_amd/eval/utils/dsm.py; every reduction here is in a fixed order,
// so every result is bit-reproducible run to run.
#include "lattice.h"
#include "reduce.h"

namespace snerf {

// ---- rasterisation ---------------------------------------------------------------------------------------------------
// One pass over the points; a point adds round((z - z0)/q) to the int64 sum and 1 to the u32 count of every cell of its
// cell_window() (lattice.h): its (2r+1)^2 window inside the lattice extent AND the output window.  Integer atomics commute, so
// the result does not depend on the order in which points arrive.  stats[0] = max |round((z - z0)/q)| of the points that
// reached a cell (the host bounds the sums with it), stats[1] = number of points whose quantised altitude is not finite or not
// below 2^62 (they add nothing).
__global__ __launch_bounds__(256) void dsm_accumulate_kernel(const double* __restrict__ xyz, int n, SnerfDsmGrid g, int r,
                                                             double z0, double inv_q, unsigned* __restrict__ count,
                                                             unsigned long long* __restrict__ sum,
                                                             unsigned long long* __restrict__ stats) {
  unsigned long long kmax = 0, bad = 0;
  const double lim = 4611686018427387904.0;   // 2^62
  for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (long long)gridDim.x * blockDim.x) {
    const double x = xyz[3 * p], y = xyz[3 * p + 1], z = xyz[3 * p + 2];
    const double kq = rint((z - z0) * inv_q);
    if (!(fabs(kq) < lim)) { bad++; continue; }
    const CellWindow w = cell_window(x, y, g, r);
    if (w.i0 >= w.i1 || w.j0 >= w.j1) continue;
    const long long k = (long long)kq;
    const unsigned long long ak = (unsigned long long)(k < 0 ? -k : k);
    kmax = ak > kmax ? ak : kmax;
    for (long long lj = w.j0; lj < w.j1; ++lj)
      for (long long li = w.i0; li < w.i1; ++li) {
        const long long cell = (lj - g.joff) * g.out_w + (li - g.ioff);
        atomicAdd(&count[cell], 1u);
        atomicAdd(&sum[cell], (unsigned long long)k);   // two's complement: a signed sum
      }
  }
  kmax = wave_reduce(kmax, OpMax());
  bad = wave_reduce(bad, OpSum());
  if ((threadIdx.x & 63) == 0) {
    if (kmax) atomicMax(&stats[0], kmax);
    if (bad) atomicAdd(&stats[1], bad);
  }
}

// cell value = z0 + q * sum / count (fp64, one rounding to fp32), NaN where nothing arrived; stats[2] = largest count
__global__ __launch_bounds__(256) void dsm_finish_kernel(const unsigned* __restrict__ count, const long long* __restrict__ sum,
                                                         long long cells, double z0, double q, float* __restrict__ dsm,
                                                         unsigned long long* __restrict__ stats) {
  unsigned long long cmax = 0;
  for (long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x; c < cells; c += (long long)gridDim.x * blockDim.x) {
    const unsigned m = count[c];
    cmax = m > cmax ? m : cmax;
    dsm[c] = m ? (float)(z0 + q * ((double)sum[c] / (double)m)) : __builtin_nanf("");
  }
  cmax = wave_reduce(cmax, OpMax());
  if ((threadIdx.x & 63) == 0 && cmax) atomicMax(&stats[2], cmax);
}

// ---- pyramid: dsmr.downsample2x_ ----------------------------------------------------------------------------------------
// out[J][I] = NaN-aware mean of u[j:j+2, i:i+2] at j = min(2J+1, H-1), i = min(2I+1, W-1) (the reference's loop writes
// every cell up to four times and the last write wins), summed in its order (i,j), (i,j+1), (i+1,j), (i+1,j+1), in fp64.
template <typename T>
__global__ __launch_bounds__(256) void downsample2x_kernel(const T* __restrict__ u, int h, int w, double* __restrict__ out) {
  const int ho = (h + 1) / 2, wo = (w + 1) / 2;
  const long long total = (long long)ho * wo;
  for (long long o = (long long)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (long long)gridDim.x * blockDim.x) {
    const int J = (int)(o / wo), I = (int)(o % wo);
    const int j = min(2 * J + 1, h - 1), i = min(2 * I + 1, w - 1);
    double s = 0.0;
    int c = 0;
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
      for (int l = 0; l < 2; ++l) {
        const int ii = i + k, jj = j + l;
        if (ii < w && jj < h) {
          const double t = (double)u[(long long)jj * w + ii];
          if (__builtin_isfinite(t)) { s += t; c++; }
        }
      }
    out[o] = c ? s / (double)c : __builtin_nan("");
  }
}

// ---- NCC search: dsmr.mean_std over every shift of one search window ------------------------------------------------------
// A workgroup stages a TILE x TILE block of u and the block of v it meets under every shift (an r-pixel halo around the
// search centre), both as fp64 in LDS, and thread s accumulates shift s over the whole tile.  Pass 0: (count, sum u, sum v)
// over the pixels where both values are finite; pass 1: the centred (sum u'^2, sum v'^2, sum u'v') about the means of pass 0.
// The v tile's row pitch is = 2r+1 (mod 32) doubles: the 2r+1 shifts of one row of the window are consecutive addresses, so
// the 32-lane groups of a ds_read_b64 touch 32 consecutive doubles (conflict-free); every lane reads the same u (broadcast).
constexpr int NCC_TILE = 32;
constexpr int NCC_THREADS = 128;
constexpr int NCC_MAX_R = 7;

__host__ __device__ inline int ncc_vpitch(int r) {
  const int need = NCC_TILE + 2 * r, want = (2 * r + 1) & 31;
  return need + ((want - need % 32) + 32) % 32;
}

template <typename T>
__global__ __launch_bounds__(NCC_THREADS) void ncc_tile_kernel(const T* __restrict__ u, const T* __restrict__ v, int h, int w,
                                                               int cx, int cy, int r, int pass,
                                                               const double* __restrict__ stats, double* __restrict__ partial) {
  extern __shared__ double lds[];
  const int S1 = 2 * r + 1, S = S1 * S1, vp = ncc_vpitch(r), vrows = NCC_TILE + 2 * r;
  double* U = lds;                                   // [TILE][TILE]
  double* V = lds + NCC_TILE * NCC_TILE;             // [TILE + 2r][vp]
  const int i0 = blockIdx.x * NCC_TILE, j0 = blockIdx.y * NCC_TILE;
  const double nan = __builtin_nan("");
  for (int t = threadIdx.x; t < NCC_TILE * NCC_TILE; t += NCC_THREADS) {
    const int jj = j0 + t / NCC_TILE, ii = i0 + t % NCC_TILE;
    U[t] = (jj < h && ii < w) ? (double)u[(long long)jj * w + ii] : nan;
  }
  for (int t = threadIdx.x; t < vrows * vp; t += NCC_THREADS) {
    const int tr = t / vp, tc = t % vp;
    const int jj = j0 + cy - r + tr, ii = i0 + cx - r + tc;
    V[t] = (tc < NCC_TILE + 2 * r && jj >= 0 && jj < h && ii >= 0 && ii < w) ? (double)v[(long long)jj * w + ii] : nan;
  }
  __syncthreads();
  const long long blk = (long long)blockIdx.y * gridDim.x + blockIdx.x;
  for (int s = threadIdx.x; s < S; s += NCC_THREADS) {
    const int oy = s / S1, ox = s % S1;              // shift (cx - r + ox, cy - r + oy): y outer, x inner, as compute_ncc
    const double* Vs = V + oy * vp + ox;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    if (pass == 0) {
      int c = 0;
      for (int jj = 0; jj < NCC_TILE; ++jj)
        for (int ii = 0; ii < NCC_TILE; ++ii) {
          const double uu = U[jj * NCC_TILE + ii], vv = Vs[jj * vp + ii];
          if (__builtin_isfinite(uu) && __builtin_isfinite(vv)) { c++; a1 += uu; a2 += vv; }
        }
      a0 = (double)c;
    } else {
      const double cnt = stats[s * 6 + 0];
      const double muu = stats[s * 6 + 1] / cnt, muv = stats[s * 6 + 2] / cnt;
      for (int jj = 0; jj < NCC_TILE; ++jj)
        for (int ii = 0; ii < NCC_TILE; ++ii) {
          const double du = U[jj * NCC_TILE + ii] - muu, dv = Vs[jj * vp + ii] - muv;
          if (__builtin_isfinite(du) && __builtin_isfinite(dv)) { a0 += du * du; a1 += dv * dv; a2 += du * dv; }
        }
    }
    partial[(blk * 3 + 0) * S + s] = a0;
    partial[(blk * 3 + 1) * S + s] = a1;
    partial[(blk * 3 + 2) * S + s] = a2;
  }
}

// one workgroup per (component k, shift s): the per-block partials partial[(b * 3 + k) * S + s], b ascending (reduce.h)
__global__ __launch_bounds__(256) void ncc_reduce_kernel(const double* __restrict__ partial, long long nblk, int S, int pass,
                                                         double* __restrict__ stats) {
  __shared__ double red[256];
  const int k = blockIdx.x / S, s = blockIdx.x % S;
  block_strided_sum<256>(red, threadIdx.x, partial + k * S + s, nblk, 3LL * S);
  if (threadIdx.x == 0) stats[s * 6 + 3 * pass + k] = red[0];
}

// ---- shift, difference and reduction: dsmr.apply_shift_ (a = 1) and compute_mae's diff = rdsm - gt ----------------------
constexpr int DIFF_THREADS = 256;
constexpr int DIFF_MAX_BLOCKS = 1024;

__global__ __launch_bounds__(DIFF_THREADS) void shift_diff_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                                  int h, int w, int dx, int dy, double b,
                                                                  float* __restrict__ rdsm, float* __restrict__ diff,
                                                                  double* __restrict__ partial) {
  __shared__ double red[2 * DIFF_THREADS];             // the sums of |d|, then the counts
  const long long cells = (long long)h * w;
  double s = 0.0, c = 0.0;
  for (long long p = (long long)blockIdx.x * DIFF_THREADS + threadIdx.x; p < cells; p += (long long)gridDim.x * DIFF_THREADS) {
    const int j = (int)(p / w), i = (int)(p % w);
    const int sj = j + dy, si = i + dx;
    float rv = __builtin_nanf("");
    if (sj >= 0 && sj < h && si >= 0 && si < w) rv = (float)((double)pred[(long long)sj * w + si] + b);
    float g = gt[p];
    if (g < -500.f) g = 0.f;                         // dsm.py:229-231: gt_dsm[gt_dsm < -500.0] = 0.0
    const float d = rv - g;
    if (rdsm) rdsm[p] = rv;
    if (diff) diff[p] = d;
    if (__builtin_isfinite(d)) { s += fabs((double)d); c += 1.0; }
  }
  const double sc[2] = {s, c};
  block_tree<DIFF_THREADS, 2>(red, threadIdx.x, sc, [](int, double a, double b) { return a + b; });
  if (threadIdx.x == 0) { partial[2 * blockIdx.x] = red[0]; partial[2 * blockIdx.x + 1] = red[DIFF_THREADS]; }
}

// one thread, serially over the blocks in ascending order: this order is part of the totals' bits
__global__ __launch_bounds__(64) void diff_total_kernel(const double* __restrict__ partial, int nblk, double* __restrict__ totals) {
  if (threadIdx.x == 0) {
    double s = 0.0, c = 0.0;
    for (int b = 0; b < nblk; ++b) { s += partial[2 * b]; c += partial[2 * b + 1]; }
    totals[0] = s;
    totals[1] = c;
  }
}

}  // namespace snerf

using namespace snerf;

extern "C" int snerf_dsm_accumulate(const double* xyz, int n, const SnerfDsmGrid* grid, int radius, double z0, double q,
                                    unsigned* count, long long* sum, unsigned long long* stats, void* stream) {
  if (!grid || !count || !sum || !stats || (n > 0 && !xyz)) { set_error("snerf_dsm_accumulate: null pointer"); return SNERF_ERR_NULL; }
  if (n < 0) { set_error("snerf_dsm_accumulate: n must be >= 0"); return SNERF_ERR_BAD_DESC; }
  if (!lattice_grid_ok("snerf_dsm_accumulate", grid)) return SNERF_ERR_BAD_DESC;
  if (radius < 0 || radius > 64) { set_error("snerf_dsm_accumulate: radius must lie in [0, 64]"); return SNERF_ERR_BAD_DESC; }
  if (!quant_ok("snerf_dsm_accumulate", z0, q, "q > 0 and finite z0 required")) return SNERF_ERR_BAD_DESC;
  if (n == 0) return SNERF_OK;
  hipLaunchKernelGGL(dsm_accumulate_kernel, dim3(blocks_for(n, 256, 4096)), dim3(256), 0, (hipStream_t)stream, xyz, n, *grid,
                     radius, z0, 1.0 / q, count, (unsigned long long*)sum, stats);
  SNERF_LAUNCH_CHECK();
  return SNERF_OK;
}

extern "C" int snerf_dsm_finish(const unsigned* count, const long long* sum, long long cells, double z0, double q, float* dsm,
                                unsigned long long* stats, void* stream) {
  if (!count || !sum || !dsm || !stats) { set_error("snerf_dsm_finish: null pointer"); return SNERF_ERR_NULL; }
  if (cells <= 0) { set_error("snerf_dsm_finish: cells must be > 0"); return SNERF_ERR_BAD_DESC; }
  if (!quant_ok("snerf_dsm_finish", z0, q, "q > 0 and finite z0 required")) return SNERF_ERR_BAD_DESC;
  hipLaunchKernelGGL(dsm_finish_kernel, dim3(blocks_for(cells, 256, 4096)), dim3(256), 0, (hipStream_t)stream, count, sum, cells,
                     z0, q, dsm, stats);
  SNERF_LAUNCH_CHECK();
  return SNERF_OK;
}

extern "C" int snerf_dsm_downsample2x(const void* u, int u_f64, int h, int w, double* out, void* stream) {
  if (!u || !out) { set_error("snerf_dsm_downsample2x: null pointer"); return SNERF_ERR_NULL; }
  if (h <= 0 || w <= 0) { set_error("snerf_dsm_downsample2x: h, w must be > 0"); return SNERF_ERR_BAD_DESC; }
  const long long total = (long long)((h + 1) / 2) * ((w + 1) / 2);
  const dim3 grid(blocks_for(total, 256, 4096));
  if (u_f64) hipLaunchKernelGGL(downsample2x_kernel<double>, grid, dim3(256), 0, (hipStream_t)stream, (const double*)u, h, w, out);
  else hipLaunchKernelGGL(downsample2x_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)u, h, w, out);
  SNERF_LAUNCH_CHECK();
  return SNERF_OK;
}

extern "C" size_t snerf_dsm_workspace_bytes(int h, int w, int radius) {
  if (h <= 0 || w <= 0) { set_error("snerf_dsm_workspace_bytes: h, w must be > 0"); return 0; }
  if (radius < 0 || radius > NCC_MAX_R) { set_error("snerf_dsm_workspace_bytes: radius must lie in [0, %d]", NCC_MAX_R); return 0; }
  const long long nblk = (long long)((w + NCC_TILE - 1) / NCC_TILE) * ((h + NCC_TILE - 1) / NCC_TILE);
  const long long S = (2LL * radius + 1) * (2LL * radius + 1);
  const size_t ncc = (size_t)(nblk * 3 * S) * sizeof(double);
  const size_t dif = (size_t)(2 * DIFF_MAX_BLOCKS) * sizeof(double);
  return ncc > dif ? ncc : dif;
}

extern "C" int snerf_dsm_ncc_search(const void* u, const void* v, int f64, int h, int w, int cx, int cy, int radius,
                                    double* stats, void* workspace, size_t workspace_bytes, void* stream) {
  if (!u || !v || !stats || !workspace) { set_error("snerf_dsm_ncc_search: null pointer"); return SNERF_ERR_NULL; }
  if (h <= 0 || w <= 0) { set_error("snerf_dsm_ncc_search: h, w must be > 0"); return SNERF_ERR_BAD_DESC; }
  if (radius < 0 || radius > NCC_MAX_R) { set_error("snerf_dsm_ncc_search: radius must lie in [0, %d]", NCC_MAX_R); return SNERF_ERR_BAD_DESC; }
  if (cx < -(1 << 20) || cx > (1 << 20) || cy < -(1 << 20) || cy > (1 << 20)) { set_error("snerf_dsm_ncc_search: search centre out of range"); return SNERF_ERR_BAD_DESC; }
  const size_t need = snerf_dsm_workspace_bytes(h, w, radius);
  if (workspace_bytes < need) { set_error("snerf_dsm_ncc_search: workspace of %zu bytes < %zu", workspace_bytes, need); return SNERF_ERR_WORKSPACE; }
  const int S = (2 * radius + 1) * (2 * radius + 1);
  const dim3 grid((w + NCC_TILE - 1) / NCC_TILE, (h + NCC_TILE - 1) / NCC_TILE);
  const long long nblk = (long long)grid.x * grid.y;
  const size_t lds = (size_t)(NCC_TILE * NCC_TILE + (NCC_TILE + 2 * radius) * ncc_vpitch(radius)) * sizeof(double);
  double* partial = (double*)workspace;
  hipStream_t st = (hipStream_t)stream;
  for (int pass = 0; pass < 2; ++pass) {
    if (f64) hipLaunchKernelGGL(ncc_tile_kernel<double>, grid, dim3(NCC_THREADS), lds, st, (const double*)u, (const double*)v, h, w,
                                cx, cy, radius, pass, (const double*)stats, partial);
    else hipLaunchKernelGGL(ncc_tile_kernel<float>, grid, dim3(NCC_THREADS), lds, st, (const float*)u, (const float*)v, h, w,
                            cx, cy, radius, pass, (const double*)stats, partial);
    SNERF_LAUNCH_CHECK();
    hipLaunchKernelGGL(ncc_reduce_kernel, dim3(3 * S), dim3(256), 0, st, (const double*)partial, nblk, S, pass, stats);
    SNERF_LAUNCH_CHECK();
  }
  return SNERF_OK;
}

extern "C" int snerf_dsm_shift_diff(const float* pred, const float* gt, int h, int w, int dx, int dy, double b, float* rdsm,
                                    float* diff, double* totals, void* workspace, size_t workspace_bytes, void* stream) {
  if (!pred || !gt || !totals || !workspace) { set_error("snerf_dsm_shift_diff: null pointer"); return SNERF_ERR_NULL; }
  if (h <= 0 || w <= 0) { set_error("snerf_dsm_shift_diff: h, w must be > 0"); return SNERF_ERR_BAD_DESC; }
  if (dx < -(1 << 20) || dx > (1 << 20) || dy < -(1 << 20) || dy > (1 << 20)) { set_error("snerf_dsm_shift_diff: shift out of range"); return SNERF_ERR_BAD_DESC; }
  if (workspace_bytes < (size_t)(2 * DIFF_MAX_BLOCKS) * sizeof(double)) {
    set_error("snerf_dsm_shift_diff: workspace of %zu bytes is too small", workspace_bytes); return SNERF_ERR_WORKSPACE; }
  const int nblk = (int)blocks_for((long long)h * w, DIFF_THREADS, DIFF_MAX_BLOCKS);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(shift_diff_kernel, dim3(nblk), dim3(DIFF_THREADS), 0, st, pred, gt, h, w, dx, dy, b, rdsm, diff,
                     (double*)workspace);
  SNERF_LAUNCH_CHECK();
  hipLaunchKernelGGL(diff_total_kernel, dim3(1), dim3(64), 0, st, (const double*)workspace, nblk, totals);
  SNERF_LAUNCH_CHECK();
  return SNERF_OK;
}
