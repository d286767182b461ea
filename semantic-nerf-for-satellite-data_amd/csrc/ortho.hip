// Geo-referenced ortho products on the DSM lattice: the top-surface z-buffer of an (E, N, alt) cloud (one 64-bit key per cell,
// integer atomic max), the gather of the winners' colour / label / scalar, and per-cell label votes (integer atomic add) with
// their argmax.  The spec is the ortho section of include/snerf_hip.h and DESIGN.md section 5j; the cell arithmetic is
// cell_window() of csrc/lattice.h, which dsm_accumulate_kernel (csrc/dsm.hip) shares.  Integer atomics only: every result is
// independent of the order in which points arrive.
#include "lattice.h"
#include "reduce.h"

#pragma clang fp contract(off)

namespace snerf {

constexpr int ORTHO_THREADS = 256;
constexpr unsigned ORTHO_MAX_BLOCKS = 4096;

// ---- top surface -----------------------------------------------------------------------------------------------------------
// One thread per point (grid-stride above 4096 x 256 points).  key = (quantised altitude + 2^31) << 32 | (2^32 - 1 - global index).
__global__ __launch_bounds__(ORTHO_THREADS) void ortho_top_kernel(const double* __restrict__ xyz, long long n,
                                                                  unsigned long long index0, SnerfDsmGrid g, int r, double z0,
                                                                  double q, unsigned long long* __restrict__ top,
                                                                  unsigned long long* __restrict__ stats) {
  unsigned long long bad = 0, reached = 0;
  for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (long long)gridDim.x * blockDim.x) {
    const double x = xyz[3 * p], y = xyz[3 * p + 1], z = xyz[3 * p + 2];
    unsigned long long key;
    if (!lattice_key(z, z0, q, index0 + (unsigned long long)p, &key)) { bad++; continue; }
    const CellWindow w = cell_window(x, y, g, r);
    if (w.i0 >= w.i1 || w.j0 >= w.j1) continue;
    for (long long lj = w.j0; lj < w.j1; ++lj)
      for (long long li = w.i0; li < w.i1; ++li) atomicMax(&top[(lj - g.joff) * g.out_w + (li - g.ioff)], key);
    reached++;
  }
  bad = wave_reduce(bad, OpSum());
  reached = wave_reduce(reached, OpSum());
  if ((threadIdx.x & 63) == 0) {
    if (bad) atomicAdd(&stats[0], bad);
    if (reached) atomicAdd(&stats[1], reached);
  }
}

// One thread per cell: decode the key; payloads only where the winner belongs to [index0, index0 + n).
__global__ __launch_bounds__(ORTHO_THREADS) void ortho_gather_kernel(const unsigned long long* __restrict__ top, long long cells,
                                                                     long long index0, long long n, double z0, double q,
                                                                     const float* __restrict__ rgb, const long long* __restrict__ labels,
                                                                     const float* __restrict__ scalar, float* __restrict__ alt_out,
                                                                     long long* __restrict__ idx_out, float* __restrict__ rgb_out,
                                                                     unsigned char* __restrict__ label_out,
                                                                     float* __restrict__ scalar_out) {
  for (long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x; c < cells; c += (long long)gridDim.x * blockDim.x) {
    const unsigned long long key = top[c];
    if (key == 0) {
      alt_out[c] = __builtin_nanf("");
      idx_out[c] = -1;
      continue;
    }
    const long long k = (long long)(key >> 32) - 2147483648LL;
    const long long idx = (long long)(0xFFFFFFFFull - (key & 0xFFFFFFFFull));
    alt_out[c] = (float)(z0 + q * (double)k);
    idx_out[c] = idx;
    const long long row = idx - index0;
    if (row < 0 || row >= n) continue;
    if (rgb_out) {
      rgb_out[c] = rgb[3 * row];
      rgb_out[cells + c] = rgb[3 * row + 1];
      rgb_out[2 * cells + c] = rgb[3 * row + 2];
    }
    if (label_out) {
      const long long l = labels[row];
      label_out[c] = (l >= 0 && l <= 254) ? (unsigned char)l : (unsigned char)SNERF_ORTHO_NO_LABEL;
    }
    if (scalar_out) scalar_out[c] = scalar[row];
  }
}

// ---- votes -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ORTHO_THREADS) void ortho_votes_kernel(const double* __restrict__ xyz, const long long* __restrict__ labels,
                                                                    long long n, SnerfDsmGrid g, int r, int n_classes,
                                                                    unsigned* __restrict__ votes,
                                                                    unsigned long long* __restrict__ stats) {
  unsigned long long bad = 0;
  const long long cells = (long long)g.out_h * g.out_w;
  for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (long long)gridDim.x * blockDim.x) {
    const double x = xyz[3 * p], y = xyz[3 * p + 1];
    const long long l = labels[p];
    if (l < 0 || l >= n_classes || !__builtin_isfinite(x) || !__builtin_isfinite(y)) { bad++; continue; }
    const CellWindow w = cell_window(x, y, g, r);
    if (w.i0 >= w.i1 || w.j0 >= w.j1) continue;
    unsigned* plane = votes + l * cells;
    for (long long lj = w.j0; lj < w.j1; ++lj)
      for (long long li = w.i0; li < w.i1; ++li) atomicAdd(&plane[(lj - g.joff) * g.out_w + (li - g.ioff)], 1u);
  }
  bad = wave_reduce(bad, OpSum());
  if ((threadIdx.x & 63) == 0 && bad) atomicAdd(&stats[0], bad);
}

__global__ __launch_bounds__(ORTHO_THREADS) void ortho_votes_finish_kernel(const unsigned* __restrict__ votes, int n_classes,
                                                                           long long cells, unsigned char* __restrict__ label_out,
                                                                           float* __restrict__ share_out,
                                                                           unsigned long long* __restrict__ stats) {
  unsigned long long tmax = 0;
  for (long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x; c < cells; c += (long long)gridDim.x * blockDim.x) {
    unsigned best = 0;
    int arg = SNERF_ORTHO_NO_LABEL;
    unsigned long long total = 0;
    for (int k = 0; k < n_classes; ++k) {
      const unsigned v = votes[(long long)k * cells + c];
      total += v;
      if (v > best) { best = v; arg = k; }          // strict: the lowest class keeps a tie
    }
    label_out[c] = (unsigned char)arg;
    share_out[c] = total ? (float)((double)best / (double)total) : __builtin_nanf("");
    tmax = total > tmax ? total : tmax;
  }
  tmax = wave_reduce(tmax, OpMax());
  if ((threadIdx.x & 63) == 0 && tmax) atomicMax(&stats[1], tmax);
}

}  // namespace snerf

using namespace snerf;

extern "C" int snerf_ortho_top(const double* xyz, long long n, long long index0, const SnerfDsmGrid* grid, int radius, double z0,
                               double q, unsigned long long* top, unsigned long long* stats, void* stream) {
  if (!grid || !top || !stats || (n > 0 && !xyz)) { set_error("snerf_ortho_top: null pointer"); return SNERF_ERR_NULL; }
  if (n < 0 || n > LATTICE_MAX_POINTS) { set_error("snerf_ortho_top: n must lie in [0, 2^31]"); return SNERF_ERR_BAD_DESC; }
  if (index0 < 0 || index0 > ORTHO_MAX_INDEX || index0 + n > ORTHO_MAX_INDEX) {
    set_error("snerf_ortho_top: index0 >= 0 and index0 + n <= 2^32 - 1 required (index0 = %lld, n = %lld)", index0, n);
    return SNERF_ERR_BAD_DESC;
  }
  if (radius < 0 || radius > SNERF_ORTHO_MAX_RADIUS) { set_error("snerf_ortho_top: radius must lie in [0, %d]", SNERF_ORTHO_MAX_RADIUS); return SNERF_ERR_BAD_DESC; }
  if (!lattice_grid_ok("snerf_ortho_top", grid) || !lattice_window_fits_int32("snerf_ortho_top", grid)) return SNERF_ERR_BAD_DESC;
  if (!quant_ok("snerf_ortho_top", z0, q)) return SNERF_ERR_BAD_DESC;
  if (n == 0) return SNERF_OK;
  hipLaunchKernelGGL(ortho_top_kernel, dim3(blocks_for(n, ORTHO_THREADS, ORTHO_MAX_BLOCKS)), dim3(ORTHO_THREADS), 0, (hipStream_t)stream, xyz, n,
                     (unsigned long long)index0, *grid, radius, z0, q, top, stats);
  SNERF_LAUNCH_CHECK();
  return SNERF_OK;
}

extern "C" int snerf_ortho_gather(const unsigned long long* top, long long cells, long long index0, long long n, double z0, double q,
                                  const float* rgb, const long long* labels, const float* scalar, float* alt_out, long long* idx_out,
                                  float* rgb_out, unsigned char* label_out, float* scalar_out, void* stream) {
  if (!top || !alt_out || !idx_out) { set_error("snerf_ortho_gather: null pointer"); return SNERF_ERR_NULL; }
  if (!rgb != !rgb_out || !labels != !label_out || !scalar != !scalar_out) {
    set_error("snerf_ortho_gather: a payload and its output are given together or not at all"); return SNERF_ERR_NULL; }
  if (cells < 1 || cells > (1LL << 62)) { set_error("snerf_ortho_gather: cells must be >= 1"); return SNERF_ERR_BAD_DESC; }
  if (n < 0 || n > LATTICE_MAX_POINTS) { set_error("snerf_ortho_gather: n must lie in [0, 2^31]"); return SNERF_ERR_BAD_DESC; }
  if (index0 < 0 || index0 > ORTHO_MAX_INDEX || index0 + n > ORTHO_MAX_INDEX) {
    set_error("snerf_ortho_gather: index0 >= 0 and index0 + n <= 2^32 - 1 required (index0 = %lld, n = %lld)", index0, n);
    return SNERF_ERR_BAD_DESC;
  }
  if (!quant_ok("snerf_ortho_gather", z0, q)) return SNERF_ERR_BAD_DESC;
  if (n == 0) return SNERF_OK;
  hipLaunchKernelGGL(ortho_gather_kernel, dim3(blocks_for(cells, ORTHO_THREADS, ORTHO_MAX_BLOCKS)), dim3(ORTHO_THREADS), 0, (hipStream_t)stream, top, cells, index0,
                     n, z0, q, rgb, labels, scalar, alt_out, idx_out, rgb_out, label_out, scalar_out);
  SNERF_LAUNCH_CHECK();
  return SNERF_OK;
}

extern "C" int snerf_ortho_votes(const double* xyz, const long long* labels, long long n, const SnerfDsmGrid* grid, int radius,
                                 int n_classes, unsigned* votes, unsigned long long* stats, void* stream) {
  if (!grid || !votes || !stats || (n > 0 && (!xyz || !labels))) { set_error("snerf_ortho_votes: null pointer"); return SNERF_ERR_NULL; }
  if (n < 0 || n > LATTICE_MAX_POINTS) { set_error("snerf_ortho_votes: n must lie in [0, 2^31]"); return SNERF_ERR_BAD_DESC; }
  if (radius < 0 || radius > SNERF_ORTHO_MAX_RADIUS) { set_error("snerf_ortho_votes: radius must lie in [0, %d]", SNERF_ORTHO_MAX_RADIUS); return SNERF_ERR_BAD_DESC; }
  if (n_classes < 1 || n_classes > SNERF_ORTHO_MAX_CLASSES) { set_error("snerf_ortho_votes: n_classes must lie in [1, %d]", SNERF_ORTHO_MAX_CLASSES); return SNERF_ERR_BAD_DESC; }
  if (!lattice_grid_ok("snerf_ortho_votes", grid) || !lattice_window_fits_int32("snerf_ortho_votes", grid)) return SNERF_ERR_BAD_DESC;
  if (n == 0) return SNERF_OK;
  hipLaunchKernelGGL(ortho_votes_kernel, dim3(blocks_for(n, ORTHO_THREADS, ORTHO_MAX_BLOCKS)), dim3(ORTHO_THREADS), 0, (hipStream_t)stream, xyz, labels, n, *grid,
                     radius, n_classes, votes, stats);
  SNERF_LAUNCH_CHECK();
  return SNERF_OK;
}

extern "C" int snerf_ortho_votes_finish(const unsigned* votes, int n_classes, long long cells, unsigned char* label_out,
                                        float* share_out, unsigned long long* stats, void* stream) {
  if (!votes || !label_out || !share_out || !stats) { set_error("snerf_ortho_votes_finish: null pointer"); return SNERF_ERR_NULL; }
  if (n_classes < 1 || n_classes > SNERF_ORTHO_MAX_CLASSES) { set_error("snerf_ortho_votes_finish: n_classes must lie in [1, %d]", SNERF_ORTHO_MAX_CLASSES); return SNERF_ERR_BAD_DESC; }
  if (cells < 1 || cells > (1LL << 53)) { set_error("snerf_ortho_votes_finish: cells must be >= 1"); return SNERF_ERR_BAD_DESC; }
  hipLaunchKernelGGL(ortho_votes_finish_kernel, dim3(blocks_for(cells, ORTHO_THREADS, ORTHO_MAX_BLOCKS)), dim3(ORTHO_THREADS), 0, (hipStream_t)stream, votes,
                     n_classes, cells, label_out, share_out, stats);
  SNERF_LAUNCH_CHECK();
  return SNERF_OK;
}
