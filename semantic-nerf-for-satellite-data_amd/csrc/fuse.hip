// Per-cell altitude quantiles over all views on the DSM lattice: the offers of an (E, N, alt) cloud bucketed by cell (count, the
// caller's prefix sums, scatter) and exact order statistics of every bucket (select).  The spec is include/snerf_fuse.h and
// DESIGN.md section 5w; the cell arithmetic is cell_window() and the key lattice_key() of csrc/lattice.h, which ortho_top_kernel
// (csrc/ortho.hip) shares.  Integer atomics only: every word is independent of the order in which points arrive.
#include "lattice.h"
#include "reduce.h"
#include "../../include/snerf_fuse.h"

#pragma clang fp contract(off)

namespace snerf {

constexpr int FUSE_THREADS = 256;
constexpr unsigned FUSE_MAX_BLOCKS = 4096;
constexpr int FUSE_WAVE = 64;                            // the select's workgroup: one wave64, which owns a cell
constexpr int FUSE_BINS = 256;                           // 8 bits a pass
constexpr int FUSE_UNROLL = 4;                           // keys a lane has in flight in a histogram pass
constexpr unsigned FUSE_SELECT_MAX_BLOCKS = 65536;       // cells beyond it are taken in a grid-stride

// ---- the two walks ---------------------------------------------------------------------------------------------------------
// One thread per point (grid-stride above 4096 x 256 points), the loop of ortho_top_kernel.  SCATTER = false: slots = count.
// SCATTER = true: slots = cursor, and the offer's key goes to its slot when the slot lies in the cell's segment and in the buffer.
template <bool SCATTER>
__global__ __launch_bounds__(FUSE_THREADS) void fuse_walk_kernel(const double* __restrict__ xyz, long long n, unsigned long long index0,
                                                                 SnerfDsmGrid g, int r, double z0, double q, unsigned* __restrict__ slots,
                                                                 const long long* __restrict__ offsets, long long capacity,
                                                                 unsigned long long* __restrict__ keys,
                                                                 unsigned long long* __restrict__ stats) {
  unsigned long long bad = 0, reached = 0, dropped = 0;
  for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (long long)gridDim.x * blockDim.x) {
    const double x = xyz[3 * p], y = xyz[3 * p + 1], z = xyz[3 * p + 2];
    unsigned long long key;
    if (!lattice_key(z, z0, q, index0 + (unsigned long long)p, &key)) { bad++; continue; }
    const CellWindow w = cell_window(x, y, g, r);
    if (w.i0 >= w.i1 || w.j0 >= w.j1) continue;
    for (long long lj = w.j0; lj < w.j1; ++lj)
      for (long long li = w.i0; li < w.i1; ++li) {
        const long long c = (lj - g.joff) * g.out_w + (li - g.ioff);
        if (!SCATTER) {
          atomicAdd(&slots[c], 1u);
        } else {
          const unsigned long long t = atomicAdd(&slots[c], 1u);
          const long long lo = offsets[c], hi = offsets[c + 1];
          // 0 <= lo <= lo + t < hi and lo + t < capacity, without forming a sum that could overflow
          if (lo >= 0 && lo < hi && t < (unsigned long long)(hi - lo) && lo < capacity && t < (unsigned long long)(capacity - lo))
            keys[lo + (long long)t] = key;
          else
            dropped++;
        }
      }
    reached++;
  }
  bad = wave_reduce(bad, OpSum());
  reached = wave_reduce(reached, OpSum());
  if (SCATTER) dropped = wave_reduce(dropped, OpSum());
  if ((threadIdx.x & 63) == 0) {
    if (bad) atomicAdd(&stats[0], bad);
    if (reached) atomicAdd(&stats[1], reached);
    if (SCATTER && dropped) atomicAdd(&stats[2], dropped);
  }
}

// ---- the select ------------------------------------------------------------------------------------------------------------
struct FuseQuantiles {
  int num[SNERF_FUSE_MAX_QUANTILES], den[SNERF_FUSE_MAX_QUANTILES];
};

// One wave64 per cell (a workgroup IS one wave: its barriers order the wave's own LDS traffic and cost nothing else).
//   m <= 64: one key per lane; a lane's rank is the number of keys below its own (ties, which a valid segment has none of, by
//     lane), read across the lanes; the lane whose rank is r_k stores its key.
//   m > 64: MSB-first radix select, 8 passes of 8 bits.  A pass reads the segment once; a key that still carries quantile k's
//     prefix adds 1 to bin (k, its byte) of the (K, 256) histogram in LDS; each lane then owns 4 bins, a wave scan of the lanes'
//     sums finds the lane and the bin that hold the remaining rank, and the bin's byte joins the prefix.  After 8 passes the prefix
//     is the key.  The keys are never moved; all counts are at most m <= 2^32 - 1 and fit a u32.
__global__ __launch_bounds__(FUSE_WAVE) void fuse_select_kernel(const unsigned long long* __restrict__ keys,
                                                                const long long* __restrict__ offsets, long long capacity,
                                                                const unsigned* __restrict__ cursor, long long cells,
                                                                FuseQuantiles qs, int K, unsigned long long* __restrict__ words,
                                                                unsigned long long* __restrict__ stats) {
  __shared__ unsigned hist[SNERF_FUSE_MAX_QUANTILES * FUSE_BINS];
  const int lane = threadIdx.x;
  for (long long c = blockIdx.x; c < cells; c += gridDim.x) {
    const long long lo = offsets[c], hi = offsets[c + 1];
    const bool empty = hi == lo;
    const bool refused = !empty && (lo < 0 || hi < lo || hi > capacity || (long long)cursor[c] != hi - lo);
    if (empty || refused) {                                  // retires at once; no key is read
      if (lane < K) words[(long long)lane * cells + c] = 0;
      if (refused && lane == 0) atomicAdd(&stats[3], 1ull);
      continue;
    }
    const unsigned long long m = (unsigned long long)(hi - lo);     // 1 <= m <= 2^32 - 1: it equals a u32 cursor
    const unsigned long long* __restrict__ seg = keys + lo;
    unsigned rank[SNERF_FUSE_MAX_QUANTILES];
#pragma unroll
    for (int k = 0; k < SNERF_FUSE_MAX_QUANTILES; ++k)
      rank[k] = k < K ? (unsigned)(((m - 1) * (unsigned long long)qs.num[k]) / (unsigned long long)qs.den[k]) : 0u;

    if (m <= FUSE_WAVE) {
      const bool have = (unsigned long long)lane < m;
      const unsigned long long key = have ? seg[lane] : ~0ull;
      unsigned below = 0;
      for (int j = 0; j < (int)m; ++j) {
        const unsigned long long other = __shfl(key, j, FUSE_WAVE);
        below += (other < key || (other == key && j < lane)) ? 1u : 0u;
      }
#pragma unroll
      for (int k = 0; k < SNERF_FUSE_MAX_QUANTILES; ++k)
        if (k < K && have && below == rank[k]) words[(long long)k * cells + c] = key;
      continue;
    }

    unsigned long long prefix[SNERF_FUSE_MAX_QUANTILES];
#pragma unroll
    for (int k = 0; k < SNERF_FUSE_MAX_QUANTILES; ++k) prefix[k] = 0;
    for (int pass = 7; pass >= 0; --pass) {
      const int shift = 8 * pass;
      const unsigned long long above = pass == 7 ? 0ull : (~0ull << (shift + 8));     // the bits the earlier passes fixed
      __syncthreads();                                       // the scan of the pass before has read its bins
      for (int b = lane; b < K * FUSE_BINS; b += FUSE_WAVE) hist[b] = 0;
      __syncthreads();
      for (unsigned long long base = 0; base < m; base += FUSE_UNROLL * FUSE_WAVE) {
        unsigned long long key[FUSE_UNROLL];
        bool on[FUSE_UNROLL];
#pragma unroll
        for (int u = 0; u < FUSE_UNROLL; ++u) {
          const unsigned long long i = base + (unsigned long long)(u * FUSE_WAVE + lane);
          on[u] = i < m;
          key[u] = on[u] ? seg[i] : 0ull;
        }
#pragma unroll
        for (int u = 0; u < FUSE_UNROLL; ++u) {
          if (!on[u]) continue;
          const unsigned digit = (unsigned)(key[u] >> shift) & (FUSE_BINS - 1);
#pragma unroll
          for (int k = 0; k < SNERF_FUSE_MAX_QUANTILES; ++k)
            if (k < K && ((key[u] ^ prefix[k]) & above) == 0) atomicAdd(&hist[k * FUSE_BINS + digit], 1u);
        }
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < SNERF_FUSE_MAX_QUANTILES; ++k) {
        if (k >= K) continue;
        const unsigned* bins = hist + k * FUSE_BINS + 4 * lane;
        const unsigned h0 = bins[0], h1 = bins[1], h2 = bins[2], h3 = bins[3];
        const unsigned mine = h0 + h1 + h2 + h3;
        unsigned incl = mine;
#pragma unroll
        for (int o = 1; o < FUSE_WAVE; o <<= 1) {
          const unsigned up = __shfl_up(incl, o, FUSE_WAVE);
          if (lane >= o) incl += up;
        }
        const unsigned r = rank[k];
        unsigned at = incl - mine;                           // the keys in the bins of the lanes before this one
        const bool holds = r >= at && r < incl;              // exactly one lane: r < the total of the bins
        unsigned d = 0;
        if (holds) {
          if (r >= at + h0) { at += h0; d = 1;
            if (r >= at + h1) { at += h1; d = 2;
              if (r >= at + h2) { at += h2; d = 3; } } }
        }
        const int src = __ffsll((long long)__ballot(holds)) - 1;
        const unsigned digit = (unsigned)__shfl((int)(4 * lane + d), src, FUSE_WAVE);
        const unsigned under = (unsigned)__shfl((int)at, src, FUSE_WAVE);
        prefix[k] |= (unsigned long long)digit << shift;
        rank[k] = r - under;
      }
    }
#pragma unroll
    for (int k = 0; k < SNERF_FUSE_MAX_QUANTILES; ++k)
      if (k < K && lane == 0) words[(long long)k * cells + c] = prefix[k];
  }
}

// the checks the two walks share
static int fuse_walk_check(const char* who, const double* xyz, long long n, const SnerfDsmGrid* grid, int radius, double z0, double q,
                           const void* slots, const unsigned long long* stats) {
  if (!grid || !slots || !stats || (n > 0 && !xyz)) { set_error("%s: null pointer", who); return SNERF_ERR_NULL; }
  if (n < 0 || n > LATTICE_MAX_POINTS) { set_error("%s: n must lie in [0, 2^31] (n = %lld)", who, n); return SNERF_ERR_BAD_DESC; }
  if (radius < 0 || radius > SNERF_ORTHO_MAX_RADIUS) {
    set_error("%s: radius must lie in [0, %d] (radius = %d)", who, SNERF_ORTHO_MAX_RADIUS, radius);
    return SNERF_ERR_BAD_DESC;
  }
  if (!lattice_grid_ok(who, grid) || !lattice_window_fits_int32(who, grid)) return SNERF_ERR_BAD_DESC;
  if (!quant_ok(who, z0, q)) return SNERF_ERR_BAD_DESC;
  return SNERF_OK;
}

}  // namespace snerf

using namespace snerf;

extern "C" int snerf_fuse_count(const double* xyz, long long n, const SnerfDsmGrid* grid, int radius, double z0, double q,
                                unsigned* count, unsigned long long* stats, void* stream) {
  const int rc = fuse_walk_check("snerf_fuse_count", xyz, n, grid, radius, z0, q, count, stats);
  if (rc != SNERF_OK) return rc;
  if (n == 0) return SNERF_OK;
  hipLaunchKernelGGL(fuse_walk_kernel<false>, dim3(blocks_for(n, FUSE_THREADS, FUSE_MAX_BLOCKS)), dim3(FUSE_THREADS), 0,
                     (hipStream_t)stream, xyz, n, 0ull, *grid, radius, z0, q, count, (const long long*)nullptr, 0LL,
                     (unsigned long long*)nullptr, stats);
  SNERF_LAUNCH_CHECK();
  return SNERF_OK;
}

extern "C" int snerf_fuse_scatter(const double* xyz, long long n, long long index0, const SnerfDsmGrid* grid, int radius, double z0,
                                  double q, const long long* offsets, long long capacity, unsigned* cursor, unsigned long long* keys,
                                  unsigned long long* stats, void* stream) {
  const char* who = "snerf_fuse_scatter";
  if (!offsets || !keys) { set_error("%s: null pointer", who); return SNERF_ERR_NULL; }
  const int rc = fuse_walk_check(who, xyz, n, grid, radius, z0, q, cursor, stats);
  if (rc != SNERF_OK) return rc;
  if (index0 < 0 || index0 > ORTHO_MAX_INDEX || index0 + n > ORTHO_MAX_INDEX) {
    set_error("%s: index0 >= 0 and index0 + n <= 2^32 - 1 required (index0 = %lld, n = %lld)", who, index0, n);
    return SNERF_ERR_BAD_DESC;
  }
  if (capacity < 0) { set_error("%s: capacity must be >= 0 (capacity = %lld)", who, capacity); return SNERF_ERR_BAD_DESC; }
  if (n == 0) return SNERF_OK;
  hipLaunchKernelGGL(fuse_walk_kernel<true>, dim3(blocks_for(n, FUSE_THREADS, FUSE_MAX_BLOCKS)), dim3(FUSE_THREADS), 0,
                     (hipStream_t)stream, xyz, n, (unsigned long long)index0, *grid, radius, z0, q, cursor, offsets, capacity, keys,
                     stats);
  SNERF_LAUNCH_CHECK();
  return SNERF_OK;
}

extern "C" int snerf_fuse_select(const unsigned long long* keys, const long long* offsets, long long capacity, const unsigned* cursor,
                                 long long cells, const int* quantiles_host, int n_quantiles, unsigned long long* words,
                                 unsigned long long* stats, void* stream) {
  const char* who = "snerf_fuse_select";
  if (!keys || !offsets || !cursor || !quantiles_host || !words || !stats) { set_error("%s: null pointer", who); return SNERF_ERR_NULL; }
  if (capacity < 0) { set_error("%s: capacity must be >= 0 (capacity = %lld)", who, capacity); return SNERF_ERR_BAD_DESC; }
  if (cells < 1 || cells > 2147483647LL) { set_error("%s: cells must lie in [1, 2^31) (cells = %lld)", who, cells); return SNERF_ERR_BAD_DESC; }
  if (n_quantiles < 1 || n_quantiles > SNERF_FUSE_MAX_QUANTILES) {
    set_error("%s: n_quantiles = %d outside [1, %d]", who, n_quantiles, SNERF_FUSE_MAX_QUANTILES);
    return SNERF_ERR_BAD_DESC;
  }
  FuseQuantiles qs = {};
  for (int k = 0; k < SNERF_FUSE_MAX_QUANTILES; ++k) qs.den[k] = 1;
  for (int k = 0; k < n_quantiles; ++k) {
    const int num = quantiles_host[2 * k], den = quantiles_host[2 * k + 1];
    if (den < 1 || den > 65536 || num < 0 || num > den) {
      set_error("%s: quantile %d = (%d, %d): 0 <= num <= den and 1 <= den <= 65536 required", who, k, num, den);
      return SNERF_ERR_BAD_DESC;
    }
    qs.num[k] = num;
    qs.den[k] = den;
  }
  const unsigned blocks = (unsigned)(cells < (long long)FUSE_SELECT_MAX_BLOCKS ? cells : (long long)FUSE_SELECT_MAX_BLOCKS);
  hipLaunchKernelGGL(fuse_select_kernel, dim3(blocks), dim3(FUSE_WAVE), 0, (hipStream_t)stream, keys, offsets, capacity, cursor, cells,
                     qs, n_quantiles, words, stats);
  SNERF_LAUNCH_CHECK();
  return SNERF_OK;
}
