// Bare-earth terrain on the map: altitudes to integer keys, one level of a progressive morphological filter (a grey-scale opening
// by a square of up to 1025 cells a side, separable, van Herk / Gil-Werman in every pass) and a scan-line fill of the ground under
// everything that is not ground.  The spec is include/snerf_terrain.h and DESIGN.md section 5y; tests/terrain_numpy.py restates it.
// In every pass consecutive lanes read consecutive addresses: along rows a wave scans over its lanes with a carry, along columns the
// lanes lie across columns and a thread walks one block of its column, or one of 16 segments of a long block.  Every loop is
// counted by h, w and radius.
#include "lattice.h"
#include "reduce.h"
#include "../../include/snerf_terrain.h"

#include <limits.h>

// the fill's fp64 arithmetic is restated operation by operation in numpy: no fused multiply-add (csrc/shadow.hip has the long form)
#pragma clang fp contract(off)

namespace snerf {

constexpr int TER_THREADS = 256;
constexpr int TER_WAVES = TER_THREADS / 64;
constexpr int TER_NONE_MIN = INT_MAX;        // "none" among minima: the identity of min, above every valid key
constexpr int TER_NONE_MAX = INT_MIN;        // "none" among maxima: the identity of max, below every valid key = the stored hole

struct TerClasses {
  unsigned long long bits[4];
};
__device__ __forceinline__ bool ter_in_classes(const TerClasses& t, unsigned c) {
  const unsigned long long lo = c & 64 ? t.bits[1] : t.bits[0], hi = c & 64 ? t.bits[3] : t.bits[2];
  return (((c & 128 ? hi : lo) >> (c & 63)) & 1ull) != 0;
}

__device__ __forceinline__ bool ter_valid(int k) { return k != INT_MIN && k != INT_MAX; }

// ---- keys --------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TER_THREADS) void terrain_keys_kernel(const float* __restrict__ alt, const unsigned char* __restrict__ label,
                                                                   long long cells, TerClasses blocked, double z0, double q,
                                                                   int* __restrict__ key, unsigned char* __restrict__ flags,
                                                                   unsigned long long* __restrict__ stats) {
  unsigned long long out_of_range = 0, not_finite = 0, n_blocked = 0;
  for (long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x; c < cells; c += (long long)gridDim.x * blockDim.x) {
    const float a = alt[c];
    const double kq = rint(((double)a - z0) / q);
    int k = SNERF_TERRAIN_HOLE;
    unsigned f = 0;
    if (kq > -2147483648.0 && kq < 2147483647.0) {
      k = (int)kq;
    } else {
      f = SNERF_TERRAIN_IS_HOLE;
      if (isfinite(a)) out_of_range++; else not_finite++;
    }
    if (label != nullptr && ter_in_classes(blocked, label[c])) {
      f |= SNERF_TERRAIN_BLOCKED;
      n_blocked++;
    }
    key[c] = k;
    flags[c] = (unsigned char)f;
  }
  out_of_range = wave_reduce(out_of_range, OpSum());
  not_finite = wave_reduce(not_finite, OpSum());
  n_blocked = wave_reduce(n_blocked, OpSum());
  if ((threadIdx.x & 63) == 0) {
    if (out_of_range) atomicAdd(&stats[0], out_of_range);
    if (not_finite) atomicAdd(&stats[1], not_finite);
    if (n_blocked) atomicAdd(&stats[2], n_blocked);
  }
}

// ---- the window minimum / maximum along one axis ------------------------------------------------------------------------------------
// out[x] = op over in[x - r .. x + r] clipped to [0, n).  With L = 2 r + 1 and a = x - r the window is [a, a + L - 1]; cut the axis
// into blocks of L starting at -r.  For a at offset t of the block that starts at p:
//     out = op( S[a] = op over [a, p + L - 1],  G[t] = op over [p + L, p + L + t - 1] )          (G[0] is empty)
// S is a suffix scan of block p, G an exclusive prefix scan of the next block; a position outside [0, n) reads as op's identity,
// which clips the window.  S[a] is parked in out[x] by the thread that later combines it with G[t]: no other scratch.
template <bool MAX>
__device__ __forceinline__ int ter_identity() { return MAX ? TER_NONE_MAX : TER_NONE_MIN; }
template <bool MAX>
__device__ __forceinline__ int ter_op(int a, int b) { return MAX ? (b > a ? b : a) : (b < a ? b : a); }
// MAP: the first pass of the erosion reads holes as "none"; the first pass of the dilation reads the erosion's "none" as its own
template <bool MAX, bool MAP>
__device__ __forceinline__ int ter_load(const int* __restrict__ in, long long at, long long pos, long long n) {
  if (pos < 0 || pos >= n) return ter_identity<MAX>();
  const int v = in[at];
  if (MAP) return (MAX ? v == TER_NONE_MIN : v == INT_MIN) ? ter_identity<MAX>() : v;
  return v;
}

// Rows.  One wave per (row, group of nb blocks): nb = max(1, 64 / L) blocks lie side by side in the lanes when L <= 64, one block
// spans `chunks` steps of 64 lanes when it is longer.  Lane l of step s holds offset 64 s + l of the group in BOTH scans, so it
// reads back the S it stored itself.  The scans are Hillis-Steele over the lanes, cut at the block boundaries, with a carry from
// step to step (a longer block only).
template <bool MAX, bool MAP>
__global__ __launch_bounds__(TER_THREADS) void terrain_rows_kernel(const int* __restrict__ in, int h, int w, int r, int nb, int chunks,
                                                                   int groups, int* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const long long wave = (long long)blockIdx.x * TER_WAVES + (threadIdx.x >> 6);
  if (wave >= (long long)h * groups) return;                 // wave-uniform
  const int L = 2 * r + 1, span = nb * L;
  const int j = (int)(wave / groups), g = (int)(wave - (long long)j * groups);
  const long long row = (long long)j * w, p = (long long)g * span - r;      // the group's first a
  // suffix scan, the steps from the last to the first
  int carry = ter_identity<MAX>();
  for (int s = chunks - 1; s >= 0; --s) {
    const int off = s * 64 + lane, t = nb > 1 ? off % L : off;
    const bool live = off < span;
    const long long a = p + off;
    int v = live ? ter_load<MAX, MAP>(in, row + a, a, w) : ter_identity<MAX>();
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int o = __shfl_down(v, d, 64);
      if (lane + d < 64 && t + d < L) v = ter_op<MAX>(v, o);
    }
    v = ter_op<MAX>(v, carry);                               // the carry is the identity unless the block goes on in the next step
    carry = __shfl(v, 0, 64);
    const long long x = a + r;
    if (live && x < w) out[row + x] = v;                     // x >= 0: a >= -r
  }
  // exclusive prefix scan of the next block, the steps from the first to the last
  carry = ter_identity<MAX>();
  for (int s = 0; s < chunks; ++s) {
    const int off = s * 64 + lane, t = nb > 1 ? off % L : off;
    const bool live = off < span;
    const long long a = p + off, y = a + L - 1;              // G[t] as an inclusive scan ends at y; t = 0 has none
    int v = live && t > 0 ? ter_load<MAX, MAP>(in, row + y, y, w) : ter_identity<MAX>();
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int o = __shfl_up(v, d, 64);
      if (lane >= d && t - d >= 1) v = ter_op<MAX>(v, o);
    }
    v = ter_op<MAX>(v, carry);
    carry = __shfl(v, 63, 64);
    const long long x = a + r;
    if (live && x < w) out[row + x] = ter_op<MAX>(out[row + x], v);
  }
}

// Columns.  The lanes of a wave lie across 64 columns; a thread walks the offsets [t0, t1) of block m of its column: upwards for S
// (starting from carry_s, the extreme of the block's offsets from t1 on), parking it in out[x], then downwards for G (starting from
// carry_g, the extreme of the next block's cells below offset t0) and combining.  EPILOGUE (the last pass of the dilation): key_out
// and the flag update; returns the cells newly flagged.
template <bool MAX, bool EPILOGUE>
__device__ __forceinline__ unsigned ter_col_walks(const int* __restrict__ in, int h, int w, int r, int i, long long p, int t0, int t1,
                                                  int carry_s, int carry_g, int* __restrict__ out, const int* __restrict__ key_in,
                                                  long long threshold, unsigned char* __restrict__ flags) {
  const int L = 2 * r + 1;
  unsigned newly = 0;
  int run = carry_s;
#pragma unroll 4
  for (int t = t1 - 1; t >= t0; --t) {
    const long long a = p + t, x = a + r;
    run = ter_op<MAX>(run, ter_load<MAX, false>(in, a * w + i, a, h));
    if (x < h) out[x * w + i] = run;
  }
  run = carry_g;
#pragma unroll 4
  for (int t = t0; t < t1; ++t) {
    const long long x = p + t + r, y = p + L + t - 1;
    if (t > 0) run = ter_op<MAX>(run, ter_load<MAX, false>(in, y * w + i, y, h));
    if (x >= h) continue;
    const long long c = x * w + i;
    int v = ter_op<MAX>(out[c], run);
    if (EPILOGUE) {
      const int k = key_in[c];
      if (!ter_valid(k)) {
        v = SNERF_TERRAIN_HOLE;
      } else if (flags != nullptr && (long long)k - (long long)v > threshold) {
        const unsigned f = flags[c];
        if (!(f & SNERF_TERRAIN_FLAGGED)) {
          flags[c] = (unsigned char)(f | SNERF_TERRAIN_FLAGGED);
          newly++;
        }
      }
    }
    out[c] = v;
  }
  return newly;
}

// A short block (L < TER_SEG_MIN_L): blockDim = (64, 4), a thread walks the whole of block m of its column; the blocks of a column
// are independent and give the parallelism.
template <bool MAX, bool EPILOGUE>
__global__ __launch_bounds__(TER_THREADS) void terrain_cols_kernel(const int* __restrict__ in, int h, int w, int r, int blocks, int col_tiles,
                                                                   int* __restrict__ out, const int* __restrict__ key_in,
                                                                   long long threshold, unsigned char* __restrict__ flags,
                                                                   unsigned long long* __restrict__ stats) {
  const int tile = (int)(blockIdx.x % (unsigned)col_tiles);
  const long long m = (long long)(blockIdx.x / (unsigned)col_tiles) * TER_WAVES + threadIdx.y;
  const int i = tile * 64 + threadIdx.x;
  const int L = 2 * r + 1;
  unsigned long long newly = 0;
  if (i < w && m < blocks)
    newly = ter_col_walks<MAX, EPILOGUE>(in, h, w, r, i, m * L - r, 0, L, ter_identity<MAX>(), ter_identity<MAX>(), out, key_in, threshold,
                                         flags);
  if (EPILOGUE) {
    newly = wave_reduce(newly, OpSum());
    if (threadIdx.x == 0 && newly) atomicAdd(&stats[0], newly);
  }
}

// A long block: few blocks per column, long walks -- too few threads and too long a dependent chain.  blockDim = (64, TER_SEGS): a
// workgroup takes one block of 64 columns and cuts it into TER_SEGS segments, one per wave.  A first walk folds each segment of the
// block and of the next block into two totals, exchanged through LDS; every thread then starts its two walks from the totals of the
// segments behind (S) and ahead of (G) its own.  Four loads of the input per cell instead of two, for TER_SEGS times the threads.
constexpr int TER_SEGS = 16;
constexpr int TER_SEG_MIN_L = 64;
template <bool MAX, bool EPILOGUE>
__global__ __launch_bounds__(64 * TER_SEGS) void terrain_cols_seg_kernel(const int* __restrict__ in, int h, int w, int r, int col_tiles,
                                                                         int* __restrict__ out, const int* __restrict__ key_in,
                                                                         long long threshold, unsigned char* __restrict__ flags,
                                                                         unsigned long long* __restrict__ stats) {
  __shared__ int totals[2][TER_SEGS][64];
  const int tile = (int)(blockIdx.x % (unsigned)col_tiles), lane = threadIdx.x, seg = threadIdx.y;
  const long long m = blockIdx.x / (unsigned)col_tiles;      // the grid holds exactly the blocks of a column
  const int i = tile * 64 + lane;
  const bool mine = i < w;
  const int L = 2 * r + 1, len = (L + TER_SEGS - 1) / TER_SEGS;
  const int t0 = seg * len < L ? seg * len : L, t1 = t0 + len < L ? t0 + len : L;
  const long long p = m * L - r;
  int total_s = ter_identity<MAX>(), total_g = ter_identity<MAX>();
  if (mine) {
#pragma unroll 4
    for (int t = t0; t < t1; ++t) {
      const long long a = p + t, y = p + L + t - 1;
      total_s = ter_op<MAX>(total_s, ter_load<MAX, false>(in, a * w + i, a, h));
      if (t > 0) total_g = ter_op<MAX>(total_g, ter_load<MAX, false>(in, y * w + i, y, h));
    }
  }
  totals[0][seg][lane] = total_s;
  totals[1][seg][lane] = total_g;
  __syncthreads();
  int carry_s = ter_identity<MAX>(), carry_g = ter_identity<MAX>();
#pragma unroll
  for (int k = 0; k < TER_SEGS; ++k) {
    if (k > seg) carry_s = ter_op<MAX>(carry_s, totals[0][k][lane]);
    if (k < seg) carry_g = ter_op<MAX>(carry_g, totals[1][k][lane]);
  }
  unsigned long long newly = 0;
  if (mine) newly = ter_col_walks<MAX, EPILOGUE>(in, h, w, r, i, p, t0, t1, carry_s, carry_g, out, key_in, threshold, flags);
  if (EPILOGUE) {
    newly = wave_reduce(newly, OpSum());
    if (lane == 0 && newly) atomicAdd(&stats[0], newly);
  }
}

// ---- fill --------------------------------------------------------------------------------------------------------------------------
// The column of the nearest ground cell at or to the W (west) and at or to the E (east) of every cell, -1 for none: one wave per row,
// a max / min scan over the lanes with a carry from step to step.
__global__ __launch_bounds__(TER_THREADS) void terrain_fill_rows_kernel(const unsigned char* __restrict__ flags, int h, int w,
                                                                        int* __restrict__ west, int* __restrict__ east) {
  const int lane = threadIdx.x & 63;
  const long long j = (long long)blockIdx.x * TER_WAVES + (threadIdx.x >> 6);
  if (j >= h) return;                                        // wave-uniform
  const long long row = j * w;
  const int steps = (w + 63) / 64;
  int carry = -1;
  for (int s = 0; s < steps; ++s) {
    const long long i = (long long)s * 64 + lane;
    int v = i < w && flags[row + i] == 0 ? (int)i : -1;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int o = __shfl_up(v, d, 64);
      if (lane >= d && o > v) v = o;
    }
    v = carry > v ? carry : v;
    carry = __shfl(v, 63, 64);
    if (i < w) west[row + i] = v;
  }
  carry = INT_MAX;
  for (int s = steps - 1; s >= 0; --s) {
    const long long i = (long long)s * 64 + lane;
    int v = i < w && flags[row + i] == 0 ? (int)i : INT_MAX;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int o = __shfl_down(v, d, 64);
      if (lane + d < 64 && o < v) v = o;
    }
    v = carry < v ? carry : v;
    carry = __shfl(v, 0, 64);
    if (i < w) east[row + i] = v == INT_MAX ? -1 : v;
  }
}

// The row of the nearest ground cell at or to the N and at or to the S of every cell, -1 for none: one thread per column.
__global__ __launch_bounds__(TER_THREADS) void terrain_fill_cols_kernel(const unsigned char* __restrict__ flags, int h, int w,
                                                                        int* __restrict__ north, int* __restrict__ south) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= w) return;
  int last = -1;
#pragma unroll 8
  for (int j = 0; j < h; ++j) {
    const long long c = (long long)j * w + i;
    last = flags[c] == 0 ? j : last;
    north[c] = last;
  }
  last = -1;
#pragma unroll 8
  for (int j = h - 1; j >= 0; --j) {
    const long long c = (long long)j * w + i;
    last = flags[c] == 0 ? j : last;
    south[c] = last;
  }
}

// one thread per cell
__global__ __launch_bounds__(TER_THREADS) void terrain_fill_combine_kernel(const int* __restrict__ key, const unsigned char* __restrict__ flags,
                                                                           const float* __restrict__ alt, int h, int w, double z0, double q,
                                                                           const int* __restrict__ west, const int* __restrict__ east,
                                                                           const int* __restrict__ north, const int* __restrict__ south,
                                                                           float* __restrict__ dtm, float* __restrict__ ndsm,
                                                                           int* __restrict__ reach, unsigned long long* __restrict__ stats) {
  const long long cells = (long long)h * w;
  unsigned long long n_ground = 0, n_filled = 0, n_unreachable = 0;
  for (long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x; c < cells; c += (long long)gridDim.x * blockDim.x) {
    const float a = alt[c];
    float t_out, n_out;
    int r_out;
    if (flags[c] == 0) {
      t_out = a;
      n_out = 0.0f;
      r_out = 0;
      n_ground++;
    } else {
      const int j = (int)(c / w), i = (int)(c - (long long)j * w);
      const int at[4] = {west[c], east[c], north[c], south[c]};
      long long k[4];
      int d[4];
      long long b = LLONG_MAX;
      int nearest = INT_MAX;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        if (at[s] < 0) continue;
        k[s] = s < 2 ? key[(long long)j * w + at[s]] : key[(long long)at[s] * w + i];
        d[s] = s == 0 ? i - at[s] : s == 1 ? at[s] - i : s == 2 ? j - at[s] : at[s] - j;
        b = k[s] < b ? k[s] : b;
        nearest = d[s] < nearest ? d[s] : nearest;
      }
      if (nearest == INT_MAX) {
        t_out = n_out = __builtin_nanf("");
        r_out = -1;
        n_unreachable++;
      } else {
        double num = 0.0, den = 0.0;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          if (at[s] < 0) continue;
          num += (double)(k[s] - b) / (double)d[s];
          den += 1.0 / (double)d[s];
        }
        const double t = z0 + q * ((double)b + num / den);
        t_out = (float)t;
        n_out = isfinite(a) ? (float)((double)a - t) : __builtin_nanf("");
        r_out = nearest;
        n_filled++;
      }
    }
    dtm[c] = t_out;
    ndsm[c] = n_out;
    if (reach != nullptr) reach[c] = r_out;
  }
  n_ground = wave_reduce(n_ground, OpSum());
  n_filled = wave_reduce(n_filled, OpSum());
  n_unreachable = wave_reduce(n_unreachable, OpSum());
  if ((threadIdx.x & 63) == 0) {
    if (n_ground) atomicAdd(&stats[0], n_ground);
    if (n_filled) atomicAdd(&stats[1], n_filled);
    if (n_unreachable) atomicAdd(&stats[2], n_unreachable);
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
constexpr unsigned TER_MAX_BLOCKS = 65536;               // cells beyond it are taken in a grid-stride

// the four passes' launch shapes: every count below fits 32 bits for h * w < 2^31 (a group or a block holds at least 3 cells)
struct TerPassShape {
  int nb, chunks, groups;            // rows: blocks per wave, steps per wave, waves per row
  unsigned row_grid;
  int blocks, col_tiles;             // columns: blocks per column, tiles of 64 columns
  bool segmented;                    // a long block: one workgroup of TER_SEGS waves per (tile, block)
  unsigned col_grid;
  dim3 col_block;
};
static TerPassShape terrain_pass_shape(int h, int w, int radius) {
  TerPassShape s;
  const int L = 2 * radius + 1;
  s.nb = L <= 64 ? 64 / L : 1;
  s.chunks = (s.nb * L + 63) / 64;
  s.groups = (int)(((long long)w + (long long)s.nb * L - 1) / ((long long)s.nb * L));
  s.row_grid = (unsigned)(((long long)h * s.groups + TER_WAVES - 1) / TER_WAVES);
  s.blocks = (int)(((long long)h + L - 1) / L);
  s.col_tiles = (w + 63) / 64;
  s.segmented = L >= TER_SEG_MIN_L;
  s.col_grid = (unsigned)((long long)s.col_tiles * (s.segmented ? s.blocks : (s.blocks + TER_WAVES - 1) / TER_WAVES));
  s.col_block = s.segmented ? dim3(64, TER_SEGS) : dim3(64, TER_WAVES);
  return s;
}

}  // namespace snerf

using namespace snerf;

extern "C" long long snerf_terrain_workspace_bytes(int h, int w) {
  if (!lattice_cells_ok("snerf_terrain_workspace_bytes", h, w)) return -1;
  return 16LL * h * w;
}

extern "C" int snerf_terrain_keys(const float* alt, const unsigned char* label, int h, int w, const unsigned char* blocked_host,
                                  double z0, double q, int* key, unsigned char* flags, unsigned long long* stats, void* stream) {
  const char* who = "snerf_terrain_keys";
  if (!alt || !key || !flags || !stats) { set_error("%s: null pointer", who); return SNERF_ERR_NULL; }
  if ((label == nullptr) != (blocked_host == nullptr)) {
    set_error("%s: label and blocked_host are both given or both null (label %s, blocked_host %s)", who, label ? "given" : "null",
              blocked_host ? "given" : "null");
    return SNERF_ERR_NULL;
  }
  if (!lattice_cells_ok(who, h, w)) return SNERF_ERR_BAD_DESC;
  if (!quant_ok(who, z0, q)) return SNERF_ERR_BAD_DESC;
  TerClasses blocked = {{0, 0, 0, 0}};
  if (blocked_host) {
    if (blocked_host[255]) {
      set_error("%s: blocked_host[255] is set: class 255 means no label and is in no set", who);
      return SNERF_ERR_BAD_DESC;
    }
    for (int c = 0; c < 256; ++c)
      if (blocked_host[c]) blocked.bits[c >> 6] |= 1ull << (c & 63);
  }
  const long long cells = (long long)h * w;
  hipLaunchKernelGGL(terrain_keys_kernel, dim3(blocks_for(cells, TER_THREADS, TER_MAX_BLOCKS)), dim3(TER_THREADS), 0, (hipStream_t)stream,
                     alt, label, cells, blocked, z0, q, key, flags, stats);
  SNERF_LAUNCH_CHECK();
  return SNERF_OK;
}

extern "C" int snerf_terrain_open(const int* key_in, int h, int w, int radius, long long threshold, int* key_out, unsigned char* flags,
                                  void* ws, unsigned long long* stats, void* stream) {
  const char* who = "snerf_terrain_open";
  if (!key_in || !key_out || !ws || !stats) { set_error("%s: null pointer", who); return SNERF_ERR_NULL; }
  if (!lattice_cells_ok(who, h, w)) return SNERF_ERR_BAD_DESC;
  if (radius < 1 || radius > SNERF_TERRAIN_MAX_RADIUS) {
    set_error("%s: radius must lie in [1, %d] (radius = %d)", who, SNERF_TERRAIN_MAX_RADIUS, radius);
    return SNERF_ERR_BAD_DESC;
  }
  if (threshold < 0) { set_error("%s: threshold must be >= 0 (threshold = %lld)", who, threshold); return SNERF_ERR_BAD_DESC; }
  if (key_out == key_in) { set_error("%s: key_out must not alias key_in", who); return SNERF_ERR_BAD_DESC; }
  const TerPassShape s = terrain_pass_shape(h, w, radius);
  int* plane0 = (int*)ws;
  int* plane1 = plane0 + (long long)h * w;
  const dim3 row_block(TER_THREADS);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL((terrain_rows_kernel<false, true>), dim3(s.row_grid), row_block, 0, st, key_in, h, w, radius, s.nb, s.chunks, s.groups,
                     plane0);
  SNERF_LAUNCH_CHECK();
  if (s.segmented)
    hipLaunchKernelGGL((terrain_cols_seg_kernel<false, false>), dim3(s.col_grid), s.col_block, 0, st, (const int*)plane0, h, w, radius,
                       s.col_tiles, plane1, (const int*)nullptr, 0LL, (unsigned char*)nullptr, (unsigned long long*)nullptr);
  else
    hipLaunchKernelGGL((terrain_cols_kernel<false, false>), dim3(s.col_grid), s.col_block, 0, st, (const int*)plane0, h, w, radius, s.blocks,
                       s.col_tiles, plane1, (const int*)nullptr, 0LL, (unsigned char*)nullptr, (unsigned long long*)nullptr);
  SNERF_LAUNCH_CHECK();
  hipLaunchKernelGGL((terrain_rows_kernel<true, true>), dim3(s.row_grid), row_block, 0, st, (const int*)plane1, h, w, radius, s.nb, s.chunks,
                     s.groups, plane0);
  SNERF_LAUNCH_CHECK();
  if (s.segmented)
    hipLaunchKernelGGL((terrain_cols_seg_kernel<true, true>), dim3(s.col_grid), s.col_block, 0, st, (const int*)plane0, h, w, radius,
                       s.col_tiles, key_out, key_in, threshold, flags, stats);
  else
    hipLaunchKernelGGL((terrain_cols_kernel<true, true>), dim3(s.col_grid), s.col_block, 0, st, (const int*)plane0, h, w, radius, s.blocks,
                       s.col_tiles, key_out, key_in, threshold, flags, stats);
  SNERF_LAUNCH_CHECK();
  return SNERF_OK;
}

extern "C" int snerf_terrain_fill(const int* key, const unsigned char* flags, const float* alt, int h, int w, double z0, double q,
                                  float* dtm, float* ndsm, int* reach, void* ws, unsigned long long* stats, void* stream) {
  const char* who = "snerf_terrain_fill";
  if (!key || !flags || !alt || !dtm || !ndsm || !ws || !stats) { set_error("%s: null pointer", who); return SNERF_ERR_NULL; }
  if (!lattice_cells_ok(who, h, w)) return SNERF_ERR_BAD_DESC;
  if (!quant_ok(who, z0, q)) return SNERF_ERR_BAD_DESC;
  const long long cells = (long long)h * w;
  int* west = (int*)ws;
  int *east = west + cells, *north = east + cells, *south = north + cells;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(terrain_fill_rows_kernel, dim3((unsigned)(((long long)h + TER_WAVES - 1) / TER_WAVES)), dim3(TER_THREADS), 0, st, flags,
                     h, w, west, east);
  SNERF_LAUNCH_CHECK();
  hipLaunchKernelGGL(terrain_fill_cols_kernel, dim3((unsigned)(((long long)w + TER_THREADS - 1) / TER_THREADS)), dim3(TER_THREADS), 0, st,
                     flags, h, w, north, south);
  SNERF_LAUNCH_CHECK();
  hipLaunchKernelGGL(terrain_fill_combine_kernel, dim3(blocks_for(cells, TER_THREADS, TER_MAX_BLOCKS)), dim3(TER_THREADS), 0, st, key, flags,
                     alt, h, w, z0, q, (const int*)west, (const int*)east, (const int*)north, (const int*)south, dtm, ndsm, reach, stats);
  SNERF_LAUNCH_CHECK();
  return SNERF_OK;
}
