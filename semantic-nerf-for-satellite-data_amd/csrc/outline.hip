// Outlines on the map: the boundary rings of the objects of an id raster.  Every boundary edge finds its successor in the 2 x 2 cells
// at its head (sides, link), the rings are the cycles of that permutation, ordered by pointer jumping (rank: a minimum over the
// cycle, a cut in front of its start, Wyllie's list ranking with two sums), and one thread per edge writes the corners and folds the
// per-ring words (emit: a reduction inside the wave over the lanes that share a ring, then one lane's integer atomics).  The spec is
// include/snerf_outline.h and DESIGN.md section 5ze.  Integers only; every trip count is fixed on the host, and every index read
// from a buffer is range-checked before it is used.
#include "outline_common.h"
#include "../../include/snerf_outline.h"

namespace snerf {

// ---- sides -------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(OUT_THREADS) void outline_sides_kernel(IdRaster g, long long cells, unsigned char* __restrict__ sides,
                                                                    unsigned long long* __restrict__ stats) {
  unsigned long long bad = 0, object_cells = 0, edges = 0, corners = 0;
  for (long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x; c < cells; c += (long long)gridDim.x * blockDim.x) {
    const int raw = g.ids[c];
    const bool out = raw < 0 || raw > g.K;
    bad += out ? 1 : 0;
    const int n = out ? 0 : raw;
    unsigned mask = 0;
    if (n > 0) {
      const int j = (int)c / g.w, i = (int)c - j * g.w;          // c < 2^29: a 32-bit division
      object_cells++;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        if (g.at(j + step_j((s + 3) & 3), i + step_i((s + 3) & 3)) == n) continue;
        mask |= 1u << s;
        edges++;
        corners += is_corner(g, j, i, s, n) ? 1 : 0;
      }
    }
    sides[c] = (unsigned char)mask;
  }
  unsigned long long counts[4] = {bad, object_cells, edges, corners};
  add_counts(counts, stats);
}

// ---- link --------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(OUT_THREADS) void outline_link_kernel(IdRaster g, long long cells, const unsigned char* __restrict__ sides,
                                                                   const int* __restrict__ offsets, int connectivity, long long E,
                                                                   int* __restrict__ slot, int* __restrict__ next, int* __restrict__ flags,
                                                                   unsigned long long* __restrict__ stats) {
  unsigned long long trips = 0, written = 0;
  for (long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x; c < cells; c += (long long)gridDim.x * blockDim.x) {
    const int raw = g.ids[c];
    const int n = (raw < 0 || raw > g.K) ? 0 : raw;
    const unsigned mask = sides[c] & 15u;
    if (n == 0 || mask == 0) continue;
    const int j = (int)c / g.w, i = (int)c - j * g.w;          // c < 2^29: a 32-bit division
    long long p = offsets[c];
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      if (!((mask >> d) & 1u)) continue;
      const int bj = j + step_j(d), bi = i + step_i(d);
      const int aj = bj + step_j((d + 3) & 3), ai = bi + step_i((d + 3) & 3);
      const bool B = g.at(bj, bi) == n, A = g.at(aj, ai) == n;
      int tj = j, ti = i, ts = (d + 1) & 3;
      if (A && (B || connectivity == 8)) {
        tj = aj, ti = ai, ts = (d + 3) & 3;
      } else if (B) {
        tj = bj, ti = bi, ts = d;
      }
      // (tj, ti) carries n, so it lies inside the raster
      const long long t = (long long)tj * g.w + ti;
      const long long tp = (long long)offsets[t] + __popc(sides[t] & ((1u << ts) - 1u));
      if (p < 0 || p >= E || tp < 0 || tp >= E) {
        trips++;
      } else {
        slot[p] = (int)(4 * c + d);
        next[p] = (int)tp;
        flags[p] = (is_corner(g, j, i, d, n) ? SNERF_OUTLINE_CORNER : 0) | d << 1;
        written++;
      }
      p++;
    }
  }
  unsigned long long counts[2] = {trips, written};
  add_counts(counts, stats);
}

// ---- rank --------------------------------------------------------------------------------------------------------------------------
// next[p], or p where it is no index
__device__ __forceinline__ int next_of(const int* __restrict__ next, long long p, long long E) {
  const int t = next[p];
  return (t < 0 || t >= E) ? (int)p : t;
}

__global__ __launch_bounds__(OUT_THREADS) void outline_min_init_kernel(const int* __restrict__ next, long long E, int* __restrict__ m,
                                                                       int* __restrict__ t, unsigned long long* __restrict__ stats) {
  unsigned long long bad = 0;
  for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < E; p += (long long)gridDim.x * blockDim.x) {
    const int raw = next[p];
    const bool out = raw < 0 || raw >= E;
    bad += out ? 1 : 0;
    m[p] = (int)p;
    t[p] = out ? (int)p : raw;
  }
  unsigned long long counts[1] = {bad};
  add_counts(counts, stats);
}

// m, t hold indices this entry wrote itself: in [0, E)
__global__ __launch_bounds__(OUT_THREADS) void outline_min_round_kernel(const int* __restrict__ m, const int* __restrict__ t, long long E,
                                                                        int* __restrict__ m_out, int* __restrict__ t_out) {
  for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < E; p += (long long)gridDim.x * blockDim.x) {
    const int tp = t[p];
    const int a = m[p], b = m[tp];
    m_out[p] = b < a ? b : a;
    t_out[p] = t[tp];
  }
}

__global__ __launch_bounds__(OUT_THREADS) void outline_cut_kernel(const int* __restrict__ next, const int* __restrict__ flags,
                                                                  const int* __restrict__ ring, long long E, int* __restrict__ q,
                                                                  unsigned* __restrict__ u, unsigned* __restrict__ v) {
  for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < E; p += (long long)gridDim.x * blockDim.x) {
    const int t = next_of(next, p, E);
    const bool cut = ring[t] == t;
    q[p] = cut ? OUT_NIL : t;
    u[p] = cut ? 0u : 1u;
    v[p] = cut ? 0u : (unsigned)(flags[t] & SNERF_OUTLINE_CORNER);
  }
}

__global__ __launch_bounds__(OUT_THREADS) void outline_jump_kernel(const int* __restrict__ q, const unsigned* __restrict__ u,
                                                                   const unsigned* __restrict__ v, long long E, int* __restrict__ q_out,
                                                                   unsigned* __restrict__ u_out, unsigned* __restrict__ v_out) {
  for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < E; p += (long long)gridDim.x * blockDim.x) {
    const int t = q[p];
    unsigned a = u[p], b = v[p];
    int t2 = OUT_NIL;
    if (t != OUT_NIL) {
      a += u[t];
      b += v[t];
      t2 = q[t];
    }
    q_out[p] = t2;
    u_out[p] = a;
    v_out[p] = b;
  }
}

__global__ __launch_bounds__(OUT_THREADS) void outline_finish_kernel(const int* __restrict__ flags, const int* __restrict__ ring,
                                                                     const unsigned* __restrict__ u, const unsigned* __restrict__ v,
                                                                     long long E, int* __restrict__ rank, int* __restrict__ ordinal,
                                                                     int* __restrict__ totals) {
  for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < E; p += (long long)gridDim.x * blockDim.x) {
    const int s = ring[p];                                 // a minimum of indices: in [0, E)
    const unsigned L = u[s] + 1u, C = v[s] + (unsigned)(flags[s] & SNERF_OUTLINE_CORNER);
    rank[p] = (int)(L - 1u - u[p]);
    ordinal[p] = (int)(C - v[p] - (unsigned)(flags[p] & SNERF_OUTLINE_CORNER));
    const bool start = s == p;
    totals[2 * p] = start ? (int)L : 0;
    totals[2 * p + 1] = start ? (int)C : 0;
  }
}

__global__ __launch_bounds__(OUT_THREADS) void outline_check_kernel(const int* __restrict__ next, const int* __restrict__ ring,
                                                                    const int* __restrict__ rank, const int* __restrict__ totals, long long E,
                                                                    unsigned long long* __restrict__ stats) {
  unsigned long long trips = 0, edges = 0;
  for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < E; p += (long long)gridDim.x * blockDim.x) {
    const int t = next_of(next, p, E);
    trips += ring[t] != ring[p] ? 1 : 0;
    trips += (t != ring[p] && (unsigned)rank[t] != (unsigned)rank[p] + 1u) ? 1 : 0;
    edges += (unsigned)totals[2 * p];
  }
  unsigned long long counts[2] = {trips, edges};
  add_counts(counts, stats);
}

// ---- emit --------------------------------------------------------------------------------------------------------------------------
// What a wave has folded for one ring and not yet added to its row: the same in every lane.
struct RingFold {
  int row;                                                   // -1: nothing is held
  unsigned edges, corners, id, min_x, max_x, min_y, max_y;
  long long area;
};

__device__ __forceinline__ void flush_fold(const RingFold& f, unsigned long long* __restrict__ rows) {
  unsigned long long* out = rows + (long long)f.row * SNERF_OUTLINE_ROW_WORDS;
  atomicAdd(&out[0], (unsigned long long)f.edges);
  if (f.corners) atomicAdd(&out[1], (unsigned long long)f.corners);
  atomicMax(&out[2], (unsigned long long)f.id);
  if (f.area) atomicAdd(&out[3], (unsigned long long)f.area);
  atomicMin(&out[4], (unsigned long long)f.min_x);
  atomicMax(&out[5], (unsigned long long)f.max_x);
  atomicMin(&out[6], (unsigned long long)f.min_y);
  atomicMax(&out[7], (unsigned long long)f.max_y);
}

// One thread per edge.  A thread places its own corner; the wave then takes the first lane that still has a ring, ballots the lanes
// of that ring and reduces their values across the wave (the others hold the identities).  The result is HELD while the next group
// belongs to the same ring -- through the trips of the grid-stride too -- and one lane issues the row's atomics when the ring changes
// and at the end: a ring as long as the raster costs a wave one set of atomics, not one per 64 edges.  The words are integer sums and
// extremes: the grouping does not show in them.
__global__ __launch_bounds__(OUT_THREADS) void outline_emit_kernel(const int* __restrict__ ids, const int* __restrict__ slot,
                                                                   const int* __restrict__ flags, const int* __restrict__ ring,
                                                                   const int* __restrict__ ordinal, const int* __restrict__ ring_row,
                                                                   const long long* __restrict__ vertex_offset, int w, long long slots,
                                                                   long long E, long long n_rings, long long V, int* __restrict__ vertices,
                                                                   unsigned long long* __restrict__ rows, unsigned long long* __restrict__ stats) {
  const int lane = threadIdx.x & 63;
  unsigned long long trips = 0, placed = 0;
  RingFold held = {-1, 0, 0, 0, 0, 0, 0, 0, 0};
  // every thread of a workgroup makes the same number of trips: the wave's ballots and shuffles run with all lanes
  for (long long base = (long long)blockIdx.x * blockDim.x; base < E; base += (long long)gridDim.x * blockDim.x) {
    const long long p = base + threadIdx.x;
    int row = -1;
    unsigned corner = 0, id = 0, x0 = 0, y0 = 0;
    long long area = 0;
    if (p < E) {
      const int sl = slot[p], s0 = ring[p];
      if (sl < 0 || sl >= slots || s0 < 0 || s0 >= E) {
        trips++;
      } else {
        const int r = ring_row[s0];
        if (r < 0 || r >= n_rings) {
          trips++;
        } else {
          row = r;
          const int c = sl >> 2, s = sl & 3;
          const int j = c / w, i = c - j * w;
          x0 = (unsigned)(i + (s == 1 || s == 2 ? 1 : 0));
          y0 = (unsigned)(j + (s == 2 || s == 3 ? 1 : 0));
          const long long x1 = (long long)x0 + step_i(s), y1 = (long long)y0 + step_j(s);
          area = (long long)x0 * y1 - x1 * (long long)y0;
          const int raw = ids[c];
          id = raw < 0 ? 0u : (unsigned)raw;
          corner = (unsigned)(flags[p] & SNERF_OUTLINE_CORNER);
          if (corner) {
            // the offset is checked before anything is added to it: both terms then fit 32 bits and the sum cannot wrap
            const long long first = vertex_offset[r];
            const long long at = (first < 0 || first > V) ? -1 : first + ordinal[p];
            if (at < 0 || at >= V) {
              trips++;
            } else {
              vertices[2 * at] = (int)x0;
              vertices[2 * at + 1] = (int)y0;
              placed++;
            }
          }
        }
      }
    }
    unsigned long long todo = __ballot(row >= 0);
    while (todo) {                                           // wave-uniform: `todo` is the same word in every lane
      const int leader = __ffsll((long long)todo) - 1;
      const int group = __shfl(row, leader, 64);
      const bool in = row == group;                          // (group >= 0: a lane of `todo`)
      todo &= ~__ballot(in);
      RingFold f;
      f.row = group;
      f.edges = wave_reduce(in ? 1u : 0u, OpSum());
      f.corners = wave_reduce(in ? corner : 0u, OpSum());
      f.id = wave_reduce(in ? id : 0u, OpMax());
      f.area = wave_reduce(in ? area : 0ll, OpSum());
      f.min_x = wave_reduce(in ? x0 : 0xFFFFFFFFu, OpMin());
      f.max_x = wave_reduce(in ? x0 : 0u, OpMax());
      f.min_y = wave_reduce(in ? y0 : 0xFFFFFFFFu, OpMin());
      f.max_y = wave_reduce(in ? y0 : 0u, OpMax());
      if (held.row == group) {                               // wave-uniform: both are the same in every lane
        held.edges += f.edges;
        held.corners += f.corners;
        held.id = f.id > held.id ? f.id : held.id;
        held.area += f.area;
        held.min_x = f.min_x < held.min_x ? f.min_x : held.min_x;
        held.max_x = f.max_x > held.max_x ? f.max_x : held.max_x;
        held.min_y = f.min_y < held.min_y ? f.min_y : held.min_y;
        held.max_y = f.max_y > held.max_y ? f.max_y : held.max_y;
      } else {
        if (held.row >= 0 && lane == 0) flush_fold(held, rows);
        held = f;
      }
    }
  }
  if (held.row >= 0 && lane == 0) flush_fold(held, rows);
  unsigned long long counts[2] = {trips, placed};
  add_counts(counts, stats);
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
constexpr long long OUT_MAX_EDGES = 1LL << 31;

static bool outline_cells_ok(const char* who, int h, int w) {
  if (h < 1 || w < 1) { set_error("%s: h and w must be >= 1 (h = %d, w = %d)", who, h, w); return false; }
  if ((long long)h * w >= SNERF_OUTLINE_MAX_CELLS) { set_error("%s: h * w must be below 2^29 (h = %d, w = %d)", who, h, w); return false; }
  return true;
}

static bool outline_ids_ok(const char* who, long long K) {
  if (K >= 0 && K < OUT_MAX_EDGES) return true;
  set_error("%s: K must lie in [0, 2^31) (K = %lld)", who, K);
  return false;
}

static bool outline_count_ok(const char* who, const char* what, long long n, int h, int w) {
  if (n >= 0 && n <= 4LL * h * w) return true;
  set_error("%s: %s must lie in [0, 4 h w] (%s = %lld, h = %d, w = %d)", who, what, what, n, h, w);
  return false;
}

static int outline_rounds(long long E) {
  int R = 1;
  while ((1LL << R) < E) ++R;
  return R;
}

}  // namespace snerf

using namespace snerf;

extern "C" int snerf_outline_sides(const int* ids, int h, int w, long long K, unsigned char* sides, unsigned long long* stats,
                                   void* stream) {
  const char* who = "snerf_outline_sides";
  if (!ids || !sides || !stats) { set_error("%s: null pointer", who); return SNERF_ERR_NULL; }
  if (!outline_cells_ok(who, h, w) || !outline_ids_ok(who, K)) return SNERF_ERR_BAD_DESC;
  const long long cells = (long long)h * w;
  const IdRaster g = {ids, h, w, K};
  hipLaunchKernelGGL(outline_sides_kernel, dim3(blocks_for(cells, OUT_THREADS, OUT_COUNT_BLOCKS)), dim3(OUT_THREADS), 0, (hipStream_t)stream, g,
                     cells, sides, stats);
  SNERF_LAUNCH_CHECK();
  return SNERF_OK;
}

extern "C" int snerf_outline_link(const int* ids, const unsigned char* sides, const int* offsets, int h, int w, long long K,
                                  int connectivity, long long E, int* slot, int* next, int* flags, unsigned long long* stats, void* stream) {
  const char* who = "snerf_outline_link";
  if (!ids || !sides || !offsets || !stats || (E > 0 && (!slot || !next || !flags))) { set_error("%s: null pointer", who); return SNERF_ERR_NULL; }
  if (!outline_cells_ok(who, h, w) || !outline_ids_ok(who, K)) return SNERF_ERR_BAD_DESC;
  if (connectivity != 4 && connectivity != 8) {
    set_error("%s: connectivity must be 4 or 8 (connectivity = %d)", who, connectivity);
    return SNERF_ERR_BAD_DESC;
  }
  if (!outline_count_ok(who, "E", E, h, w)) return SNERF_ERR_BAD_DESC;
  if (E == 0) return SNERF_OK;
  const long long cells = (long long)h * w;
  const IdRaster g = {ids, h, w, K};
  hipLaunchKernelGGL(outline_link_kernel, dim3(blocks_for(cells, OUT_THREADS, OUT_COUNT_BLOCKS)), dim3(OUT_THREADS), 0, (hipStream_t)stream, g,
                     cells, sides, offsets, connectivity, E, slot, next, flags, stats);
  SNERF_LAUNCH_CHECK();
  return SNERF_OK;
}

extern "C" long long snerf_outline_workspace_bytes(long long E) {
  if (E < 0 || E >= OUT_MAX_EDGES) {
    set_error("snerf_outline_workspace_bytes: E must lie in [0, 2^31) (E = %lld)", E);
    return -1;
  }
  return 6 * E * (long long)sizeof(int);
}

extern "C" int snerf_outline_rank(const int* next, const int* flags, long long E, int* ring, int* rank, int* ordinal, int* totals,
                                  void* workspace, long long workspace_bytes, unsigned long long* stats, void* stream) {
  const char* who = "snerf_outline_rank";
  if (!stats || (E > 0 && (!next || !flags || !ring || !rank || !ordinal || !totals || !workspace))) {
    set_error("%s: null pointer", who);
    return SNERF_ERR_NULL;
  }
  if (E < 0 || E >= OUT_MAX_EDGES) { set_error("%s: E must lie in [0, 2^31) (E = %lld)", who, E); return SNERF_ERR_BAD_DESC; }
  if ((uintptr_t)workspace % sizeof(int) != 0) { set_error("%s: the workspace must be 4-byte aligned", who); return SNERF_ERR_BAD_DESC; }
  const long long need = 6 * E * (long long)sizeof(int);
  if (workspace_bytes < need) {
    set_error("%s: the workspace holds %lld bytes, %lld are needed (snerf_outline_workspace_bytes)", who, workspace_bytes, need);
    return SNERF_ERR_BAD_DESC;
  }
  if (E == 0) return SNERF_OK;
  const int R = outline_rounds(E);
  const dim3 grid(blocks_for(E, OUT_THREADS, OUT_MAX_BLOCKS)), counting(blocks_for(E, OUT_THREADS, OUT_COUNT_BLOCKS)), block(OUT_THREADS);
  hipStream_t st = (hipStream_t)stream;
  int* A[6];
  for (int k = 0; k < 6; ++k) A[k] = (int*)workspace + k * E;
  // 1. the minimum over the cycle: m in A0 / A1, t in A2 / A3; the last round writes m into `ring`
  hipLaunchKernelGGL(outline_min_init_kernel, counting, block, 0, st, next, E, A[0], A[2], stats);
  for (int r = 0; r < R; ++r) {
    const int from = r & 1, to = from ^ 1;
    hipLaunchKernelGGL(outline_min_round_kernel, grid, block, 0, st, A[from], A[2 + from], E, r == R - 1 ? ring : A[to], A[2 + to]);
  }
  // 2., 3. the cut and the ranking: q in A0 / A1, u in A2 / A3, v in A4 / A5
  hipLaunchKernelGGL(outline_cut_kernel, grid, block, 0, st, next, flags, ring, E, A[0], (unsigned*)A[2], (unsigned*)A[4]);
  for (int r = 0; r < R; ++r) {
    const int from = r & 1, to = from ^ 1;
    hipLaunchKernelGGL(outline_jump_kernel, grid, block, 0, st, A[from], (unsigned*)A[2 + from], (unsigned*)A[4 + from], E, A[to],
                       (unsigned*)A[2 + to], (unsigned*)A[4 + to]);
  }
  const int last = R & 1;
  hipLaunchKernelGGL(outline_finish_kernel, grid, block, 0, st, flags, ring, (unsigned*)A[2 + last], (unsigned*)A[4 + last], E, rank, ordinal,
                     totals);
  hipLaunchKernelGGL(outline_check_kernel, counting, block, 0, st, next, ring, rank, totals, E, stats);
  SNERF_LAUNCH_CHECK();
  return SNERF_OK;
}

extern "C" int snerf_outline_emit(const int* ids, const int* slot, const int* flags, const int* ring, const int* ordinal,
                                  const int* ring_row, const long long* vertex_offset, int h, int w, long long E, long long n_rings,
                                  long long V, int* vertices, unsigned long long* rows, unsigned long long* stats, void* stream) {
  const char* who = "snerf_outline_emit";
  if (!ids || !stats || (E > 0 && (!slot || !flags || !ring || !ordinal || !ring_row || !vertex_offset || !vertices || !rows))) {
    set_error("%s: null pointer", who);
    return SNERF_ERR_NULL;
  }
  if (!outline_cells_ok(who, h, w)) return SNERF_ERR_BAD_DESC;
  if (!outline_count_ok(who, "E", E, h, w) || !outline_count_ok(who, "n_rings", n_rings, h, w) || !outline_count_ok(who, "V", V, h, w))
    return SNERF_ERR_BAD_DESC;
  if (E == 0) return SNERF_OK;
  hipLaunchKernelGGL(outline_emit_kernel, dim3(blocks_for(E, OUT_THREADS, OUT_COUNT_BLOCKS)), dim3(OUT_THREADS), 0, (hipStream_t)stream, ids, slot,
                     flags, ring, ordinal, ring_row, vertex_offset, w, 4LL * h * w, E, n_rings, V, vertices, rows, stats);
  SNERF_LAUNCH_CHECK();
  return SNERF_OK;
}
