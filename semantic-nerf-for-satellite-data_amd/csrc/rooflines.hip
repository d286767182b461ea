// Roof lines on the map: the kept facets grown over the building cells the facet filter dropped (grow: one Jacobi launch per round, a
// taker joins the neighbouring facet of its building whose plane it fits best), and the arcs of a partition -- the runs of boundary
// edges between two nodes, on top of what the outline entries wrote (first: the node bit of every edge's tail and every ring's first
// break; mark: left, twin and the ring-ordered position of every edge; fold: one thread per position writes the arcs' vertices and
// folds the per-arc words, a reduction inside the wave over the lanes that share an arc, held while the arc stays, then one lane's
// integer atomics).  The spec is include/snerf_rooflines.h and DESIGN.md section 5zf; tests/rooflines_numpy.py restates it.  Every
// trip count is fixed on the host, and every index read from a buffer is range-checked before it is used.
#include "outline_common.h"
#include "roof_plane.h"
#include "../../include/snerf_outline.h"
#include "../../include/snerf_rooflines.h"
#include "../../include/snerf_roofs.h"

#include <cmath>

namespace snerf {

// ---- grow --------------------------------------------------------------------------------------------------------------------------
// One thread per cell.  Only a taker reads more than its own three words: its four neighbours' facets and objects, and per candidate
// the facet's root, the root's key and the plane.
__global__ __launch_bounds__(OUT_THREADS) void roofs_grow_kernel(const int* __restrict__ in, const int* __restrict__ ids,
                                                                 const int* __restrict__ key, const int* __restrict__ facet_root,
                                                                 const double* __restrict__ planes, int h, int w, long long F, double unit,
                                                                 long long max_rq, int* __restrict__ out,
                                                                 unsigned long long* __restrict__ assigned_word,
                                                                 unsigned long long* __restrict__ guard_word) {
  const long long cells = (long long)h * w;
  unsigned long long assigned = 0, trips = 0;
  for (long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x; c < cells; c += (long long)gridDim.x * blockDim.x) {
    const int own = in[c];
    int result = own;
    if (own < 0 || own > F) {
      trips++;
    } else if (own == 0 && ids[c] > 0 && roof_valid(key[c])) {
      const int oid = ids[c], kc = key[c];
      const int j = (int)(c / w), i = (int)(c - (long long)j * w);
      int best_n = 0;
      long long best_rq = 0;
#pragma unroll
      for (int d = 0; d < 4; ++d) {                          // N, E, S, W
        const int nj = j + (d == 0 ? -1 : d == 2 ? 1 : 0), ni = i + (d == 1 ? 1 : d == 3 ? -1 : 0);
        if (nj < 0 || nj >= h || ni < 0 || ni >= w) continue;
        const long long t = (long long)nj * w + ni;
        const int n = in[t];
        if (n < 1 || n > F || ids[t] != oid) continue;
        const double* p = planes + (long long)(n - 1) * 3;
        const double gamma = p[0], alpha = p[1], beta = p[2];
        if (!(isfinite(gamma) && isfinite(alpha) && isfinite(beta))) continue;
        const int rt = facet_root[n - 1];
        if (rt < 0 || rt >= cells) { trips++; continue; }
        const int k0 = key[rt];
        if (!roof_valid(k0)) continue;
        const int j0 = rt / w, i0 = rt - j0 * w;
        const RoofMisfit m = roof_misfit(gamma, alpha, beta, i - i0, j - j0, (long long)kc - k0, unit);
        const long long mag = m.rq < 0 ? -m.rq : m.rq;
        if (m.clamped || mag > max_rq) continue;
        if (best_n == 0 || mag < best_rq || (mag == best_rq && n < best_n)) { best_n = n; best_rq = mag; }
      }
      if (best_n > 0) { result = best_n; assigned++; }
    }
    out[c] = result;
  }
  unsigned long long counts[2] = {assigned, trips};
  __shared__ unsigned long long partial[2][OUT_THREADS / 64];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const unsigned long long sum = wave_reduce(counts[k], OpSum());
    if ((threadIdx.x & 63) == 0) partial[k][threadIdx.x >> 6] = sum;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long a = 0, g = 0;
    for (int wave = 0; wave < OUT_THREADS / 64; ++wave) { a += partial[0][wave]; g += partial[1][wave]; }
    if (a) atomicAdd(assigned_word, a);
    if (g) atomicAdd(guard_word, g);
  }
}

// ---- arcs --------------------------------------------------------------------------------------------------------------------------
// the tail of the edge of side s of cell (j, i), as snerf_outline_emit forms it
__device__ __forceinline__ int tail_x(int i, int s) { return i + (s == 1 || s == 2 ? 1 : 0); }
__device__ __forceinline__ int tail_y(int j, int s) { return j + (s == 2 || s == 3 ? 1 : 0); }

// a node: at least three cracks among the four cells round the vertex (x, y)
__device__ __forceinline__ bool is_node(const IdRaster& g, int x, int y) {
  const int nw = g.at(y - 1, x - 1), ne = g.at(y - 1, x), se = g.at(y, x), sw = g.at(y, x - 1);
  return (nw != ne) + (ne != se) + (se != sw) + (sw != nw) >= 3;
}

__global__ __launch_bounds__(OUT_THREADS) void arcs_first_kernel(IdRaster g, const int* __restrict__ slot, const int* __restrict__ ring,
                                                                 const int* __restrict__ rank, long long slots, long long E,
                                                                 int* __restrict__ node, int* __restrict__ first,
                                                                 unsigned long long* __restrict__ stats) {
  unsigned long long trips = 0, breaks = 0;
  for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < E; p += (long long)gridDim.x * blockDim.x) {
    const int sl = slot[p];
    if (sl < 0 || sl >= slots) { trips++; continue; }
    const int c = sl >> 2, s = sl & 3;
    const int j = c / g.w, i = c - j * g.w;
    const bool nd = is_node(g, tail_x(i, s), tail_y(j, s));
    node[p] = nd ? 1 : 0;
    if (!nd) continue;
    breaks++;
    const int s0 = ring[p];
    if (s0 < 0 || s0 >= E) { trips++; continue; }
    atomicMin(&first[s0], rank[p]);
  }
  unsigned long long counts[2] = {trips, breaks};
  add_counts(counts, stats);
}

__global__ __launch_bounds__(OUT_THREADS) void arcs_mark_kernel(IdRaster g, const unsigned char* __restrict__ sides,
                                                                const int* __restrict__ offsets, const int* __restrict__ slot,
                                                                const int* __restrict__ flags, const int* __restrict__ ring,
                                                                const int* __restrict__ rank, const int* __restrict__ totals,
                                                                const int* __restrict__ node, const int* __restrict__ first,
                                                                const int* __restrict__ ring_row, const long long* __restrict__ ring_base,
                                                                long long slots, long long E, long long n_rings, int* __restrict__ left,
                                                                int* __restrict__ twin, int* __restrict__ pos_of, int* __restrict__ order,
                                                                int* __restrict__ hf, int* __restrict__ vf,
                                                                unsigned long long* __restrict__ stats) {
  unsigned long long trips = 0, written = 0, breaks = 0, twins = 0;
  for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < E; p += (long long)gridDim.x * blockDim.x) {
    const int sl = slot[p], s0 = ring[p];
    if (sl < 0 || sl >= slots || s0 < 0 || s0 >= E) { trips++; continue; }
    const int r = ring_row[s0];
    const long long L = totals[2 * (long long)s0];
    if (r < 0 || r >= n_rings || L < 1 || L > E) { trips++; continue; }
    const int raw_first = first[s0], rk = rank[p];
    const long long f = raw_first == SNERF_ARCS_NO_FIRST ? 0 : raw_first;
    const long long base = ring_base[r];
    if (f < 0 || f >= L || rk < 0 || rk >= L || base < 0 || base > E) { trips++; continue; }
    const long long pos = base + (rk - f + L) % L;
    if (pos >= E) { trips++; continue; }
    const int c = sl >> 2, s = sl & 3;
    const int j = c / g.w, i = c - j * g.w;
    const int aj = j + step_j((s + 3) & 3), ai = i + step_i((s + 3) & 3);
    const int lf = g.at(aj, ai);
    int tw = -1;
    if (lf > 0) {                                            // the cell across carries an id: it lies inside the raster
      const long long t = (long long)aj * g.w + ai;
      const int ts = (s + 2) & 3;
      const unsigned sb = sides[t] & 15u;
      const long long tp = (long long)offsets[t] + __popc(sb & ((1u << ts) - 1u));
      if (!((sb >> ts) & 1u) || tp < 0 || tp >= E) trips++;
      else tw = (int)tp;
    }
    const bool brk = node[p] != 0;
    left[p] = lf;
    twin[p] = tw;
    pos_of[p] = (int)pos;
    order[pos] = (int)p;
    hf[pos] = (brk || pos == base) ? 1 : 0;
    vf[pos] = (brk || (flags[p] & SNERF_OUTLINE_CORNER)) ? 1 : 0;
    written++;
    breaks += brk ? 1 : 0;
    twins += tw >= 0 ? 1 : 0;
  }
  unsigned long long counts[4] = {trips, written, breaks, twins};
  add_counts(counts, stats);
}

// What a wave has folded for one arc and not yet added to its row: the same in every lane.
struct ArcFold {
  int arc;                                                   // -1: nothing is held
  unsigned edges, vfs, right, left, ring, twin_first, keyed, open;
  unsigned long long twin_sum, key_right, key_left;
};

__device__ __forceinline__ void flush_fold(const ArcFold& f, unsigned long long* __restrict__ rows) {
  unsigned long long* out = rows + (long long)f.arc * SNERF_ARCS_ROW_WORDS;
  atomicAdd(&out[0], (unsigned long long)f.edges);
  if (f.vfs) atomicAdd(&out[1], (unsigned long long)f.vfs);
  if (f.right) atomicMax(&out[2], (unsigned long long)f.right);
  if (f.left) atomicMax(&out[3], (unsigned long long)f.left);
  if (f.ring) atomicMax(&out[4], (unsigned long long)f.ring);
  if (f.twin_first) atomicMax(&out[5], (unsigned long long)f.twin_first);
  if (f.twin_sum) atomicAdd(&out[6], f.twin_sum);
  if (f.keyed) {
    atomicAdd(&out[7], (unsigned long long)f.keyed);
    atomicAdd(&out[8], f.key_right);
    atomicAdd(&out[9], f.key_left);
  }
  if (f.open) atomicMax(&out[10], (unsigned long long)f.open);
}

// One thread per position: consecutive lanes hold consecutive edges of one ring, so a wave meets few arcs.  A thread places its own
// vertices; the wave then folds arc by arc as outline_emit_kernel folds ring by ring, and HOLDS the result while the next group
// belongs to the same arc, through the trips of the grid-stride too.
__global__ __launch_bounds__(OUT_THREADS) void arcs_fold_kernel(const int* __restrict__ ids, const int* __restrict__ key,
                                                                const int* __restrict__ slot, const int* __restrict__ ring,
                                                                const int* __restrict__ left, const int* __restrict__ twin,
                                                                const int* __restrict__ pos_of, const int* __restrict__ node,
                                                                const int* __restrict__ ring_row, const int* __restrict__ order,
                                                                const int* __restrict__ hf, const int* __restrict__ vf,
                                                                const int* __restrict__ arc_of, const int* __restrict__ ordinal,
                                                                const int* __restrict__ last, const long long* __restrict__ vertex_offset,
                                                                int h, int w, long long slots, long long E, long long A, long long n_rings,
                                                                long long V, int* __restrict__ vertices, unsigned long long* __restrict__ rows,
                                                                unsigned long long* __restrict__ stats) {
  const int lane = threadIdx.x & 63;
  unsigned long long trips = 0, placed = 0;
  ArcFold held = {-1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  // every thread of a workgroup makes the same number of trips: the wave's ballots and shuffles run with all lanes
  for (long long first_pos = (long long)blockIdx.x * blockDim.x; first_pos < E; first_pos += (long long)gridDim.x * blockDim.x) {
    const long long pos = first_pos + threadIdx.x;
    int arc = -1;
    unsigned is_vf = 0, right = 0, lft = 0, ringw = 0, twin_first = 0, keyed = 0, open = 0;
    unsigned long long twin_one = 0, key_right = 0, key_left = 0;
    if (pos < E) {
      const int p = order[pos], a = arc_of[pos];
      const int sl = (p < 0 || p >= E) ? -1 : slot[p];
      if (sl < 0 || sl >= slots || a < 0 || a >= A) {
        trips++;
      } else {
        arc = a;
        const int c = sl >> 2, s = sl & 3;
        const int j = c / w, i = c - j * w;
        const int x0 = tail_x(i, s), y0 = tail_y(j, s);
        const int raw = ids[c], lf = left[p];
        right = raw < 0 ? 0u : (unsigned)raw;
        lft = lf < 0 ? 0u : (unsigned)lf;
        is_vf = vf[pos] != 0 ? 1u : 0u;
        const bool head = hf[pos] != 0, is_last = last[pos] != 0;
        open = (head && node[p] != 0) ? 1u : 0u;
        const int s0 = ring[p];
        if (s0 < 0 || s0 >= E) {
          trips++;
        } else {
          const int r = ring_row[s0];
          if (r < 0 || r >= n_rings) trips++;
          else ringw = (unsigned)r + 1u;
        }
        const int t = twin[p];
        if (t != -1) {
          const int tp = (t < 0 || t >= E) ? -1 : pos_of[t];
          const int ta = (tp < 0 || tp >= E) ? -1 : arc_of[tp];
          if (ta < 0 || ta >= A) trips++;
          else twin_one = 1ull + (unsigned long long)ta;
        }
        twin_first = head ? (unsigned)twin_one : 0u;
        if (key != nullptr) {
          const int aj = j + step_j((s + 3) & 3), ai = i + step_i((s + 3) & 3);
          if (aj >= 0 && aj < h && ai >= 0 && ai < w) {
            const int kr = key[c], kl = key[(long long)aj * w + ai];
            if (roof_valid(kr) && roof_valid(kl)) {
              keyed = 1;
              key_right = (unsigned long long)((long long)kr + 2147483648LL);
              key_left = (unsigned long long)((long long)kl + 2147483648LL);
            }
          }
        }
        if (is_vf || is_last) {
          // the offset is checked before anything is added to it: the terms then fit 33 bits and the sum cannot wrap
          const long long v0 = vertex_offset[a];
          const bool ok = v0 >= 0 && v0 <= V;
          if (is_vf) {
            const long long at = ok ? v0 + ordinal[pos] : -1;
            if (at < 0 || at >= V) {
              trips++;
            } else {
              vertices[2 * at] = x0;
              vertices[2 * at + 1] = y0;
              placed++;
            }
          }
          if (is_last) {
            const long long at = ok ? v0 + ordinal[pos] + (long long)is_vf : -1;
            if (at < 0 || at >= V) {
              trips++;
            } else {
              vertices[2 * at] = x0 + step_i(s);
              vertices[2 * at + 1] = y0 + step_j(s);
              placed++;
            }
          }
        }
      }
    }
    unsigned long long todo = __ballot(arc >= 0);
    while (todo) {                                           // wave-uniform: `todo` is the same word in every lane
      const int leader = __ffsll((long long)todo) - 1;
      const int group = __shfl(arc, leader, 64);
      const bool in = arc == group;                          // (group >= 0: a lane of `todo`)
      todo &= ~__ballot(in);
      ArcFold f;
      f.arc = group;
      f.edges = wave_reduce(in ? 1u : 0u, OpSum());
      f.vfs = wave_reduce(in ? is_vf : 0u, OpSum());
      f.right = wave_reduce(in ? right : 0u, OpMax());
      f.left = wave_reduce(in ? lft : 0u, OpMax());
      f.ring = wave_reduce(in ? ringw : 0u, OpMax());
      f.twin_first = wave_reduce(in ? twin_first : 0u, OpMax());
      f.keyed = wave_reduce(in ? keyed : 0u, OpSum());
      f.open = wave_reduce(in ? open : 0u, OpMax());
      f.twin_sum = wave_reduce(in ? twin_one : 0ull, OpSum());
      f.key_right = wave_reduce(in ? key_right : 0ull, OpSum());
      f.key_left = wave_reduce(in ? key_left : 0ull, OpSum());
      if (held.arc == group) {                               // wave-uniform: both are the same in every lane
        held.edges += f.edges;
        held.vfs += f.vfs;
        held.right = f.right > held.right ? f.right : held.right;
        held.left = f.left > held.left ? f.left : held.left;
        held.ring = f.ring > held.ring ? f.ring : held.ring;
        held.twin_first = f.twin_first > held.twin_first ? f.twin_first : held.twin_first;
        held.keyed += f.keyed;
        held.open = f.open > held.open ? f.open : held.open;
        held.twin_sum += f.twin_sum;
        held.key_right += f.key_right;
        held.key_left += f.key_left;
      } else {
        if (held.arc >= 0 && lane == 0) flush_fold(held, rows);
        held = f;
      }
    }
  }
  if (held.arc >= 0 && lane == 0) flush_fold(held, rows);
  unsigned long long counts[2] = {trips, placed};
  add_counts(counts, stats);
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
static bool arcs_cells_ok(const char* who, int h, int w) {
  if (h < 1 || w < 1) { set_error("%s: h and w must be >= 1 (h = %d, w = %d)", who, h, w); return false; }
  if ((long long)h * w >= SNERF_OUTLINE_MAX_CELLS) { set_error("%s: h * w must be below 2^29 (h = %d, w = %d)", who, h, w); return false; }
  return true;
}

static bool arcs_ids_ok(const char* who, long long K) {
  if (K >= 0 && K < (1LL << 31)) return true;
  set_error("%s: K must lie in [0, 2^31) (K = %lld)", who, K);
  return false;
}

static bool arcs_count_ok(const char* who, const char* what, long long n, int h, int w) {
  if (n >= 0 && n <= 4LL * h * w) return true;
  set_error("%s: %s must lie in [0, 4 h w] (%s = %lld, h = %d, w = %d)", who, what, what, n, h, w);
  return false;
}

// an arc of one edge has two vertices: up to 2 E of them
static bool arcs_vertices_ok(const char* who, long long V, int h, int w) {
  if (V >= 0 && V <= 8LL * h * w) return true;
  set_error("%s: V must lie in [0, 8 h w] (V = %lld, h = %d, w = %d)", who, V, h, w);
  return false;
}

}  // namespace snerf

using namespace snerf;

extern "C" int snerf_roofs_grow(const int* fids, const int* ids, const int* key, const int* facet_root, const double* planes, int h, int w,
                                long long F, double unit, long long max_rq, int rounds, int* a, int* b, unsigned long long* stats,
                                void* stream) {
  const char* who = "snerf_roofs_grow";
  if (!fids || !ids || !key || !a || !b || !stats || (F > 0 && (!facet_root || !planes))) {
    set_error("%s: null pointer", who);
    return SNERF_ERR_NULL;
  }
  if (h < 1 || w < 1) { set_error("%s: h and w must be >= 1 (h = %d, w = %d)", who, h, w); return SNERF_ERR_BAD_DESC; }
  if (h > SNERF_ROOFS_MAX_SIDE || w > SNERF_ROOFS_MAX_SIDE) {
    set_error("%s: h and w must be at most %d (h = %d, w = %d)", who, SNERF_ROOFS_MAX_SIDE, h, w);
    return SNERF_ERR_BAD_DESC;
  }
  if (F < 0 || F >= SNERF_ROOFS_MAX_OBJECTS) { set_error("%s: F must lie in [0, 2^27) (F = %lld)", who, F); return SNERF_ERR_BAD_DESC; }
  if (rounds < 1 || rounds > SNERF_GROW_MAX_ROUNDS) {
    set_error("%s: rounds must lie in [1, %d] (rounds = %d)", who, SNERF_GROW_MAX_ROUNDS, rounds);
    return SNERF_ERR_BAD_DESC;
  }
  if (!(unit > 0.0 && std::isfinite(unit))) { set_error("%s: unit > 0 and finite required (unit = %g)", who, unit); return SNERF_ERR_BAD_DESC; }
  if (max_rq < 0) { set_error("%s: max_rq must not be negative (max_rq = %lld)", who, max_rq); return SNERF_ERR_BAD_DESC; }
  const long long cells = (long long)h * w;
  hipStream_t st = (hipStream_t)stream;
  if (F == 0) {
    SNERF_HIP_CHECK(hipMemcpyAsync((rounds & 1) ? a : b, fids, (size_t)cells * sizeof(int), hipMemcpyDeviceToDevice, st));
    return SNERF_OK;
  }
  const dim3 grid(blocks_for(cells, OUT_THREADS, OUT_COUNT_BLOCKS)), block(OUT_THREADS);
  for (int r = 0; r < rounds; ++r) {
    const int* in = r == 0 ? fids : ((r & 1) ? a : b);
    hipLaunchKernelGGL(roofs_grow_kernel, grid, block, 0, st, in, ids, key, facet_root, planes, h, w, F, unit, max_rq, (r & 1) ? b : a,
                       stats + r, stats + rounds);
  }
  SNERF_LAUNCH_CHECK();
  return SNERF_OK;
}

extern "C" int snerf_arcs_first(const int* ids, const int* slot, const int* ring, const int* rank, int h, int w, long long K, long long E,
                                int* node, int* first, unsigned long long* stats, void* stream) {
  const char* who = "snerf_arcs_first";
  if (!ids || !stats || (E > 0 && (!slot || !ring || !rank || !node || !first))) { set_error("%s: null pointer", who); return SNERF_ERR_NULL; }
  if (!arcs_cells_ok(who, h, w) || !arcs_ids_ok(who, K) || !arcs_count_ok(who, "E", E, h, w)) return SNERF_ERR_BAD_DESC;
  if (E == 0) return SNERF_OK;
  const IdRaster g = {ids, h, w, K};
  hipLaunchKernelGGL(arcs_first_kernel, dim3(blocks_for(E, OUT_THREADS, OUT_COUNT_BLOCKS)), dim3(OUT_THREADS), 0, (hipStream_t)stream, g, slot,
                     ring, rank, 4LL * h * w, E, node, first, stats);
  SNERF_LAUNCH_CHECK();
  return SNERF_OK;
}

extern "C" int snerf_arcs_mark(const int* ids, const unsigned char* sides, const int* offsets, const int* slot, const int* flags,
                               const int* ring, const int* rank, const int* totals, const int* node, const int* first, const int* ring_row,
                               const long long* ring_base, int h, int w, long long K, long long E, long long n_rings, int* left, int* twin,
                               int* pos_of, int* order, int* hf, int* vf, unsigned long long* stats, void* stream) {
  const char* who = "snerf_arcs_mark";
  if (!ids || !sides || !offsets || !stats ||
      (E > 0 && (!slot || !flags || !ring || !rank || !totals || !node || !first || !ring_row || !ring_base || !left || !twin || !pos_of ||
                 !order || !hf || !vf))) {
    set_error("%s: null pointer", who);
    return SNERF_ERR_NULL;
  }
  if (!arcs_cells_ok(who, h, w) || !arcs_ids_ok(who, K)) return SNERF_ERR_BAD_DESC;
  if (!arcs_count_ok(who, "E", E, h, w) || !arcs_count_ok(who, "n_rings", n_rings, h, w)) return SNERF_ERR_BAD_DESC;
  if (E == 0) return SNERF_OK;
  const IdRaster g = {ids, h, w, K};
  hipLaunchKernelGGL(arcs_mark_kernel, dim3(blocks_for(E, OUT_THREADS, OUT_COUNT_BLOCKS)), dim3(OUT_THREADS), 0, (hipStream_t)stream, g, sides,
                     offsets, slot, flags, ring, rank, totals, node, first, ring_row, ring_base, 4LL * h * w, E, n_rings, left, twin, pos_of,
                     order, hf, vf, stats);
  SNERF_LAUNCH_CHECK();
  return SNERF_OK;
}

extern "C" int snerf_arcs_fold(const int* ids, const int* key, const int* slot, const int* ring, const int* left, const int* twin,
                               const int* pos_of, const int* node, const int* ring_row, const int* order, const int* hf, const int* vf,
                               const int* arc_of, const int* ordinal, const int* last, const long long* vertex_offset, int h, int w,
                               long long E, long long A, long long n_rings, long long V, int* vertices, unsigned long long* rows,
                               unsigned long long* stats, void* stream) {
  const char* who = "snerf_arcs_fold";
  if (!ids || !stats ||
      (E > 0 && (!slot || !ring || !left || !twin || !pos_of || !node || !ring_row || !order || !hf || !vf || !arc_of || !ordinal || !last ||
                 !vertex_offset || !vertices || !rows))) {
    set_error("%s: null pointer", who);
    return SNERF_ERR_NULL;
  }
  if (!arcs_cells_ok(who, h, w)) return SNERF_ERR_BAD_DESC;
  if (!arcs_count_ok(who, "E", E, h, w) || !arcs_count_ok(who, "A", A, h, w) || !arcs_count_ok(who, "n_rings", n_rings, h, w) ||
      !arcs_vertices_ok(who, V, h, w))
    return SNERF_ERR_BAD_DESC;
  if (E == 0) return SNERF_OK;
  hipLaunchKernelGGL(arcs_fold_kernel, dim3(blocks_for(E, OUT_THREADS, OUT_COUNT_BLOCKS)), dim3(OUT_THREADS), 0, (hipStream_t)stream, ids, key,
                     slot, ring, left, twin, pos_of, node, ring_row, order, hf, vf, arc_of, ordinal, last, vertex_offset, h, w, 4LL * h * w, E, A,
                     n_rings, V, vertices, rows, stats);
  SNERF_LAUNCH_CHECK();
  return SNERF_OK;
}
