// Objects on the map: the connected components of a class raster (init, merge, flatten over a lock-free union-find) and per-object
// reductions in one launch (a reduction inside the wave over the lanes that share an object, then one lane's integer atomics).  The
// spec is include/snerf_objects.h and DESIGN.md section 5x; the walk is csrc/objects_walk.h, which csrc/objects_walk_main.cpp runs
// on the host under ThreadSanitizer.  Integer atomics only: every word is independent of the order in which cells arrive.
#include "lattice.h"
#include "link_kernels.h"
#include "reduce.h"
#include "../../include/snerf_objects.h"

#pragma clang fp contract(off)

namespace snerf {

constexpr int OBJ_THREADS = 256;
constexpr unsigned OBJ_MAX_BLOCKS = 65536;               // cells beyond it are taken in a grid-stride

// a class table by value: bit c of the 256
struct ObjClasses {
  unsigned long long bits[4];
};
__device__ __forceinline__ bool in_classes(const ObjClasses& t, unsigned c) {
  const unsigned long long lo = c & 64 ? t.bits[1] : t.bits[0], hi = c & 64 ? t.bits[3] : t.bits[2];
  return (((c & 128 ? hi : lo) >> (c & 63)) & 1ull) != 0;
}

// what links two cells of a class raster (csrc/link_kernels.h: init, merge, flatten): the same class, one of `member_set`
struct ClassLink {
  const unsigned char* label;
  ObjClasses member_set;
  __device__ __forceinline__ int load(long long c) const { return label[c]; }
  __device__ __forceinline__ bool member(int l) const { return in_classes(member_set, (unsigned)l); }
};

// ---- stats -------------------------------------------------------------------------------------------------------------------------
// rint((alt - z0) / q) as lattice_key quantises; false when it is not in [-2^31, 2^31)
__device__ __forceinline__ bool quantise(float alt, double z0, double q, long long* k) {
  const double kq = rint(((double)alt - z0) / q);
  if (!(kq >= -2147483648.0 && kq < 2147483648.0)) return false;
  *k = (long long)kq;
  return true;
}

// One thread per cell of the band.  A thread folds its own cell and its own ring window; the wave then takes the first lane that
// still has an object, ballots the lanes of that object, reduces their values across the wave (the others hold the identities) and
// lets that lane issue the row's atomics; the sums are integers, so the grouping does not show in the words.
__global__ __launch_bounds__(OBJ_THREADS) void objects_stats_kernel(const int* __restrict__ ids, const unsigned char* __restrict__ label,
                                                                    const float* __restrict__ alt, int h, int w, long long K,
                                                                    ObjClasses ground, int ring, double z0, double q, long long first,
                                                                    long long end, unsigned long long* __restrict__ rows,
                                                                    unsigned long long* __restrict__ stats) {
  const int lane = threadIdx.x & 63;
  unsigned long long out_of_range = 0, holes = 0, bad_ids = 0, pairs_all = 0;
  // every thread of a workgroup makes the same number of trips: the wave's ballots and shuffles run with all lanes
  for (long long base = first + (long long)blockIdx.x * blockDim.x; base < end; base += (long long)gridDim.x * blockDim.x) {
    const long long c = base + threadIdx.x;
    int id = 0;
    if (c < end) {
      id = ids[c];
      if (id < 0 || id > K) { bad_ids++; id = 0; }
    }
    unsigned area = 0, valid = 0, pairs = 0, perim = 0, cls = 0;
    unsigned min_i = 0xFFFFFFFFu, max_i = 0, min_j = 0xFFFFFFFFu, max_j = 0, min_k = 0xFFFFFFFFu, max_k = 0, min_g = 0xFFFFFFFFu;
    unsigned long long sum_i = 0, sum_j = 0;
    long long sum_k = 0, sum_g = 0;
    if (id > 0) {
      const int j = (int)(c / w), i = (int)(c - (long long)j * w);
      area = 1;
      sum_i = min_i = max_i = (unsigned)i;
      sum_j = min_j = max_j = (unsigned)j;
      cls = label[c];
      const float a = alt[c];
      long long k;
      if (quantise(a, z0, q, &k)) {
        valid = 1;
        sum_k = k;
        min_k = max_k = (unsigned)(k + 2147483648LL);
      } else if (isfinite(a)) {
        out_of_range++;
      } else {
        holes++;
      }
      perim += (i == 0 || ids[c - 1] != id) ? 1 : 0;
      perim += (i + 1 == w || ids[c + 1] != id) ? 1 : 0;
      perim += (j == 0 || ids[c - w] != id) ? 1 : 0;
      perim += (j + 1 == h || ids[c + w] != id) ? 1 : 0;
      if (ring > 0) {
        const int i0 = i - ring > 0 ? i - ring : 0, i1 = i + ring + 1 < w ? i + ring + 1 : w;
        const int j0 = j - ring > 0 ? j - ring : 0, j1 = j + ring + 1 < h ? j + ring + 1 : h;
        for (int gj = j0; gj < j1; ++gj)
          for (int gi = i0; gi < i1; ++gi) {
            const long long g = (long long)gj * w + gi;
            if (ids[g] != 0 || !in_classes(ground, label[g])) continue;
            long long kg;
            if (!quantise(alt[g], z0, q, &kg)) continue;
            pairs++;
            sum_g += kg;
            const unsigned biased = (unsigned)(kg + 2147483648LL);
            min_g = biased < min_g ? biased : min_g;
          }
        pairs_all += pairs;
      }
    }
    unsigned long long todo = __ballot(id > 0);
    while (todo) {                                           // wave-uniform: `todo` is the same word in every lane
      const int leader = __ffsll((long long)todo) - 1;
      const int group_id = __shfl(id, leader, 64);
      const bool in = id == group_id;                        // (group_id > 0: a lane of `todo`)
      todo &= ~__ballot(in);
      const unsigned r_area = wave_reduce(in ? area : 0u, OpSum());
      const unsigned long long r_sum_i = wave_reduce(in ? sum_i : 0ull, OpSum()), r_sum_j = wave_reduce(in ? sum_j : 0ull, OpSum());
      const unsigned r_min_i = wave_reduce(in ? min_i : 0xFFFFFFFFu, OpMin()), r_max_i = wave_reduce(in ? max_i : 0u, OpMax());
      const unsigned r_min_j = wave_reduce(in ? min_j : 0xFFFFFFFFu, OpMin()), r_max_j = wave_reduce(in ? max_j : 0u, OpMax());
      const unsigned r_valid = wave_reduce(in ? valid : 0u, OpSum());
      const long long r_sum_k = wave_reduce(in ? sum_k : 0ll, OpSum());
      const unsigned r_min_k = wave_reduce(in ? min_k : 0xFFFFFFFFu, OpMin()), r_max_k = wave_reduce(in ? max_k : 0u, OpMax());
      const unsigned r_pairs = wave_reduce(in ? pairs : 0u, OpSum());
      const long long r_sum_g = wave_reduce(in ? sum_g : 0ll, OpSum());
      const unsigned r_min_g = wave_reduce(in ? min_g : 0xFFFFFFFFu, OpMin());
      const unsigned r_perim = wave_reduce(in ? perim : 0u, OpSum());
      const unsigned r_cls = wave_reduce(in ? cls : 0u, OpMax());
      if (lane == leader) {
        unsigned long long* row = rows + (long long)(group_id - 1) * SNERF_OBJECTS_ROW_WORDS;
        atomicAdd(&row[0], (unsigned long long)r_area);
        atomicAdd(&row[1], r_sum_i);
        atomicAdd(&row[2], r_sum_j);
        atomicMin(&row[3], (unsigned long long)r_min_i);
        atomicMax(&row[4], (unsigned long long)r_max_i);
        atomicMin(&row[5], (unsigned long long)r_min_j);
        atomicMax(&row[6], (unsigned long long)r_max_j);
        if (r_valid) {
          atomicAdd(&row[7], (unsigned long long)r_valid);
          atomicAdd(&row[8], (unsigned long long)r_sum_k);
          atomicMin(&row[9], (unsigned long long)r_min_k);
          atomicMax(&row[10], (unsigned long long)r_max_k);
        }
        if (r_pairs) {
          atomicAdd(&row[11], (unsigned long long)r_pairs);
          atomicAdd(&row[12], (unsigned long long)r_sum_g);
          atomicMin(&row[13], (unsigned long long)r_min_g);
        }
        if (r_perim) atomicAdd(&row[14], (unsigned long long)r_perim);
        atomicMax(&row[15], (unsigned long long)r_cls);
      }
    }
  }
  out_of_range = wave_reduce(out_of_range, OpSum());
  holes = wave_reduce(holes, OpSum());
  bad_ids = wave_reduce(bad_ids, OpSum());
  pairs_all = wave_reduce(pairs_all, OpSum());
  if (lane == 0) {
    if (out_of_range) atomicAdd(&stats[0], out_of_range);
    if (holes) atomicAdd(&stats[1], holes);
    if (bad_ids) atomicAdd(&stats[2], bad_ids);
    if (pairs_all) atomicAdd(&stats[3], pairs_all);
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
static bool objects_table(const char* who, const char* what, const unsigned char* table_host, ObjClasses* out) {
  if (table_host[255]) { set_error("%s: %s[255] is set: class 255 means no label and is in no set", who, what); return false; }
  ObjClasses t = {{0, 0, 0, 0}};
  for (int c = 0; c < 256; ++c)
    if (table_host[c]) t.bits[c >> 6] |= 1ull << (c & 63);
  *out = t;
  return true;
}

}  // namespace snerf

using namespace snerf;

extern "C" int snerf_objects_link(const unsigned char* label, int h, int w, const unsigned char* member_host, int connectivity,
                                  int* parent, unsigned long long* stats, void* stream) {
  const char* who = "snerf_objects_link";
  if (!label || !member_host || !parent || !stats) { set_error("%s: null pointer", who); return SNERF_ERR_NULL; }
  if (!lattice_cells_ok(who, h, w)) return SNERF_ERR_BAD_DESC;
  if (connectivity != 4 && connectivity != 8) {
    set_error("%s: connectivity must be 4 or 8 (connectivity = %d)", who, connectivity);
    return SNERF_ERR_BAD_DESC;
  }
  ObjClasses member;
  if (!objects_table(who, "member_host", member_host, &member)) return SNERF_ERR_BAD_DESC;
  const ClassLink pred = {label, member};
  return link_launch(pred, h, w, connectivity, parent, stats, stream);
}

extern "C" int snerf_objects_stats(const int* ids, const unsigned char* label, const float* alt, int h, int w, long long K,
                                   const unsigned char* ground_host, int ring, double z0, double q, int row0, int row1,
                                   unsigned long long* rows, unsigned long long* stats, void* stream) {
  const char* who = "snerf_objects_stats";
  if (!ids || !label || !alt || !ground_host || !stats || (K > 0 && !rows)) { set_error("%s: null pointer", who); return SNERF_ERR_NULL; }
  if (!lattice_cells_ok(who, h, w)) return SNERF_ERR_BAD_DESC;
  if (K < 0 || K >= LATTICE_MAX_CELLS) { set_error("%s: K must lie in [0, 2^31) (K = %lld)", who, K); return SNERF_ERR_BAD_DESC; }
  if (ring < 0 || ring > SNERF_ORTHO_MAX_RADIUS) {
    set_error("%s: ring must lie in [0, %d] (ring = %d)", who, SNERF_ORTHO_MAX_RADIUS, ring);
    return SNERF_ERR_BAD_DESC;
  }
  const long long side = 2 * ring + 1;
  if ((long long)h * w * side * side >= 4294967296LL) {
    set_error("%s: h * w * (2 ring + 1)^2 must be below 2^32 (h = %d, w = %d, ring = %d)", who, h, w, ring);
    return SNERF_ERR_BAD_DESC;
  }
  if (row0 < 0 || row1 > h || row0 > row1) {
    set_error("%s: 0 <= row0 <= row1 <= h required (row0 = %d, row1 = %d, h = %d)", who, row0, row1, h);
    return SNERF_ERR_BAD_DESC;
  }
  if (!quant_ok(who, z0, q)) return SNERF_ERR_BAD_DESC;
  ObjClasses ground;
  if (!objects_table(who, "ground_host", ground_host, &ground)) return SNERF_ERR_BAD_DESC;
  if (K == 0 || row0 == row1) return SNERF_OK;
  const long long first = (long long)row0 * w, end = (long long)row1 * w;
  hipLaunchKernelGGL(objects_stats_kernel, dim3(blocks_for(end - first, OBJ_THREADS, OBJ_MAX_BLOCKS)), dim3(OBJ_THREADS), 0,
                     (hipStream_t)stream, ids, label, alt, h, w, K, ground, ring, z0, q, first, end, rows, stats);
  SNERF_LAUNCH_CHECK();
  return SNERF_OK;
}
