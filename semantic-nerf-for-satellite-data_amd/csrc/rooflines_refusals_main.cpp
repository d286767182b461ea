// The refusal paths of snerf_roofs_grow and the snerf_arcs_* entries (rooflines.hip): see refusals_main.h.
#include "refusals_main.h"
#include "../../include/snerf_rooflines.h"

int main() {
  // never dereferenced as device memory: every call is refused before a launch
  static int ids[48], key[48], fids[48], a[48], b[48], root[4], offsets[48];
  static int slot[192], flags[192], ring[192], rank[192], totals[384], node[192], first[192], ring_row[192], left[192], twin[192], pos_of[192],
      order[192], hf[192], vf[192], arc_of[192], ordinal[192], last[192], vertices[384];
  static unsigned char side_bits[48];
  static double planes[12];
  static long long ring_base[192], vertex_offset[192];
  static unsigned long long stats[65], rows[12 * 192];
  const int h = 6, w = 8;
  what_width = 40;

  g_prefix = "snerf_roofs_grow: ";
  auto grow = [&](const int* f, const int* i, const int* k, const int* r, const double* p, int hh, int ww, long long F, double unit,
                  long long max_rq, int rounds, int* x, int* y, unsigned long long* st) {
    return snerf_roofs_grow(f, i, k, r, p, hh, ww, F, unit, max_rq, rounds, x, y, st, nullptr);
  };
  expect("null fids", grow(nullptr, ids, key, root, planes, h, w, 4, 64.0, 256, 8, a, b, stats), SNERF_ERR_NULL, "null");
  expect("null ids", grow(fids, nullptr, key, root, planes, h, w, 4, 64.0, 256, 8, a, b, stats), SNERF_ERR_NULL, "null");
  expect("null key", grow(fids, ids, nullptr, root, planes, h, w, 4, 64.0, 256, 8, a, b, stats), SNERF_ERR_NULL, "null");
  expect("null facet_root", grow(fids, ids, key, nullptr, planes, h, w, 4, 64.0, 256, 8, a, b, stats), SNERF_ERR_NULL, "null");
  expect("null planes", grow(fids, ids, key, root, nullptr, h, w, 4, 64.0, 256, 8, a, b, stats), SNERF_ERR_NULL, "null");
  expect("null a", grow(fids, ids, key, root, planes, h, w, 4, 64.0, 256, 8, nullptr, b, stats), SNERF_ERR_NULL, "null");
  expect("null b", grow(fids, ids, key, root, planes, h, w, 4, 64.0, 256, 8, a, nullptr, stats), SNERF_ERR_NULL, "null");
  expect("null stats", grow(fids, ids, key, root, planes, h, w, 4, 64.0, 256, 8, a, b, nullptr), SNERF_ERR_NULL, "null");
  expect("h = 0", grow(fids, ids, key, root, planes, 0, w, 4, 64.0, 256, 8, a, b, stats), SNERF_ERR_BAD_DESC, ">= 1");
  expect("w = -1", grow(fids, ids, key, root, planes, h, -1, 4, 64.0, 256, 8, a, b, stats), SNERF_ERR_BAD_DESC, ">= 1");
  expect("h = 8193", grow(fids, ids, key, root, planes, 8193, w, 4, 64.0, 256, 8, a, b, stats), SNERF_ERR_BAD_DESC, "at most 8192");
  expect("F = -1", grow(fids, ids, key, root, planes, h, w, -1, 64.0, 256, 8, a, b, stats), SNERF_ERR_BAD_DESC, "F = -1");
  expect("F = 2^27", grow(fids, ids, key, root, planes, h, w, 134217728LL, 64.0, 256, 8, a, b, stats), SNERF_ERR_BAD_DESC, "[0, 2^27)");
  expect("rounds = 0", grow(fids, ids, key, root, planes, h, w, 4, 64.0, 256, 0, a, b, stats), SNERF_ERR_BAD_DESC, "rounds = 0");
  expect("rounds = 65", grow(fids, ids, key, root, planes, h, w, 4, 64.0, 256, 65, a, b, stats), SNERF_ERR_BAD_DESC, "rounds = 65");
  expect("unit = 0", grow(fids, ids, key, root, planes, h, w, 4, 0.0, 256, 8, a, b, stats), SNERF_ERR_BAD_DESC, "unit > 0");
  expect("unit = inf", grow(fids, ids, key, root, planes, h, w, 4, INFINITY, 256, 8, a, b, stats), SNERF_ERR_BAD_DESC, "unit > 0");
  expect("unit = nan", grow(fids, ids, key, root, planes, h, w, 4, NAN, 256, 8, a, b, stats), SNERF_ERR_BAD_DESC, "unit > 0");
  expect("max_rq = -1", grow(fids, ids, key, root, planes, h, w, 4, 64.0, -1, 8, a, b, stats), SNERF_ERR_BAD_DESC, "max_rq = -1");

  g_prefix = "snerf_arcs_first: ";
  auto fst = [&](const int* i, const int* sl, const int* rg, const int* rk, int hh, int ww, long long K, long long E, int* nd, int* fi,
                 unsigned long long* st) { return snerf_arcs_first(i, sl, rg, rk, hh, ww, K, E, nd, fi, st, nullptr); };
  expect("null ids", fst(nullptr, slot, ring, rank, h, w, 3, 10, node, first, stats), SNERF_ERR_NULL, "null");
  expect("null slot", fst(ids, nullptr, ring, rank, h, w, 3, 10, node, first, stats), SNERF_ERR_NULL, "null");
  expect("null ring", fst(ids, slot, nullptr, rank, h, w, 3, 10, node, first, stats), SNERF_ERR_NULL, "null");
  expect("null rank", fst(ids, slot, ring, nullptr, h, w, 3, 10, node, first, stats), SNERF_ERR_NULL, "null");
  expect("null node", fst(ids, slot, ring, rank, h, w, 3, 10, nullptr, first, stats), SNERF_ERR_NULL, "null");
  expect("null first", fst(ids, slot, ring, rank, h, w, 3, 10, node, nullptr, stats), SNERF_ERR_NULL, "null");
  expect("null stats", fst(ids, slot, ring, rank, h, w, 3, 10, node, first, nullptr), SNERF_ERR_NULL, "null");
  expect("h = 0", fst(ids, slot, ring, rank, 0, w, 3, 10, node, first, stats), SNERF_ERR_BAD_DESC, ">= 1");
  expect("h * w = 2^29", fst(ids, slot, ring, rank, 16384, 32768, 3, 10, node, first, stats), SNERF_ERR_BAD_DESC, "below 2^29");
  expect("K = -1", fst(ids, slot, ring, rank, h, w, -1, 10, node, first, stats), SNERF_ERR_BAD_DESC, "K = -1");
  expect("K = 2^31", fst(ids, slot, ring, rank, h, w, 2147483648LL, 10, node, first, stats), SNERF_ERR_BAD_DESC, "K = 2147483648");
  expect("E = -1", fst(ids, slot, ring, rank, h, w, 3, -1, node, first, stats), SNERF_ERR_BAD_DESC, "E = -1");
  expect("E = 4 h w + 1", fst(ids, slot, ring, rank, h, w, 3, 193, node, first, stats), SNERF_ERR_BAD_DESC, "E = 193");
  g_prefix = nullptr;
  expect("E = 0: nothing to do, null buffers", fst(ids, nullptr, nullptr, nullptr, h, w, 3, 0, nullptr, nullptr, stats), SNERF_OK, nullptr);

  g_prefix = "snerf_arcs_mark: ";
  auto mark = [&](const int* i, const unsigned char* sb, const int* of, const int* sl, int hh, int ww, long long K, long long E, long long R,
                  int* lf, unsigned long long* st) {
    return snerf_arcs_mark(i, sb, of, sl, flags, ring, rank, totals, node, first, ring_row, ring_base, hh, ww, K, E, R, lf, twin, pos_of, order,
                           hf, vf, st, nullptr);
  };
  expect("null ids", mark(nullptr, side_bits, offsets, slot, h, w, 3, 10, 2, left, stats), SNERF_ERR_NULL, "null");
  expect("null sides", mark(ids, nullptr, offsets, slot, h, w, 3, 10, 2, left, stats), SNERF_ERR_NULL, "null");
  expect("null offsets", mark(ids, side_bits, nullptr, slot, h, w, 3, 10, 2, left, stats), SNERF_ERR_NULL, "null");
  expect("null slot", mark(ids, side_bits, offsets, nullptr, h, w, 3, 10, 2, left, stats), SNERF_ERR_NULL, "null");
  expect("null left", mark(ids, side_bits, offsets, slot, h, w, 3, 10, 2, nullptr, stats), SNERF_ERR_NULL, "null");
  expect("null stats", mark(ids, side_bits, offsets, slot, h, w, 3, 10, 2, left, nullptr), SNERF_ERR_NULL, "null");
  expect("w = 0", mark(ids, side_bits, offsets, slot, h, 0, 3, 10, 2, left, stats), SNERF_ERR_BAD_DESC, ">= 1");
  expect("h * w = 2^29", mark(ids, side_bits, offsets, slot, 32768, 16384, 3, 10, 2, left, stats), SNERF_ERR_BAD_DESC, "below 2^29");
  expect("K = -2", mark(ids, side_bits, offsets, slot, h, w, -2, 10, 2, left, stats), SNERF_ERR_BAD_DESC, "K = -2");
  expect("E = 193", mark(ids, side_bits, offsets, slot, h, w, 3, 193, 2, left, stats), SNERF_ERR_BAD_DESC, "E = 193");
  expect("n_rings = -1", mark(ids, side_bits, offsets, slot, h, w, 3, 10, -1, left, stats), SNERF_ERR_BAD_DESC, "n_rings = -1");
  g_prefix = nullptr;
  expect("E = 0: nothing to do, null buffers",
         snerf_arcs_mark(ids, side_bits, offsets, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, h, w, 3, 0, 0,
                         nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, stats, nullptr),
         SNERF_OK, nullptr);

  g_prefix = "snerf_arcs_fold: ";
  auto fold = [&](const int* i, const int* k, const int* sl, const long long* vo, int hh, int ww, long long E, long long A, long long R,
                  long long V, int* vx, unsigned long long* ro, unsigned long long* st) {
    return snerf_arcs_fold(i, k, sl, ring, left, twin, pos_of, node, ring_row, order, hf, vf, arc_of, ordinal, last, vo, hh, ww, E, A, R, V, vx,
                           ro, st, nullptr);
  };
  expect("null ids", fold(nullptr, key, slot, vertex_offset, h, w, 10, 3, 2, 8, vertices, rows, stats), SNERF_ERR_NULL, "null");
  expect("null slot", fold(ids, key, nullptr, vertex_offset, h, w, 10, 3, 2, 8, vertices, rows, stats), SNERF_ERR_NULL, "null");
  expect("null vertex_offset", fold(ids, key, slot, nullptr, h, w, 10, 3, 2, 8, vertices, rows, stats), SNERF_ERR_NULL, "null");
  expect("null vertices", fold(ids, key, slot, vertex_offset, h, w, 10, 3, 2, 8, nullptr, rows, stats), SNERF_ERR_NULL, "null");
  expect("null rows", fold(ids, key, slot, vertex_offset, h, w, 10, 3, 2, 8, vertices, nullptr, stats), SNERF_ERR_NULL, "null");
  expect("null stats", fold(ids, key, slot, vertex_offset, h, w, 10, 3, 2, 8, vertices, rows, nullptr), SNERF_ERR_NULL, "null");
  expect("h = 0", fold(ids, key, slot, vertex_offset, 0, w, 10, 3, 2, 8, vertices, rows, stats), SNERF_ERR_BAD_DESC, ">= 1");
  expect("h * w = 2^29", fold(ids, key, slot, vertex_offset, 16384, 32768, 10, 3, 2, 8, vertices, rows, stats), SNERF_ERR_BAD_DESC, "below 2^29");
  expect("E = -1", fold(ids, key, slot, vertex_offset, h, w, -1, 3, 2, 8, vertices, rows, stats), SNERF_ERR_BAD_DESC, "E = -1");
  expect("A = 193", fold(ids, key, slot, vertex_offset, h, w, 10, 193, 2, 8, vertices, rows, stats), SNERF_ERR_BAD_DESC, "A = 193");
  expect("n_rings = -1", fold(ids, key, slot, vertex_offset, h, w, 10, 3, -1, 8, vertices, rows, stats), SNERF_ERR_BAD_DESC, "n_rings = -1");
  expect("V = -1", fold(ids, key, slot, vertex_offset, h, w, 10, 3, 2, -1, vertices, rows, stats), SNERF_ERR_BAD_DESC, "V = -1");
  expect("V = 8 h w + 1", fold(ids, key, slot, vertex_offset, h, w, 10, 3, 2, 385, vertices, rows, stats), SNERF_ERR_BAD_DESC, "V = 385");
  g_prefix = nullptr;
  expect("E = 0: nothing to do, null buffers, no key",
         snerf_arcs_fold(ids, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                         nullptr, nullptr, h, w, 0, 0, 0, 0, nullptr, nullptr, stats, nullptr),
         SNERF_OK, nullptr);

  bool written = false;
  for (int k = 0; k < 65; ++k) written = written || stats[k];
  for (int k = 0; k < 192; ++k)
    written = written || node[k] || first[k] || left[k] || twin[k] || pos_of[k] || order[k] || hf[k] || vf[k] || vertices[k] || rows[k];
  for (int k = 0; k < 48; ++k) written = written || a[k] || b[k];
  if (written) {
    printf("outputs were written\n");
    ++failures;
  }
  return verdict("rooflines");
}
