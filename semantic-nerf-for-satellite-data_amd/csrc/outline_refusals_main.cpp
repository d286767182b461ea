// The refusal paths of the snerf_outline_* entries (outline.hip): see refusals_main.h.
#include "refusals_main.h"
#include "../../include/snerf_outline.h"

int main() {
  // never dereferenced as device memory: every call is refused before a launch
  static int ids[48], offsets[48], slot[192], next[192], flags[192], ring[192], rank[192], ordinal[192], totals[384], ring_row[192], vertices[384];
  static unsigned char side_bits[48];
  static long long vertex_offset[192];
  static unsigned long long stats[4], rows[8 * 192];
  static int workspace[6 * 192];
  const int h = 6, w = 8;
  what_width = 40;

  g_prefix = "snerf_outline_sides: ";
  auto sides = [&](const int* i, int hh, int ww, long long K, unsigned char* s, unsigned long long* st) {
    return snerf_outline_sides(i, hh, ww, K, s, st, nullptr);
  };
  expect("null ids", sides(nullptr, h, w, 3, side_bits, stats), SNERF_ERR_NULL, "null");
  expect("null sides", sides(ids, h, w, 3, nullptr, stats), SNERF_ERR_NULL, "null");
  expect("null stats", sides(ids, h, w, 3, side_bits, nullptr), SNERF_ERR_NULL, "null");
  expect("h = 0", sides(ids, 0, w, 3, side_bits, stats), SNERF_ERR_BAD_DESC, ">= 1");
  expect("w = -1", sides(ids, h, -1, 3, side_bits, stats), SNERF_ERR_BAD_DESC, ">= 1");
  expect("h * w = 2^29", sides(ids, 16384, 32768, 3, side_bits, stats), SNERF_ERR_BAD_DESC, "below 2^29");
  expect("h * w = 2^62", sides(ids, 2147483647, 2147483647, 3, side_bits, stats), SNERF_ERR_BAD_DESC, "below 2^29");
  expect("K = -1", sides(ids, h, w, -1, side_bits, stats), SNERF_ERR_BAD_DESC, "K = -1");
  expect("K = 2^31", sides(ids, h, w, 2147483648LL, side_bits, stats), SNERF_ERR_BAD_DESC, "K = 2147483648");

  g_prefix = "snerf_outline_link: ";
  auto link = [&](const int* i, const unsigned char* s, const int* o, int hh, int ww, long long K, int conn, long long E, int* sl, int* nx,
                  int* fl, unsigned long long* st) { return snerf_outline_link(i, s, o, hh, ww, K, conn, E, sl, nx, fl, st, nullptr); };
  expect("null ids", link(nullptr, side_bits, offsets, h, w, 3, 4, 10, slot, next, flags, stats), SNERF_ERR_NULL, "null");
  expect("null sides", link(ids, nullptr, offsets, h, w, 3, 4, 10, slot, next, flags, stats), SNERF_ERR_NULL, "null");
  expect("null offsets", link(ids, side_bits, nullptr, h, w, 3, 4, 10, slot, next, flags, stats), SNERF_ERR_NULL, "null");
  expect("null slot", link(ids, side_bits, offsets, h, w, 3, 4, 10, nullptr, next, flags, stats), SNERF_ERR_NULL, "null");
  expect("null next", link(ids, side_bits, offsets, h, w, 3, 4, 10, slot, nullptr, flags, stats), SNERF_ERR_NULL, "null");
  expect("null flags", link(ids, side_bits, offsets, h, w, 3, 4, 10, slot, next, nullptr, stats), SNERF_ERR_NULL, "null");
  expect("null stats", link(ids, side_bits, offsets, h, w, 3, 4, 10, slot, next, flags, nullptr), SNERF_ERR_NULL, "null");
  expect("h = 0", link(ids, side_bits, offsets, 0, w, 3, 4, 10, slot, next, flags, stats), SNERF_ERR_BAD_DESC, ">= 1");
  expect("h * w = 2^29", link(ids, side_bits, offsets, 32768, 16384, 3, 4, 10, slot, next, flags, stats), SNERF_ERR_BAD_DESC, "below 2^29");
  expect("K = -2", link(ids, side_bits, offsets, h, w, -2, 4, 10, slot, next, flags, stats), SNERF_ERR_BAD_DESC, "K = -2");
  expect("connectivity = 6", link(ids, side_bits, offsets, h, w, 3, 6, 10, slot, next, flags, stats), SNERF_ERR_BAD_DESC, "connectivity = 6");
  expect("E = -1", link(ids, side_bits, offsets, h, w, 3, 4, -1, slot, next, flags, stats), SNERF_ERR_BAD_DESC, "E = -1");
  expect("E = 4 h w + 1", link(ids, side_bits, offsets, h, w, 3, 4, 193, slot, next, flags, stats), SNERF_ERR_BAD_DESC, "E = 193");
  g_prefix = nullptr;
  expect("E = 0: nothing to do, null outputs", link(ids, side_bits, offsets, h, w, 3, 8, 0, nullptr, nullptr, nullptr, stats), SNERF_OK, nullptr);

  g_prefix = "snerf_outline_workspace_bytes: ";
  expect("E = -1", (int)snerf_outline_workspace_bytes(-1), -1, "E = -1");
  expect("E = 2^31", (int)snerf_outline_workspace_bytes(2147483648LL), -1, "E = 2147483648");
  g_prefix = nullptr;
  expect("E = 0", (int)snerf_outline_workspace_bytes(0), 0, nullptr);
  expect("E = 192", (int)snerf_outline_workspace_bytes(192), 24 * 192, nullptr);
  expect("E = 2^31 - 1", snerf_outline_workspace_bytes(2147483647LL) == 24 * 2147483647LL ? 0 : 1, 0, nullptr);

  g_prefix = "snerf_outline_rank: ";
  auto rk = [&](const int* nx, const int* fl, long long E, int* rg, int* ra, int* od, int* to, void* ws, long long bytes,
                unsigned long long* st) { return snerf_outline_rank(nx, fl, E, rg, ra, od, to, ws, bytes, st, nullptr); };
  const long long bytes = sizeof workspace;
  expect("null next", rk(nullptr, flags, 192, ring, rank, ordinal, totals, workspace, bytes, stats), SNERF_ERR_NULL, "null");
  expect("null flags", rk(next, nullptr, 192, ring, rank, ordinal, totals, workspace, bytes, stats), SNERF_ERR_NULL, "null");
  expect("null ring", rk(next, flags, 192, nullptr, rank, ordinal, totals, workspace, bytes, stats), SNERF_ERR_NULL, "null");
  expect("null rank", rk(next, flags, 192, ring, nullptr, ordinal, totals, workspace, bytes, stats), SNERF_ERR_NULL, "null");
  expect("null ordinal", rk(next, flags, 192, ring, rank, nullptr, totals, workspace, bytes, stats), SNERF_ERR_NULL, "null");
  expect("null totals", rk(next, flags, 192, ring, rank, ordinal, nullptr, workspace, bytes, stats), SNERF_ERR_NULL, "null");
  expect("null workspace", rk(next, flags, 192, ring, rank, ordinal, totals, nullptr, bytes, stats), SNERF_ERR_NULL, "null");
  expect("null stats", rk(next, flags, 192, ring, rank, ordinal, totals, workspace, bytes, nullptr), SNERF_ERR_NULL, "null");
  expect("E = -1", rk(next, flags, -1, ring, rank, ordinal, totals, workspace, bytes, stats), SNERF_ERR_BAD_DESC, "E = -1");
  expect("E = 2^31", rk(next, flags, 2147483648LL, ring, rank, ordinal, totals, workspace, bytes, stats), SNERF_ERR_BAD_DESC, "E = 2147483648");
  expect("a workspace off by one byte", rk(next, flags, 191, ring, rank, ordinal, totals, (char*)workspace + 1, bytes - 1, stats), SNERF_ERR_BAD_DESC,
         "4-byte aligned");
  expect("a workspace one byte short", rk(next, flags, 192, ring, rank, ordinal, totals, workspace, bytes - 1, stats), SNERF_ERR_BAD_DESC,
         "4608 are needed");
  g_prefix = nullptr;
  expect("E = 0: nothing to do, null buffers", rk(nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 0, stats), SNERF_OK, nullptr);

  g_prefix = "snerf_outline_emit: ";
  auto emit = [&](const int* i, const int* sl, const int* fl, const int* rg, const int* od, const int* rr, const long long* vo, int hh, int ww,
                  long long E, long long R, long long V, int* vx, unsigned long long* ro, unsigned long long* st) {
    return snerf_outline_emit(i, sl, fl, rg, od, rr, vo, hh, ww, E, R, V, vx, ro, st, nullptr);
  };
  expect("null ids", emit(nullptr, slot, flags, ring, ordinal, ring_row, vertex_offset, h, w, 10, 2, 8, vertices, rows, stats), SNERF_ERR_NULL, "null");
  expect("null slot", emit(ids, nullptr, flags, ring, ordinal, ring_row, vertex_offset, h, w, 10, 2, 8, vertices, rows, stats), SNERF_ERR_NULL, "null");
  expect("null flags", emit(ids, slot, nullptr, ring, ordinal, ring_row, vertex_offset, h, w, 10, 2, 8, vertices, rows, stats), SNERF_ERR_NULL, "null");
  expect("null ring", emit(ids, slot, flags, nullptr, ordinal, ring_row, vertex_offset, h, w, 10, 2, 8, vertices, rows, stats), SNERF_ERR_NULL, "null");
  expect("null ordinal", emit(ids, slot, flags, ring, nullptr, ring_row, vertex_offset, h, w, 10, 2, 8, vertices, rows, stats), SNERF_ERR_NULL, "null");
  expect("null ring_row", emit(ids, slot, flags, ring, ordinal, nullptr, vertex_offset, h, w, 10, 2, 8, vertices, rows, stats), SNERF_ERR_NULL, "null");
  expect("null vertex_offset", emit(ids, slot, flags, ring, ordinal, ring_row, nullptr, h, w, 10, 2, 8, vertices, rows, stats), SNERF_ERR_NULL, "null");
  expect("null vertices", emit(ids, slot, flags, ring, ordinal, ring_row, vertex_offset, h, w, 10, 2, 8, nullptr, rows, stats), SNERF_ERR_NULL, "null");
  expect("null rows", emit(ids, slot, flags, ring, ordinal, ring_row, vertex_offset, h, w, 10, 2, 8, vertices, nullptr, stats), SNERF_ERR_NULL, "null");
  expect("null stats", emit(ids, slot, flags, ring, ordinal, ring_row, vertex_offset, h, w, 10, 2, 8, vertices, rows, nullptr), SNERF_ERR_NULL, "null");
  expect("w = 0", emit(ids, slot, flags, ring, ordinal, ring_row, vertex_offset, h, 0, 10, 2, 8, vertices, rows, stats), SNERF_ERR_BAD_DESC, ">= 1");
  expect("h * w = 2^29", emit(ids, slot, flags, ring, ordinal, ring_row, vertex_offset, 16384, 32768, 10, 2, 8, vertices, rows, stats),
         SNERF_ERR_BAD_DESC, "below 2^29");
  expect("E = -1", emit(ids, slot, flags, ring, ordinal, ring_row, vertex_offset, h, w, -1, 2, 8, vertices, rows, stats), SNERF_ERR_BAD_DESC, "E = -1");
  expect("E = 4 h w + 1", emit(ids, slot, flags, ring, ordinal, ring_row, vertex_offset, h, w, 193, 2, 8, vertices, rows, stats), SNERF_ERR_BAD_DESC,
         "E = 193");
  expect("n_rings = -1", emit(ids, slot, flags, ring, ordinal, ring_row, vertex_offset, h, w, 10, -1, 8, vertices, rows, stats), SNERF_ERR_BAD_DESC,
         "n_rings = -1");
  expect("n_rings = 4 h w + 1", emit(ids, slot, flags, ring, ordinal, ring_row, vertex_offset, h, w, 10, 193, 8, vertices, rows, stats),
         SNERF_ERR_BAD_DESC, "n_rings = 193");
  expect("V = -1", emit(ids, slot, flags, ring, ordinal, ring_row, vertex_offset, h, w, 10, 2, -1, vertices, rows, stats), SNERF_ERR_BAD_DESC, "V = -1");
  expect("V = 4 h w + 1", emit(ids, slot, flags, ring, ordinal, ring_row, vertex_offset, h, w, 10, 2, 193, vertices, rows, stats), SNERF_ERR_BAD_DESC,
         "V = 193");
  g_prefix = nullptr;
  expect("E = 0: nothing to do, null buffers",
         emit(ids, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, h, w, 0, 0, 0, nullptr, nullptr, stats), SNERF_OK, nullptr);

  bool written = stats[0] || stats[1] || stats[2] || stats[3];
  for (int k = 0; k < 192; ++k) written = written || slot[k] || next[k] || flags[k] || ring[k] || rank[k] || ordinal[k] || vertices[k] || rows[k];
  for (int k = 0; k < 48; ++k) written = written || side_bits[k];
  if (written) {
    printf("outputs were written\n");
    ++failures;
  }
  return verdict("outline");
}
