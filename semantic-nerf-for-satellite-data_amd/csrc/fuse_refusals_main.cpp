// The refusal paths of snerf_fuse_count, snerf_fuse_scatter and snerf_fuse_select (fuse.hip): see refusals_main.h.
#include "refusals_main.h"
#include "../../include/snerf_fuse.h"

static SnerfDsmGrid grid_of(double res, int xsize, int ysize, int ioff, int joff, int out_w, int out_h) {
  SnerfDsmGrid g = {1000.0, 2000.0, res, xsize, ysize, ioff, joff, out_w, out_h};
  return g;
}

int main() {
  // never dereferenced as device memory: every call is refused before a launch
  static double xyz[6];
  static unsigned slots[12];
  static long long offsets[13];
  static unsigned long long keys[8], words[12], stats[4];
  const SnerfDsmGrid good = grid_of(0.5, 4, 3, 0, 0, 4, 3);
  const double q = 1.0 / 65536.0;
  const int half[2] = {1, 2};

  // ---- what the two walks share: count, then scatter, through the same list ----
  for (int walk = 0; walk < 2; ++walk) {
    g_prefix = walk ? "snerf_fuse_scatter: " : "snerf_fuse_count: ";
    auto call = [&](const double* x, long long n, const SnerfDsmGrid* g, int radius, double z0, double qq, unsigned* s,
                    unsigned long long* st) {
      return walk ? snerf_fuse_scatter(x, n, 0, g, radius, z0, qq, offsets, 8, s, keys, st, nullptr)
                  : snerf_fuse_count(x, n, g, radius, z0, qq, s, st, nullptr);
    };
    expect("null xyz", call(nullptr, 2, &good, 0, 0.0, q, slots, stats), SNERF_ERR_NULL, "null");
    expect("null grid", call(xyz, 2, nullptr, 0, 0.0, q, slots, stats), SNERF_ERR_NULL, "null");
    expect("null count / cursor", call(xyz, 2, &good, 0, 0.0, q, nullptr, stats), SNERF_ERR_NULL, "null");
    expect("null stats", call(xyz, 2, &good, 0, 0.0, q, slots, nullptr), SNERF_ERR_NULL, "null");
    expect("n = -1", call(xyz, -1, &good, 0, 0.0, q, slots, stats), SNERF_ERR_BAD_DESC, "n = -1");
    expect("n = 2^31 + 1", call(xyz, 2147483649LL, &good, 0, 0.0, q, slots, stats), SNERF_ERR_BAD_DESC, "[0, 2^31]");
    expect("radius = -1", call(xyz, 2, &good, -1, 0.0, q, slots, stats), SNERF_ERR_BAD_DESC, "radius = -1");
    expect("radius = 8", call(xyz, 2, &good, 8, 0.0, q, slots, stats), SNERF_ERR_BAD_DESC, "radius = 8");
    SnerfDsmGrid g = grid_of(0.0, 4, 3, 0, 0, 4, 3);
    expect("res = 0", call(xyz, 2, &g, 0, 0.0, q, slots, stats), SNERF_ERR_BAD_DESC, "res > 0");
    g = grid_of(NAN, 4, 3, 0, 0, 4, 3);
    expect("res = NaN", call(xyz, 2, &g, 0, 0.0, q, slots, stats), SNERF_ERR_BAD_DESC, "res > 0");
    g = grid_of(0.5, 4, 3, 0, 0, 4, 0);
    expect("out_h = 0", call(xyz, 2, &g, 0, 0.0, q, slots, stats), SNERF_ERR_BAD_DESC, "positive sizes");
    g = grid_of(0.5, -2, 3, 0, 0, 4, 3);
    expect("xsize = -2", call(xyz, 2, &g, 0, 0.0, q, slots, stats), SNERF_ERR_BAD_DESC, "positive sizes");
    g = grid_of(0.5, 4, 3, 0, 2147483645, 4, 3);
    expect("joff + out_h > int32", call(xyz, 2, &g, 0, 0.0, q, slots, stats), SNERF_ERR_BAD_DESC, "int32");
    g = grid_of(0.5, 4, 3, 2147483644, 0, 4, 3);
    expect("ioff + out_w > int32", call(xyz, 2, &g, 0, 0.0, q, slots, stats), SNERF_ERR_BAD_DESC, "int32");
    g = good;
    g.yoff = INFINITY;
    expect("yoff = inf", call(xyz, 2, &g, 0, 0.0, q, slots, stats), SNERF_ERR_BAD_DESC, "res > 0");
    expect("q = 0", call(xyz, 2, &good, 0, 0.0, 0.0, slots, stats), SNERF_ERR_BAD_DESC, "q > 0");
    expect("q = -1", call(xyz, 2, &good, 0, 0.0, -1.0, slots, stats), SNERF_ERR_BAD_DESC, "q > 0");
    expect("q = inf", call(xyz, 2, &good, 0, 0.0, INFINITY, slots, stats), SNERF_ERR_BAD_DESC, "q > 0");
    expect("q = NaN", call(xyz, 2, &good, 0, 0.0, NAN, slots, stats), SNERF_ERR_BAD_DESC, "q > 0");
    expect("z0 = NaN", call(xyz, 2, &good, 0, NAN, q, slots, stats), SNERF_ERR_BAD_DESC, "z0 finite");
    // n == 0 is accepted and launches nothing; a bad argument beside it is still refused
    g_prefix = nullptr;
    expect("n = 0", call(nullptr, 0, &good, 0, 0.0, q, slots, stats), SNERF_OK, nullptr);
    g_prefix = walk ? "snerf_fuse_scatter: " : "snerf_fuse_count: ";
    expect("n = 0, radius = 9", call(xyz, 0, &good, 9, 0.0, q, slots, stats), SNERF_ERR_BAD_DESC, "radius = 9");
  }

  // ---- the scatter's own ----
  g_prefix = "snerf_fuse_scatter: ";
  expect("null offsets", snerf_fuse_scatter(xyz, 2, 0, &good, 0, 0.0, q, nullptr, 8, slots, keys, stats, nullptr), SNERF_ERR_NULL, "null");
  expect("null keys", snerf_fuse_scatter(xyz, 2, 0, &good, 0, 0.0, q, offsets, 8, slots, nullptr, stats, nullptr), SNERF_ERR_NULL, "null");
  expect("index0 = -1", snerf_fuse_scatter(xyz, 2, -1, &good, 0, 0.0, q, offsets, 8, slots, keys, stats, nullptr), SNERF_ERR_BAD_DESC,
         "index0 = -1");
  expect("index0 + n = 2^32", snerf_fuse_scatter(xyz, 2, 4294967294LL, &good, 0, 0.0, q, offsets, 8, slots, keys, stats, nullptr),
         SNERF_ERR_BAD_DESC, "index0 + n <= 2^32 - 1");
  expect("index0 = 2^63 - 1", snerf_fuse_scatter(xyz, 2, 9223372036854775807LL, &good, 0, 0.0, q, offsets, 8, slots, keys, stats, nullptr),
         SNERF_ERR_BAD_DESC, "index0");
  expect("capacity = -1", snerf_fuse_scatter(xyz, 2, 0, &good, 0, 0.0, q, offsets, -1, slots, keys, stats, nullptr), SNERF_ERR_BAD_DESC,
         "capacity = -1");

  // ---- the select ----
  g_prefix = "snerf_fuse_select: ";
  expect("null keys", snerf_fuse_select(nullptr, offsets, 8, slots, 12, half, 1, words, stats, nullptr), SNERF_ERR_NULL, "null");
  expect("null offsets", snerf_fuse_select(keys, nullptr, 8, slots, 12, half, 1, words, stats, nullptr), SNERF_ERR_NULL, "null");
  expect("null cursor", snerf_fuse_select(keys, offsets, 8, nullptr, 12, half, 1, words, stats, nullptr), SNERF_ERR_NULL, "null");
  expect("null quantiles", snerf_fuse_select(keys, offsets, 8, slots, 12, nullptr, 1, words, stats, nullptr), SNERF_ERR_NULL, "null");
  expect("null words", snerf_fuse_select(keys, offsets, 8, slots, 12, half, 1, nullptr, stats, nullptr), SNERF_ERR_NULL, "null");
  expect("null stats", snerf_fuse_select(keys, offsets, 8, slots, 12, half, 1, words, nullptr, nullptr), SNERF_ERR_NULL, "null");
  expect("capacity = -5", snerf_fuse_select(keys, offsets, -5, slots, 12, half, 1, words, stats, nullptr), SNERF_ERR_BAD_DESC, "capacity = -5");
  expect("cells = 0", snerf_fuse_select(keys, offsets, 8, slots, 0, half, 1, words, stats, nullptr), SNERF_ERR_BAD_DESC, "cells = 0");
  expect("cells = 2^31", snerf_fuse_select(keys, offsets, 8, slots, 2147483648LL, half, 1, words, stats, nullptr), SNERF_ERR_BAD_DESC,
         "cells = 2147483648");
  expect("K = 0", snerf_fuse_select(keys, offsets, 8, slots, 12, half, 0, words, stats, nullptr), SNERF_ERR_BAD_DESC, "n_quantiles = 0");
  expect("K = 9", snerf_fuse_select(keys, offsets, 8, slots, 12, half, 9, words, stats, nullptr), SNERF_ERR_BAD_DESC, "n_quantiles = 9");
  const int bad[][2] = {{3, 2}, {-1, 2}, {0, 0}, {1, 65537}, {1, -4}};
  const char* needles[] = {"(3, 2)", "(-1, 2)", "(0, 0)", "(1, 65537)", "(1, -4)"};
  for (int k = 0; k < 5; ++k)
    expect(needles[k], snerf_fuse_select(keys, offsets, 8, slots, 12, bad[k], 1, words, stats, nullptr), SNERF_ERR_BAD_DESC, needles[k]);
  const int second[4] = {1, 2, 5, 4};      // the table is read to its end: the SECOND pair is the bad one
  expect("quantile 1 = (5, 4)", snerf_fuse_select(keys, offsets, 8, slots, 12, second, 2, words, stats, nullptr), SNERF_ERR_BAD_DESC,
         "quantile 1 = (5, 4)");

  for (int k = 0; k < 12; ++k) if (slots[k] || words[k] || (k < 8 && keys[k]) || (k < 4 && stats[k])) { printf("outputs were written\n"); ++failures; break; }
  return verdict("fuse");
}
