// The refusal paths of snerf_warp_planes and snerf_warp_labels (warp.hip): see refusals_main.h.
#include "refusals_main.h"
#include "../../include/snerf_warp.h"

static SnerfWarpMap base_map() {
  SnerfWarpMap m = {0.25, 2.0, -1.5, 2.0, 8, 6, 4, 3};
  return m;
}

int main() {
  // never dereferenced as device memory: every call is refused before a launch
  static float src[48], dst[12];
  static unsigned char lsrc[48], ldst[12];
  static unsigned long long stats[3];
  const SnerfWarpMap ok = base_map();
  what_width = 52;

  g_prefix = "snerf_warp_planes: ";
  auto planes = [&](const float* s, int n, const SnerfWarpMap* m, int method, double min_valid, float* d, unsigned long long* st) {
    return snerf_warp_planes(s, n, m, method, min_valid, d, st, nullptr);
  };
  expect("null src", planes(nullptr, 1, &ok, SNERF_WARP_AVERAGE, 0.5, dst, stats), SNERF_ERR_NULL, "null");
  expect("null map", planes(src, 1, nullptr, SNERF_WARP_AVERAGE, 0.5, dst, stats), SNERF_ERR_NULL, "null");
  expect("null dst", planes(src, 1, &ok, SNERF_WARP_AVERAGE, 0.5, nullptr, stats), SNERF_ERR_NULL, "null");
  expect("null stats", planes(src, 1, &ok, SNERF_WARP_AVERAGE, 0.5, dst, nullptr), SNERF_ERR_NULL, "null");
  expect("dst == src", planes(src, 1, &ok, SNERF_WARP_AVERAGE, 0.5, src, stats), SNERF_ERR_BAD_DESC, "must not alias");
  expect("method = -1", planes(src, 1, &ok, -1, 0.5, dst, stats), SNERF_ERR_BAD_DESC, "method = -1");
  expect("method = MODE", planes(src, 1, &ok, SNERF_WARP_MODE, 0.5, dst, stats), SNERF_ERR_BAD_DESC, "method = 5");
  expect("planes = 0", planes(src, 0, &ok, SNERF_WARP_AVERAGE, 0.5, dst, stats), SNERF_ERR_BAD_DESC, "planes = 0");
  expect("planes = 17", planes(src, 17, &ok, SNERF_WARP_AVERAGE, 0.5, dst, stats), SNERF_ERR_BAD_DESC, "planes = 17");
  expect("min_valid = 0", planes(src, 1, &ok, SNERF_WARP_AVERAGE, 0.0, dst, stats), SNERF_ERR_BAD_DESC, "min_valid");
  expect("min_valid = 1.5", planes(src, 1, &ok, SNERF_WARP_AVERAGE, 1.5, dst, stats), SNERF_ERR_BAD_DESC, "min_valid");
  expect("min_valid = NaN", planes(src, 1, &ok, SNERF_WARP_AVERAGE, NAN, dst, stats), SNERF_ERR_BAD_DESC, "min_valid");
  expect("min_valid = NaN, NEAREST", planes(src, 1, &ok, SNERF_WARP_NEAREST, NAN, dst, stats), SNERF_ERR_BAD_DESC, "min_valid");

  // the map's rules, through both entries
  auto both = [&](const char* what, SnerfWarpMap m, int method, int label_method, const char* needle) {
    g_prefix = "snerf_warp_planes: ";
    expect(what, planes(src, 1, &m, method, 0.5, dst, stats), SNERF_ERR_BAD_DESC, needle);
    g_prefix = "snerf_warp_labels: ";
    expect(what, snerf_warp_labels(lsrc, &m, label_method, ldst, stats, nullptr), SNERF_ERR_BAD_DESC, needle);
  };
  SnerfWarpMap m = ok;
  m.src_w = 0;
  both("src_w = 0", m, SNERF_WARP_BILINEAR, SNERF_WARP_NEAREST, ">= 1");
  m = ok, m.dst_h = -2;
  both("dst_h = -2", m, SNERF_WARP_BILINEAR, SNERF_WARP_NEAREST, ">= 1");
  m = ok, m.src_w = 65536, m.src_h = 32768;
  both("src h * w = 2^31", m, SNERF_WARP_BILINEAR, SNERF_WARP_NEAREST, "below 2^31");
  m = ok, m.dst_w = 2147483647, m.dst_h = 2147483647;
  both("dst h * w = 2^62", m, SNERF_WARP_BILINEAR, SNERF_WARP_NEAREST, "below 2^31");
  m = ok, m.step_x = 0.0;
  both("step_x = 0", m, SNERF_WARP_BILINEAR, SNERF_WARP_NEAREST, "step_x");
  m = ok, m.step_y = -1.0;
  both("step_y = -1", m, SNERF_WARP_BILINEAR, SNERF_WARP_NEAREST, "step_y");
  m = ok, m.step_x = NAN;
  both("step_x = NaN", m, SNERF_WARP_BILINEAR, SNERF_WARP_NEAREST, "step_x");
  m = ok, m.step_y = INFINITY;
  both("step_y = inf", m, SNERF_WARP_BILINEAR, SNERF_WARP_NEAREST, "step_y");
  m = ok, m.off_x = 2147483648.0;
  both("off_x = 2^31", m, SNERF_WARP_BILINEAR, SNERF_WARP_NEAREST, "below 2^31");
  m = ok, m.off_y = -2147483644.0;
  both("off_y = -2^31 + 4, 3 rows of 2", m, SNERF_WARP_BILINEAR, SNERF_WARP_NEAREST, "below 2^31");
  m = ok, m.off_x = NAN;
  both("off_x = NaN", m, SNERF_WARP_BILINEAR, SNERF_WARP_NEAREST, "below 2^31");
  m = ok, m.off_y = -INFINITY;
  both("off_y = -inf", m, SNERF_WARP_BILINEAR, SNERF_WARP_NEAREST, "below 2^31");
  m = ok, m.step_x = 1e9, m.dst_w = 4;
  both("4 columns of 1e9", m, SNERF_WARP_NEAREST, SNERF_WARP_NEAREST, "below 2^31");
  m = ok, m.step_x = 64.5;
  both("step_x = 64.5, an area method", m, SNERF_WARP_AVERAGE, SNERF_WARP_MODE, "SNERF_WARP_MAX_STEP");
  m = ok, m.step_y = 65.0;
  both("step_y = 65, an area method", m, SNERF_WARP_MAX, SNERF_WARP_MODE, "SNERF_WARP_MAX_STEP");

  g_prefix = "snerf_warp_labels: ";
  expect("null src", snerf_warp_labels(nullptr, &ok, SNERF_WARP_MODE, ldst, stats, nullptr), SNERF_ERR_NULL, "null");
  expect("null map", snerf_warp_labels(lsrc, nullptr, SNERF_WARP_MODE, ldst, stats, nullptr), SNERF_ERR_NULL, "null");
  expect("null dst", snerf_warp_labels(lsrc, &ok, SNERF_WARP_MODE, nullptr, stats, nullptr), SNERF_ERR_NULL, "null");
  expect("null stats", snerf_warp_labels(lsrc, &ok, SNERF_WARP_MODE, ldst, nullptr, nullptr), SNERF_ERR_NULL, "null");
  expect("dst == src", snerf_warp_labels(lsrc, &ok, SNERF_WARP_MODE, lsrc, stats, nullptr), SNERF_ERR_BAD_DESC, "must not alias");
  expect("method = BILINEAR", snerf_warp_labels(lsrc, &ok, SNERF_WARP_BILINEAR, ldst, stats, nullptr), SNERF_ERR_BAD_DESC, "method = 1");
  expect("method = 6", snerf_warp_labels(lsrc, &ok, 6, ldst, stats, nullptr), SNERF_ERR_BAD_DESC, "method = 6");

  for (int k = 0; k < 12; ++k)
    if (dst[k] != 0.f || ldst[k] || (k < 3 && stats[k])) {
      printf("outputs were written\n");
      ++failures;
      break;
    }
  return verdict("warp");
}
