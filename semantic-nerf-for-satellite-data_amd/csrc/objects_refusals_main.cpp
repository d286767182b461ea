// The refusal paths of snerf_objects_link and snerf_objects_stats (objects.hip): see refusals_main.h.
#include "refusals_main.h"
#include "../../include/snerf_objects.h"

int main() {
  // never dereferenced as device memory: every call is refused before a launch
  static unsigned char label[12], classes[256], with_255[256];
  static int parent[12], ids[12];
  static float alt[12];
  static unsigned long long rows[2 * SNERF_OBJECTS_ROW_WORDS], stats[4];
  classes[3] = 1;
  with_255[3] = with_255[255] = 1;
  const double q = 1.0 / 65536.0;

  g_prefix = "snerf_objects_link: ";
  expect("null label", snerf_objects_link(nullptr, 3, 4, classes, 4, parent, stats, nullptr), SNERF_ERR_NULL, "null");
  expect("null member_host", snerf_objects_link(label, 3, 4, nullptr, 4, parent, stats, nullptr), SNERF_ERR_NULL, "null");
  expect("null parent", snerf_objects_link(label, 3, 4, classes, 4, nullptr, stats, nullptr), SNERF_ERR_NULL, "null");
  expect("null stats", snerf_objects_link(label, 3, 4, classes, 4, parent, nullptr, nullptr), SNERF_ERR_NULL, "null");
  expect("h = 0", snerf_objects_link(label, 0, 4, classes, 4, parent, stats, nullptr), SNERF_ERR_BAD_DESC, "h = 0");
  expect("w = -1", snerf_objects_link(label, 3, -1, classes, 4, parent, stats, nullptr), SNERF_ERR_BAD_DESC, "w = -1");
  expect("h * w = 2^31", snerf_objects_link(label, 32768, 65536, classes, 4, parent, stats, nullptr), SNERF_ERR_BAD_DESC, "below 2^31");
  expect("h * w = 2^62", snerf_objects_link(label, 2147483647, 2147483647, classes, 4, parent, stats, nullptr), SNERF_ERR_BAD_DESC,
         "below 2^31");
  expect("connectivity = 3", snerf_objects_link(label, 3, 4, classes, 3, parent, stats, nullptr), SNERF_ERR_BAD_DESC, "connectivity = 3");
  expect("connectivity = 0", snerf_objects_link(label, 3, 4, classes, 0, parent, stats, nullptr), SNERF_ERR_BAD_DESC, "connectivity = 0");
  expect("member_host[255]", snerf_objects_link(label, 3, 4, with_255, 8, parent, stats, nullptr), SNERF_ERR_BAD_DESC, "member_host[255]");

  g_prefix = "snerf_objects_stats: ";
  auto call = [&](const int* i, const unsigned char* l, const float* a, int h, int w, long long K, const unsigned char* g, int ring,
                  double z0, double qq, int row0, int row1, unsigned long long* r, unsigned long long* s) {
    return snerf_objects_stats(i, l, a, h, w, K, g, ring, z0, qq, row0, row1, r, s, nullptr);
  };
  expect("null ids", call(nullptr, label, alt, 3, 4, 2, classes, 2, 0.0, q, 0, 3, rows, stats), SNERF_ERR_NULL, "null");
  expect("null label", call(ids, nullptr, alt, 3, 4, 2, classes, 2, 0.0, q, 0, 3, rows, stats), SNERF_ERR_NULL, "null");
  expect("null alt", call(ids, label, nullptr, 3, 4, 2, classes, 2, 0.0, q, 0, 3, rows, stats), SNERF_ERR_NULL, "null");
  expect("null ground_host", call(ids, label, alt, 3, 4, 2, nullptr, 2, 0.0, q, 0, 3, rows, stats), SNERF_ERR_NULL, "null");
  expect("null rows", call(ids, label, alt, 3, 4, 2, classes, 2, 0.0, q, 0, 3, nullptr, stats), SNERF_ERR_NULL, "null");
  expect("null stats", call(ids, label, alt, 3, 4, 2, classes, 2, 0.0, q, 0, 3, rows, nullptr), SNERF_ERR_NULL, "null");
  expect("h = 0", call(ids, label, alt, 0, 4, 2, classes, 2, 0.0, q, 0, 0, rows, stats), SNERF_ERR_BAD_DESC, "h = 0");
  expect("h * w = 2^31", call(ids, label, alt, 65536, 32768, 2, classes, 0, 0.0, q, 0, 3, rows, stats), SNERF_ERR_BAD_DESC, "below 2^31");
  expect("K = -1", call(ids, label, alt, 3, 4, -1, classes, 2, 0.0, q, 0, 3, rows, stats), SNERF_ERR_BAD_DESC, "K = -1");
  expect("K = 2^31", call(ids, label, alt, 3, 4, 2147483648LL, classes, 2, 0.0, q, 0, 3, rows, stats), SNERF_ERR_BAD_DESC,
         "K = 2147483648");
  expect("ring = -1", call(ids, label, alt, 3, 4, 2, classes, -1, 0.0, q, 0, 3, rows, stats), SNERF_ERR_BAD_DESC, "ring = -1");
  expect("ring = 8", call(ids, label, alt, 3, 4, 2, classes, 8, 0.0, q, 0, 3, rows, stats), SNERF_ERR_BAD_DESC, "ring = 8");
  // 20000 x 20000 cells x 15^2 = 9e10 pairs; x 3^2 = 3.6e9 fits, x 5^2 = 1e10 does not
  expect("pair bound, ring = 7", call(ids, label, alt, 20000, 20000, 2, classes, 7, 0.0, q, 0, 3, rows, stats), SNERF_ERR_BAD_DESC,
         "below 2^32");
  expect("pair bound, ring = 2", call(ids, label, alt, 20000, 20000, 2, classes, 2, 0.0, q, 0, 3, rows, stats), SNERF_ERR_BAD_DESC,
         "below 2^32");
  expect("row0 = -1", call(ids, label, alt, 3, 4, 2, classes, 2, 0.0, q, -1, 3, rows, stats), SNERF_ERR_BAD_DESC, "row0 = -1");
  expect("row1 = 4 > h", call(ids, label, alt, 3, 4, 2, classes, 2, 0.0, q, 0, 4, rows, stats), SNERF_ERR_BAD_DESC, "row1 = 4");
  expect("row0 > row1", call(ids, label, alt, 3, 4, 2, classes, 2, 0.0, q, 2, 1, rows, stats), SNERF_ERR_BAD_DESC, "row0 = 2");
  expect("q = 0", call(ids, label, alt, 3, 4, 2, classes, 2, 0.0, 0.0, 0, 3, rows, stats), SNERF_ERR_BAD_DESC, "q > 0");
  expect("q = NaN", call(ids, label, alt, 3, 4, 2, classes, 2, 0.0, NAN, 0, 3, rows, stats), SNERF_ERR_BAD_DESC, "q > 0");
  expect("q = inf", call(ids, label, alt, 3, 4, 2, classes, 2, 0.0, INFINITY, 0, 3, rows, stats), SNERF_ERR_BAD_DESC, "q > 0");
  expect("z0 = inf", call(ids, label, alt, 3, 4, 2, classes, 2, INFINITY, q, 0, 3, rows, stats), SNERF_ERR_BAD_DESC, "z0 finite");
  expect("ground_host[255]", call(ids, label, alt, 3, 4, 2, with_255, 2, 0.0, q, 0, 3, rows, stats), SNERF_ERR_BAD_DESC,
         "ground_host[255]");
  // an empty problem is accepted and launches nothing; a bad argument beside it is still refused
  g_prefix = nullptr;
  expect("K = 0", call(ids, label, alt, 3, 4, 0, classes, 2, 0.0, q, 0, 3, nullptr, stats), SNERF_OK, nullptr);
  expect("an empty band", call(ids, label, alt, 3, 4, 2, classes, 2, 0.0, q, 1, 1, rows, stats), SNERF_OK, nullptr);
  g_prefix = "snerf_objects_stats: ";
  expect("K = 0, ring = 9", call(ids, label, alt, 3, 4, 0, classes, 9, 0.0, q, 0, 3, rows, stats), SNERF_ERR_BAD_DESC, "ring = 9");

  for (int k = 0; k < 12; ++k)
    if (parent[k] || (k < 4 && stats[k])) { printf("outputs were written\n"); ++failures; break; }
  for (int k = 0; k < 2 * SNERF_OBJECTS_ROW_WORDS; ++k)
    if (rows[k]) { printf("outputs were written\n"); ++failures; break; }
  return verdict("objects");
}
