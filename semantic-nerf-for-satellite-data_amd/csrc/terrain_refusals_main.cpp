// The refusal paths of snerf_terrain_workspace_bytes, snerf_terrain_keys, snerf_terrain_open and snerf_terrain_fill (terrain.hip):
// see refusals_main.h.
#include "refusals_main.h"
#include "../../include/snerf_terrain.h"

int main() {
  // never dereferenced as device memory: every call is refused before a launch
  static unsigned char label[12], flags[12], classes[256], with_255[256];
  static int key[12], key_out[12], reach[12];
  static float alt[12], dtm[12], ndsm[12];
  static unsigned long long stats[3], ws[24];
  classes[3] = 1;
  with_255[3] = with_255[255] = 1;
  const double q = 1.0 / 65536.0;

  g_prefix = "snerf_terrain_workspace_bytes: ";
  expect("h = 0", (int)snerf_terrain_workspace_bytes(0, 4), -1, "h = 0");
  expect("w = -1", (int)snerf_terrain_workspace_bytes(3, -1), -1, "w = -1");
  expect("h * w = 2^31", (int)snerf_terrain_workspace_bytes(32768, 65536), -1, "below 2^31");
  expect("h * w = 2^62", (int)snerf_terrain_workspace_bytes(2147483647, 2147483647), -1, "below 2^31");
  g_prefix = nullptr;
  expect("3 x 4: 192 bytes", snerf_terrain_workspace_bytes(3, 4) == 192 ? 0 : 1, 0, nullptr);
  expect("46340^2: beyond 32 bits", snerf_terrain_workspace_bytes(46340, 46340) == 16LL * 46340 * 46340 ? 0 : 1, 0, nullptr);

  g_prefix = "snerf_terrain_keys: ";
  auto keys = [&](const float* a, const unsigned char* l, int h, int w, const unsigned char* b, double z0, double qq, int* k,
                  unsigned char* f, unsigned long long* s) { return snerf_terrain_keys(a, l, h, w, b, z0, qq, k, f, s, nullptr); };
  expect("null alt", keys(nullptr, label, 3, 4, classes, 0.0, q, key, flags, stats), SNERF_ERR_NULL, "null");
  expect("null key", keys(alt, label, 3, 4, classes, 0.0, q, nullptr, flags, stats), SNERF_ERR_NULL, "null");
  expect("null flags", keys(alt, label, 3, 4, classes, 0.0, q, key, nullptr, stats), SNERF_ERR_NULL, "null");
  expect("null stats", keys(alt, label, 3, 4, classes, 0.0, q, key, flags, nullptr), SNERF_ERR_NULL, "null");
  expect("label without a table", keys(alt, label, 3, 4, nullptr, 0.0, q, key, flags, stats), SNERF_ERR_NULL, "blocked_host null");
  expect("a table without label", keys(alt, nullptr, 3, 4, classes, 0.0, q, key, flags, stats), SNERF_ERR_NULL, "label null");
  expect("h = 0", keys(alt, label, 0, 4, classes, 0.0, q, key, flags, stats), SNERF_ERR_BAD_DESC, "h = 0");
  expect("w = -1", keys(alt, label, 3, -1, classes, 0.0, q, key, flags, stats), SNERF_ERR_BAD_DESC, "w = -1");
  expect("h * w = 2^31", keys(alt, label, 65536, 32768, classes, 0.0, q, key, flags, stats), SNERF_ERR_BAD_DESC, "below 2^31");
  expect("q = 0", keys(alt, label, 3, 4, classes, 0.0, 0.0, key, flags, stats), SNERF_ERR_BAD_DESC, "q > 0");
  expect("q = -1", keys(alt, label, 3, 4, classes, 0.0, -1.0, key, flags, stats), SNERF_ERR_BAD_DESC, "q > 0");
  expect("q = NaN", keys(alt, label, 3, 4, classes, 0.0, NAN, key, flags, stats), SNERF_ERR_BAD_DESC, "q > 0");
  expect("q = inf", keys(alt, label, 3, 4, classes, 0.0, INFINITY, key, flags, stats), SNERF_ERR_BAD_DESC, "q > 0");
  expect("z0 = NaN", keys(alt, label, 3, 4, classes, NAN, q, key, flags, stats), SNERF_ERR_BAD_DESC, "z0 finite");
  expect("z0 = inf", keys(alt, label, 3, 4, classes, INFINITY, q, key, flags, stats), SNERF_ERR_BAD_DESC, "z0 finite");
  expect("blocked_host[255]", keys(alt, label, 3, 4, with_255, 0.0, q, key, flags, stats), SNERF_ERR_BAD_DESC, "blocked_host[255]");

  g_prefix = "snerf_terrain_open: ";
  auto open = [&](const int* in, int h, int w, int radius, long long threshold, int* out, unsigned char* f, void* scratch,
                  unsigned long long* s) { return snerf_terrain_open(in, h, w, radius, threshold, out, f, scratch, s, nullptr); };
  expect("null key_in", open(nullptr, 3, 4, 2, 5, key_out, flags, ws, stats), SNERF_ERR_NULL, "null");
  expect("null key_out", open(key, 3, 4, 2, 5, nullptr, flags, ws, stats), SNERF_ERR_NULL, "null");
  expect("null ws", open(key, 3, 4, 2, 5, key_out, flags, nullptr, stats), SNERF_ERR_NULL, "null");
  expect("null stats", open(key, 3, 4, 2, 5, key_out, flags, ws, nullptr), SNERF_ERR_NULL, "null");
  expect("h = 0", open(key, 0, 4, 2, 5, key_out, flags, ws, stats), SNERF_ERR_BAD_DESC, "h = 0");
  expect("h * w = 2^31", open(key, 32768, 65536, 2, 5, key_out, flags, ws, stats), SNERF_ERR_BAD_DESC, "below 2^31");
  expect("h * w = 2^62", open(key, 2147483647, 2147483647, 2, 5, key_out, flags, ws, stats), SNERF_ERR_BAD_DESC, "below 2^31");
  expect("radius = 0", open(key, 3, 4, 0, 5, key_out, flags, ws, stats), SNERF_ERR_BAD_DESC, "radius = 0");
  expect("radius = -3", open(key, 3, 4, -3, 5, key_out, flags, ws, stats), SNERF_ERR_BAD_DESC, "radius = -3");
  expect("radius = 513", open(key, 3, 4, 513, 5, key_out, flags, ws, stats), SNERF_ERR_BAD_DESC, "radius = 513");
  expect("threshold = -1", open(key, 3, 4, 2, -1, key_out, flags, ws, stats), SNERF_ERR_BAD_DESC, "threshold = -1");
  expect("key_out == key_in", open(key, 3, 4, 2, 5, key, flags, ws, stats), SNERF_ERR_BAD_DESC, "must not alias");
  expect("key_out == key_in, no flags", open(key, 3, 4, 2, 5, key, nullptr, ws, stats), SNERF_ERR_BAD_DESC, "must not alias");

  g_prefix = "snerf_terrain_fill: ";
  auto fill = [&](const int* k, const unsigned char* f, const float* a, int h, int w, double z0, double qq, float* d, float* n, int* r,
                  void* scratch, unsigned long long* s) { return snerf_terrain_fill(k, f, a, h, w, z0, qq, d, n, r, scratch, s, nullptr); };
  expect("null key", fill(nullptr, flags, alt, 3, 4, 0.0, q, dtm, ndsm, reach, ws, stats), SNERF_ERR_NULL, "null");
  expect("null flags", fill(key, nullptr, alt, 3, 4, 0.0, q, dtm, ndsm, reach, ws, stats), SNERF_ERR_NULL, "null");
  expect("null alt", fill(key, flags, nullptr, 3, 4, 0.0, q, dtm, ndsm, reach, ws, stats), SNERF_ERR_NULL, "null");
  expect("null dtm", fill(key, flags, alt, 3, 4, 0.0, q, nullptr, ndsm, reach, ws, stats), SNERF_ERR_NULL, "null");
  expect("null ndsm", fill(key, flags, alt, 3, 4, 0.0, q, dtm, nullptr, reach, ws, stats), SNERF_ERR_NULL, "null");
  expect("null ws", fill(key, flags, alt, 3, 4, 0.0, q, dtm, ndsm, reach, nullptr, stats), SNERF_ERR_NULL, "null");
  expect("null stats", fill(key, flags, alt, 3, 4, 0.0, q, dtm, ndsm, reach, ws, nullptr), SNERF_ERR_NULL, "null");
  expect("h = -2", fill(key, flags, alt, -2, 4, 0.0, q, dtm, ndsm, reach, ws, stats), SNERF_ERR_BAD_DESC, "h = -2");
  expect("h * w = 2^31", fill(key, flags, alt, 65536, 32768, 0.0, q, dtm, ndsm, reach, ws, stats), SNERF_ERR_BAD_DESC, "below 2^31");
  expect("q = 0", fill(key, flags, alt, 3, 4, 0.0, 0.0, dtm, ndsm, reach, ws, stats), SNERF_ERR_BAD_DESC, "q > 0");
  expect("q = NaN", fill(key, flags, alt, 3, 4, 0.0, NAN, dtm, ndsm, reach, ws, stats), SNERF_ERR_BAD_DESC, "q > 0");
  expect("z0 = -inf", fill(key, flags, alt, 3, 4, -INFINITY, q, dtm, ndsm, reach, ws, stats), SNERF_ERR_BAD_DESC, "z0 finite");
  // a null reach is legal; a bad argument beside it is still refused
  expect("null reach, w = 0", fill(key, flags, alt, 3, 0, 0.0, q, dtm, ndsm, nullptr, ws, stats), SNERF_ERR_BAD_DESC, "w = 0");

  for (int k = 0; k < 12; ++k)
    if (key[k] || key_out[k] || flags[k] || reach[k] || dtm[k] != 0.f || ndsm[k] != 0.f || (k < 3 && stats[k])) {
      printf("outputs were written\n");
      ++failures;
      break;
    }
  for (int k = 0; k < 24; ++k)
    if (ws[k]) { printf("the workspace was written\n"); ++failures; break; }
  return verdict("terrain");
}
