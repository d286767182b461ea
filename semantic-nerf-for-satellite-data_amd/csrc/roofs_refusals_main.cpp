// The refusal paths of snerf_roofs_normals, snerf_roofs_link, snerf_roofs_moments and snerf_roofs_residuals (roofs.hip): see
// refusals_main.h.
#include "refusals_main.h"
#include "../../include/snerf_roofs.h"

int main() {
  // never dereferenced as device memory: every call is refused before a launch
  static int key[12], ids[12], tag[12], parent[12], fids[12], root[12];
  static float slope_e[12], slope_n[12], residual[12];
  static unsigned char code[12];
  static double planes[6];
  static unsigned long long stats[4], rows[32];
  const double q = 1.0 / 65536.0, inf = INFINITY;

  g_prefix = "snerf_roofs_normals: ";
  auto normals = [&](const int* k, const int* id, int h, int w, long long K, int r, double qq, double res, double c0, double s0, double tf,
                     double tw, float* se, float* sn, unsigned char* c, int* t, unsigned long long* s) {
    return snerf_roofs_normals(k, id, h, w, K, r, qq, res, c0, s0, tf, tw, se, sn, c, t, s, nullptr);
  };
  expect("null key", normals(nullptr, ids, 3, 4, 2, 1, q, 0.5, 1, 0, 0.01, 3, slope_e, slope_n, code, tag, stats), SNERF_ERR_NULL, "null");
  expect("null ids", normals(key, nullptr, 3, 4, 2, 1, q, 0.5, 1, 0, 0.01, 3, slope_e, slope_n, code, tag, stats), SNERF_ERR_NULL, "null");
  expect("null slope_e", normals(key, ids, 3, 4, 2, 1, q, 0.5, 1, 0, 0.01, 3, nullptr, slope_n, code, tag, stats), SNERF_ERR_NULL, "null");
  expect("null slope_n", normals(key, ids, 3, 4, 2, 1, q, 0.5, 1, 0, 0.01, 3, slope_e, nullptr, code, tag, stats), SNERF_ERR_NULL, "null");
  expect("null code", normals(key, ids, 3, 4, 2, 1, q, 0.5, 1, 0, 0.01, 3, slope_e, slope_n, nullptr, tag, stats), SNERF_ERR_NULL, "null");
  expect("null tag", normals(key, ids, 3, 4, 2, 1, q, 0.5, 1, 0, 0.01, 3, slope_e, slope_n, code, nullptr, stats), SNERF_ERR_NULL, "null");
  expect("null stats", normals(key, ids, 3, 4, 2, 1, q, 0.5, 1, 0, 0.01, 3, slope_e, slope_n, code, tag, nullptr), SNERF_ERR_NULL, "null");
  expect("h = 0", normals(key, ids, 0, 4, 2, 1, q, 0.5, 1, 0, 0.01, 3, slope_e, slope_n, code, tag, stats), SNERF_ERR_BAD_DESC, "h = 0");
  expect("w = -1", normals(key, ids, 3, -1, 2, 1, q, 0.5, 1, 0, 0.01, 3, slope_e, slope_n, code, tag, stats), SNERF_ERR_BAD_DESC, "w = -1");
  expect("h = 8193", normals(key, ids, 8193, 4, 2, 1, q, 0.5, 1, 0, 0.01, 3, slope_e, slope_n, code, tag, stats), SNERF_ERR_BAD_DESC,
         "at most 8192");
  expect("w = 2^31 - 1", normals(key, ids, 3, 2147483647, 2, 1, q, 0.5, 1, 0, 0.01, 3, slope_e, slope_n, code, tag, stats),
         SNERF_ERR_BAD_DESC, "at most 8192");
  expect("K = -1", normals(key, ids, 3, 4, -1, 1, q, 0.5, 1, 0, 0.01, 3, slope_e, slope_n, code, tag, stats), SNERF_ERR_BAD_DESC, "K = -1");
  expect("K = 2^27", normals(key, ids, 3, 4, 134217728LL, 1, q, 0.5, 1, 0, 0.01, 3, slope_e, slope_n, code, tag, stats), SNERF_ERR_BAD_DESC,
         "[0, 2^27)");
  expect("K = 2^40", normals(key, ids, 3, 4, 1LL << 40, 1, q, 0.5, 1, 0, 0.01, 3, slope_e, slope_n, code, tag, stats), SNERF_ERR_BAD_DESC,
         "[0, 2^27)");
  expect("radius = 0", normals(key, ids, 3, 4, 2, 0, q, 0.5, 1, 0, 0.01, 3, slope_e, slope_n, code, tag, stats), SNERF_ERR_BAD_DESC,
         "radius = 0");
  expect("radius = 5", normals(key, ids, 3, 4, 2, 5, q, 0.5, 1, 0, 0.01, 3, slope_e, slope_n, code, tag, stats), SNERF_ERR_BAD_DESC,
         "radius = 5");
  expect("q = 0", normals(key, ids, 3, 4, 2, 1, 0.0, 0.5, 1, 0, 0.01, 3, slope_e, slope_n, code, tag, stats), SNERF_ERR_BAD_DESC, "q > 0");
  expect("q = NaN", normals(key, ids, 3, 4, 2, 1, NAN, 0.5, 1, 0, 0.01, 3, slope_e, slope_n, code, tag, stats), SNERF_ERR_BAD_DESC, "q > 0");
  expect("res = -1", normals(key, ids, 3, 4, 2, 1, q, -1.0, 1, 0, 0.01, 3, slope_e, slope_n, code, tag, stats), SNERF_ERR_BAD_DESC, "res > 0");
  expect("res = inf", normals(key, ids, 3, 4, 2, 1, q, inf, 1, 0, 0.01, 3, slope_e, slope_n, code, tag, stats), SNERF_ERR_BAD_DESC, "res > 0");
  expect("cos0 = NaN", normals(key, ids, 3, 4, 2, 1, q, 0.5, NAN, 0, 0.01, 3, slope_e, slope_n, code, tag, stats), SNERF_ERR_BAD_DESC, "finite");
  expect("sin0 = inf", normals(key, ids, 3, 4, 2, 1, q, 0.5, 1, inf, 0.01, 3, slope_e, slope_n, code, tag, stats), SNERF_ERR_BAD_DESC, "finite");
  expect("tan2_flat = NaN", normals(key, ids, 3, 4, 2, 1, q, 0.5, 1, 0, NAN, 3, slope_e, slope_n, code, tag, stats), SNERF_ERR_BAD_DESC,
         "tan2_flat");
  expect("tan2_wall = inf", normals(key, ids, 3, 4, 2, 1, q, 0.5, 1, 0, 0.01, inf, slope_e, slope_n, code, tag, stats), SNERF_ERR_BAD_DESC,
         "tan2_flat");
  expect("tan2_flat < 0", normals(key, ids, 3, 4, 2, 1, q, 0.5, 1, 0, -0.01, 3, slope_e, slope_n, code, tag, stats), SNERF_ERR_BAD_DESC,
         "tan2_flat");
  expect("tan2_flat > tan2_wall", normals(key, ids, 3, 4, 2, 1, q, 0.5, 1, 0, 4, 3, slope_e, slope_n, code, tag, stats), SNERF_ERR_BAD_DESC,
         "tan2_flat");

  g_prefix = "snerf_roofs_link: ";
  expect("null tag", snerf_roofs_link(nullptr, 3, 4, 4, parent, stats, nullptr), SNERF_ERR_NULL, "null");
  expect("null parent", snerf_roofs_link(tag, 3, 4, 4, nullptr, stats, nullptr), SNERF_ERR_NULL, "null");
  expect("null stats", snerf_roofs_link(tag, 3, 4, 4, parent, nullptr, nullptr), SNERF_ERR_NULL, "null");
  expect("h = -2", snerf_roofs_link(tag, -2, 4, 4, parent, stats, nullptr), SNERF_ERR_BAD_DESC, "h = -2");
  expect("w = 8193", snerf_roofs_link(tag, 3, 8193, 4, parent, stats, nullptr), SNERF_ERR_BAD_DESC, "at most 8192");
  expect("connectivity = 6", snerf_roofs_link(tag, 3, 4, 6, parent, stats, nullptr), SNERF_ERR_BAD_DESC, "connectivity = 6");

  g_prefix = "snerf_roofs_moments: ";
  auto moments = [&](const int* f, const int* r, const int* k, const int* t, int h, int w, long long F, int row0, int row1,
                     unsigned long long* rw, unsigned long long* s) {
    return snerf_roofs_moments(f, r, k, t, h, w, F, row0, row1, rw, s, nullptr);
  };
  expect("null fids", moments(nullptr, root, key, tag, 3, 4, 2, 0, 3, rows, stats), SNERF_ERR_NULL, "null");
  expect("null root", moments(fids, nullptr, key, tag, 3, 4, 2, 0, 3, rows, stats), SNERF_ERR_NULL, "null");
  expect("null key", moments(fids, root, nullptr, tag, 3, 4, 2, 0, 3, rows, stats), SNERF_ERR_NULL, "null");
  expect("null tag", moments(fids, root, key, nullptr, 3, 4, 2, 0, 3, rows, stats), SNERF_ERR_NULL, "null");
  expect("null rows, F = 2", moments(fids, root, key, tag, 3, 4, 2, 0, 3, nullptr, stats), SNERF_ERR_NULL, "null");
  expect("null stats", moments(fids, root, key, tag, 3, 4, 2, 0, 3, rows, nullptr), SNERF_ERR_NULL, "null");
  expect("h = 0", moments(fids, root, key, tag, 0, 4, 2, 0, 0, rows, stats), SNERF_ERR_BAD_DESC, "h = 0");
  expect("h = 8193", moments(fids, root, key, tag, 8193, 4, 2, 0, 3, rows, stats), SNERF_ERR_BAD_DESC, "at most 8192");
  expect("F = -1", moments(fids, root, key, tag, 3, 4, -1, 0, 3, rows, stats), SNERF_ERR_BAD_DESC, "F = -1");
  expect("F = 2^27", moments(fids, root, key, tag, 3, 4, 134217728LL, 0, 3, rows, stats), SNERF_ERR_BAD_DESC, "[0, 2^27)");
  expect("row0 = -1", moments(fids, root, key, tag, 3, 4, 2, -1, 3, rows, stats), SNERF_ERR_BAD_DESC, "row0 = -1");
  expect("row1 = 4 > h", moments(fids, root, key, tag, 3, 4, 2, 0, 4, rows, stats), SNERF_ERR_BAD_DESC, "row1 = 4");
  expect("row0 > row1", moments(fids, root, key, tag, 3, 4, 2, 2, 1, rows, stats), SNERF_ERR_BAD_DESC, "row0 = 2");
  g_prefix = nullptr;
  // accepted and empty: nothing is launched, nothing is written
  expect("F = 0, null rows", moments(fids, root, key, tag, 3, 4, 0, 0, 3, nullptr, stats), SNERF_OK, nullptr);
  expect("an empty band", moments(fids, root, key, tag, 3, 4, 2, 2, 2, rows, stats), SNERF_OK, nullptr);

  g_prefix = "snerf_roofs_residuals: ";
  auto resid = [&](const int* f, const int* r, const int* k, int h, int w, long long F, const double* p, double qq, double unit, int row0,
                   int row1, float* out, unsigned long long* rw, unsigned long long* s) {
    return snerf_roofs_residuals(f, r, k, h, w, F, p, qq, unit, row0, row1, out, rw, s, nullptr);
  };
  expect("null fids", resid(nullptr, root, key, 3, 4, 2, planes, q, 64.0, 0, 3, residual, rows, stats), SNERF_ERR_NULL, "null");
  expect("null root", resid(fids, nullptr, key, 3, 4, 2, planes, q, 64.0, 0, 3, residual, rows, stats), SNERF_ERR_NULL, "null");
  expect("null key", resid(fids, root, nullptr, 3, 4, 2, planes, q, 64.0, 0, 3, residual, rows, stats), SNERF_ERR_NULL, "null");
  expect("null planes, F = 2", resid(fids, root, key, 3, 4, 2, nullptr, q, 64.0, 0, 3, residual, rows, stats), SNERF_ERR_NULL, "null");
  expect("null residual", resid(fids, root, key, 3, 4, 2, planes, q, 64.0, 0, 3, nullptr, rows, stats), SNERF_ERR_NULL, "null");
  expect("null rows, F = 2", resid(fids, root, key, 3, 4, 2, planes, q, 64.0, 0, 3, residual, nullptr, stats), SNERF_ERR_NULL, "null");
  expect("null stats", resid(fids, root, key, 3, 4, 2, planes, q, 64.0, 0, 3, residual, rows, nullptr), SNERF_ERR_NULL, "null");
  expect("w = 0", resid(fids, root, key, 3, 0, 2, planes, q, 64.0, 0, 3, residual, rows, stats), SNERF_ERR_BAD_DESC, "w = 0");
  expect("w = 8193", resid(fids, root, key, 3, 8193, 2, planes, q, 64.0, 0, 3, residual, rows, stats), SNERF_ERR_BAD_DESC, "at most 8192");
  expect("F = 2^27", resid(fids, root, key, 3, 4, 134217728LL, planes, q, 64.0, 0, 3, residual, rows, stats), SNERF_ERR_BAD_DESC, "[0, 2^27)");
  expect("row1 = 5 > h", resid(fids, root, key, 3, 4, 2, planes, q, 64.0, 0, 5, residual, rows, stats), SNERF_ERR_BAD_DESC, "row1 = 5");
  expect("q = 0", resid(fids, root, key, 3, 4, 2, planes, 0.0, 64.0, 0, 3, residual, rows, stats), SNERF_ERR_BAD_DESC, "q > 0");
  expect("q = inf", resid(fids, root, key, 3, 4, 2, planes, inf, 64.0, 0, 3, residual, rows, stats), SNERF_ERR_BAD_DESC, "q > 0");
  expect("unit = 0", resid(fids, root, key, 3, 4, 2, planes, q, 0.0, 0, 3, residual, rows, stats), SNERF_ERR_BAD_DESC, "unit > 0");
  expect("unit = NaN", resid(fids, root, key, 3, 4, 2, planes, q, NAN, 0, 3, residual, rows, stats), SNERF_ERR_BAD_DESC, "unit > 0");
  expect("unit = -64", resid(fids, root, key, 3, 4, 2, planes, q, -64.0, 0, 3, residual, rows, stats), SNERF_ERR_BAD_DESC, "unit > 0");
  g_prefix = nullptr;
  expect("an empty band", resid(fids, root, key, 3, 4, 2, planes, q, 64.0, 1, 1, residual, rows, stats), SNERF_OK, nullptr);

  for (int k = 0; k < 12; ++k)
    if (tag[k] || parent[k] || code[k] || slope_e[k] != 0.f || slope_n[k] != 0.f || residual[k] != 0.f || (k < 4 && stats[k])) {
      printf("outputs were written\n");
      ++failures;
      break;
    }
  for (int k = 0; k < 32; ++k)
    if (rows[k]) { printf("the rows were written\n"); ++failures; break; }
  return verdict("roofs");
}
