// The refusal paths of snerf_solar_horizon, snerf_solar_svf and snerf_solar_irradiate (solar.hip): see refusals_main.h.
#include "refusals_main.h"
#include "../../include/snerf_solar.h"

int main() {
  // never dereferenced as device memory: every call is refused before a launch.  The rows ARE read: they are host tables.
  static float dsm[12], horizon[24], svf[12], slope_e[12], slope_n[12];
  static double direct[12];
  static unsigned int count[12];
  const double inf = INFINITY, s2 = sqrt(0.5);
  const double good_dirs[4] = {1.0, 0.0, s2, -s2};
  const double good_suns[14] = {0.0, 0.0, 0.5, 0.0, 0.6, 0.8, 1.0, 1.0, 0.25, 0.1, 0.6, 0.0, 0.8, 0.0};

  g_prefix = "snerf_solar_horizon: ";
  auto horizon_ = [&](const float* d, int h, int w, const double* rows, int n, double bias, double z_top, double max_dist, float* out) {
    return snerf_solar_horizon(d, h, w, rows, n, bias, z_top, max_dist, out, nullptr);
  };
  auto bad_dir = [&](int at, double v) {
    static double rows[4];
    memcpy(rows, good_dirs, sizeof rows);
    rows[at] = v;
    return rows;
  };
  expect("null dsm", horizon_(nullptr, 3, 4, good_dirs, 2, 0, inf, inf, horizon), SNERF_ERR_NULL, "null");
  expect("null dirs", horizon_(dsm, 3, 4, nullptr, 2, 0, inf, inf, horizon), SNERF_ERR_NULL, "null");
  expect("null out", horizon_(dsm, 3, 4, good_dirs, 2, 0, inf, inf, nullptr), SNERF_ERR_NULL, "null");
  expect("h = 0", horizon_(dsm, 0, 4, good_dirs, 2, 0, inf, inf, horizon), SNERF_ERR_BAD_DESC, "h = 0");
  expect("w = -1", horizon_(dsm, 3, -1, good_dirs, 2, 0, inf, inf, horizon), SNERF_ERR_BAD_DESC, "w = -1");
  expect("2^31 cells", horizon_(dsm, 1 << 16, 1 << 15, good_dirs, 2, 0, inf, inf, horizon), SNERF_ERR_BAD_DESC, "2^31");
  expect("n_dirs = 0", horizon_(dsm, 3, 4, good_dirs, 0, 0, inf, inf, horizon), SNERF_ERR_BAD_DESC, "n_dirs = 0");
  expect("n_dirs = 65", horizon_(dsm, 3, 4, good_dirs, 65, 0, inf, inf, horizon), SNERF_ERR_BAD_DESC, "n_dirs = 65");
  expect("bias = inf", horizon_(dsm, 3, 4, good_dirs, 2, inf, inf, inf, horizon), SNERF_ERR_BAD_DESC, "bias");
  expect("bias = NaN", horizon_(dsm, 3, 4, good_dirs, 2, NAN, inf, inf, horizon), SNERF_ERR_BAD_DESC, "bias");
  expect("z_top = NaN", horizon_(dsm, 3, 4, good_dirs, 2, 0, NAN, inf, horizon), SNERF_ERR_BAD_DESC, "z_top");
  expect("max_dist = 0", horizon_(dsm, 3, 4, good_dirs, 2, 0, inf, 0.0, horizon), SNERF_ERR_BAD_DESC, "max_dist");
  expect("max_dist = -2", horizon_(dsm, 3, 4, good_dirs, 2, 0, inf, -2.0, horizon), SNERF_ERR_BAD_DESC, "max_dist");
  expect("max_dist = NaN", horizon_(dsm, 3, 4, good_dirs, 2, 0, inf, NAN, horizon), SNERF_ERR_BAD_DESC, "max_dist");
  expect("ux = NaN", horizon_(dsm, 3, 4, bad_dir(2, NAN), 2, 0, inf, inf, horizon), SNERF_ERR_BAD_DESC, "direction 1 is not finite");
  expect("uy = inf", horizon_(dsm, 3, 4, bad_dir(3, inf), 2, 0, inf, inf, horizon), SNERF_ERR_BAD_DESC, "direction 1 is not finite");
  expect("not a unit vector", horizon_(dsm, 3, 4, bad_dir(0, 1.0 + 1e-8), 2, 0, inf, inf, horizon), SNERF_ERR_BAD_DESC,
         "direction 0: (ux, uy)");

  g_prefix = "snerf_solar_svf: ";
  expect("null horizon", snerf_solar_svf(nullptr, 2, 3, 4, 0.5, svf, nullptr), SNERF_ERR_NULL, "null");
  expect("null out", snerf_solar_svf(horizon, 2, 3, 4, 0.5, nullptr, nullptr), SNERF_ERR_NULL, "null");
  expect("h = -3", snerf_solar_svf(horizon, 2, -3, 4, 0.5, svf, nullptr), SNERF_ERR_BAD_DESC, "h = -3");
  expect("2^31 cells", snerf_solar_svf(horizon, 2, 1 << 15, 1 << 16, 0.5, svf, nullptr), SNERF_ERR_BAD_DESC, "2^31");
  expect("n_dirs = 0", snerf_solar_svf(horizon, 0, 3, 4, 0.5, svf, nullptr), SNERF_ERR_BAD_DESC, "n_dirs = 0");
  expect("n_dirs = 721", snerf_solar_svf(horizon, 721, 3, 4, 0.5, svf, nullptr), SNERF_ERR_BAD_DESC, "n_dirs = 721");
  expect("res = 0", snerf_solar_svf(horizon, 2, 3, 4, 0.0, svf, nullptr), SNERF_ERR_BAD_DESC, "res > 0");
  expect("res = inf", snerf_solar_svf(horizon, 2, 3, 4, inf, svf, nullptr), SNERF_ERR_BAD_DESC, "res > 0");
  expect("res = NaN", snerf_solar_svf(horizon, 2, 3, 4, NAN, svf, nullptr), SNERF_ERR_BAD_DESC, "res > 0");

  g_prefix = "snerf_solar_irradiate: ";
  auto irr = [&](const float* H, int n_dirs, int h, int w, const float* se, const float* sn, const double* rows, int n, double* d,
                 unsigned int* c) { return snerf_solar_irradiate(H, n_dirs, h, w, se, sn, rows, n, d, c, nullptr); };
  auto bad_sun = [&](int at, double v) {
    static double rows[14];
    memcpy(rows, good_suns, sizeof rows);
    rows[at] = v;
    return rows;
  };
  expect("null horizon", irr(nullptr, 2, 3, 4, slope_e, slope_n, good_suns, 2, direct, count), SNERF_ERR_NULL, "null");
  expect("null suns", irr(horizon, 2, 3, 4, slope_e, slope_n, nullptr, 2, direct, count), SNERF_ERR_NULL, "null");
  expect("null direct", irr(horizon, 2, 3, 4, slope_e, slope_n, good_suns, 2, nullptr, count), SNERF_ERR_NULL, "null");
  expect("null count", irr(horizon, 2, 3, 4, slope_e, slope_n, good_suns, 2, direct, nullptr), SNERF_ERR_NULL, "null");
  expect("slope_e alone", irr(horizon, 2, 3, 4, slope_e, nullptr, good_suns, 2, direct, count), SNERF_ERR_NULL, "both null or both set");
  expect("slope_n alone", irr(horizon, 2, 3, 4, nullptr, slope_n, good_suns, 2, direct, count), SNERF_ERR_NULL, "both null or both set");
  expect("w = 0", irr(horizon, 2, 3, 0, nullptr, nullptr, good_suns, 2, direct, count), SNERF_ERR_BAD_DESC, "w = 0");
  expect("n_dirs = 0", irr(horizon, 0, 3, 4, nullptr, nullptr, good_suns, 2, direct, count), SNERF_ERR_BAD_DESC, "n_dirs = 0");
  expect("n_dirs = 721", irr(horizon, 721, 3, 4, nullptr, nullptr, good_suns, 2, direct, count), SNERF_ERR_BAD_DESC, "n_dirs = 721");
  expect("n_suns = 0", irr(horizon, 2, 3, 4, nullptr, nullptr, good_suns, 0, direct, count), SNERF_ERR_BAD_DESC, "n_suns = 0");
  expect("n_suns = 65", irr(horizon, 2, 3, 4, nullptr, nullptr, good_suns, 65, direct, count), SNERF_ERR_BAD_DESC, "n_suns = 65");
  expect("weight = NaN", irr(horizon, 2, 3, 4, nullptr, nullptr, bad_sun(13, NAN), 2, direct, count), SNERF_ERR_BAD_DESC, "sun 1 is not finite");
  expect("rise = inf", irr(horizon, 2, 3, 4, nullptr, nullptr, bad_sun(2, inf), 2, direct, count), SNERF_ERR_BAD_DESC, "sun 0 is not finite");
  expect("sector = 2", irr(horizon, 2, 3, 4, nullptr, nullptr, bad_sun(7, 2.0), 2, direct, count), SNERF_ERR_BAD_DESC, "sun 1: sector");
  expect("sector = -1", irr(horizon, 2, 3, 4, nullptr, nullptr, bad_sun(0, -1.0), 2, direct, count), SNERF_ERR_BAD_DESC, "sun 0: sector");
  expect("sector = 0.5", irr(horizon, 2, 3, 4, nullptr, nullptr, bad_sun(0, 0.5), 2, direct, count), SNERF_ERR_BAD_DESC, "sun 0: sector");
  expect("sector = 1e300", irr(horizon, 2, 3, 4, nullptr, nullptr, bad_sun(0, 1e300), 2, direct, count), SNERF_ERR_BAD_DESC, "sun 0: sector");
  expect("frac = 1", irr(horizon, 2, 3, 4, nullptr, nullptr, bad_sun(8, 1.0), 2, direct, count), SNERF_ERR_BAD_DESC, "sun 1: frac");
  expect("frac = -0.1", irr(horizon, 2, 3, 4, nullptr, nullptr, bad_sun(1, -0.1), 2, direct, count), SNERF_ERR_BAD_DESC, "sun 0: frac");
  expect("rise = 0", irr(horizon, 2, 3, 4, nullptr, nullptr, bad_sun(2, 0.0), 2, direct, count), SNERF_ERR_BAD_DESC, "sun 0: rise");
  expect("not a unit vector", irr(horizon, 2, 3, 4, nullptr, nullptr, bad_sun(4, 0.61), 2, direct, count), SNERF_ERR_BAD_DESC,
         "sun 0: (east, north, up)");
  expect("up = 0", irr(horizon, 2, 3, 4, nullptr, nullptr, bad_sun(12, -0.8), 2, direct, count), SNERF_ERR_BAD_DESC, "sun 1: up");
  expect("weight = -1", irr(horizon, 2, 3, 4, nullptr, nullptr, bad_sun(6, -1.0), 2, direct, count), SNERF_ERR_BAD_DESC, "sun 0: weight");

  for (int k = 0; k < 24; ++k)
    if (horizon[k] != 0.f || (k < 12 && (svf[k] != 0.f || direct[k] != 0.0 || count[k]))) {
      printf("outputs were written\n");
      ++failures;
      break;
    }
  return verdict("solar");
}
