// The refusal paths of snerf_shadow_cast / snerf_shadow_agreement (shadow.hip): see refusals_main.h.
#include "refusals_main.h"

int main() {
  // never dereferenced as device memory: every call is refused before a launch
  static float dsm[12], sun[12], dist[12];
  static unsigned char lit[12], valid[12];
  static unsigned long long acc[8];
  const double s2 = std::sqrt(0.5);
  const double good[6] = {1.0, 0.0, 0.5, s2, -s2, 0.25};
  const double inf = INFINITY;

  expect("cast, null dsm", snerf_shadow_cast(nullptr, 3, 4, good, 2, 0.0, inf, lit, dist, nullptr), SNERF_ERR_NULL, "null");
  expect("cast, null suns", snerf_shadow_cast(dsm, 3, 4, nullptr, 2, 0.0, inf, lit, dist, nullptr), SNERF_ERR_NULL, "null");
  expect("cast, null lit_out", snerf_shadow_cast(dsm, 3, 4, good, 2, 0.0, inf, nullptr, dist, nullptr), SNERF_ERR_NULL, "null");
  expect("cast, h = 0", snerf_shadow_cast(dsm, 0, 4, good, 2, 0.0, inf, lit, nullptr, nullptr), SNERF_ERR_BAD_DESC, "h = 0");
  expect("cast, w = -1", snerf_shadow_cast(dsm, 3, -1, good, 2, 0.0, inf, lit, nullptr, nullptr), SNERF_ERR_BAD_DESC, "w = -1");
  expect("cast, h * w = 2^31", snerf_shadow_cast(dsm, 1 << 16, 1 << 15, good, 2, 0.0, inf, lit, nullptr, nullptr), SNERF_ERR_BAD_DESC, "2^31");
  expect("cast, n_suns = 0", snerf_shadow_cast(dsm, 3, 4, good, 0, 0.0, inf, lit, nullptr, nullptr), SNERF_ERR_BAD_DESC, "n_suns = 0");
  expect("cast, n_suns = 65", snerf_shadow_cast(dsm, 3, 4, good, 65, 0.0, inf, lit, nullptr, nullptr), SNERF_ERR_BAD_DESC, "n_suns = 65");
  expect("cast, bias = inf", snerf_shadow_cast(dsm, 3, 4, good, 2, inf, inf, lit, nullptr, nullptr), SNERF_ERR_BAD_DESC, "bias");
  expect("cast, bias = NaN", snerf_shadow_cast(dsm, 3, 4, good, 2, NAN, inf, lit, nullptr, nullptr), SNERF_ERR_BAD_DESC, "bias");
  expect("cast, z_top = NaN", snerf_shadow_cast(dsm, 3, 4, good, 2, 0.0, NAN, lit, nullptr, nullptr), SNERF_ERR_BAD_DESC, "z_top");
  for (int col = 0; col < 3; ++col) {
    double rows[6];
    memcpy(rows, good, sizeof rows);
    rows[3 + col] = col == 2 ? inf : NAN;
    expect("cast, a sun value not finite", snerf_shadow_cast(dsm, 3, 4, rows, 2, 0.0, inf, lit, nullptr, nullptr), SNERF_ERR_BAD_DESC, "sun 1 is not finite");
  }
  {
    double rows[6];
    memcpy(rows, good, sizeof rows);
    rows[0] = 1.0 + 1e-8;
    expect("cast, |(ux, uy)| off by 2e-8", snerf_shadow_cast(dsm, 3, 4, rows, 2, 0.0, inf, lit, nullptr, nullptr), SNERF_ERR_BAD_DESC, "sun 0: (ux, uy)");
    memcpy(rows, good, sizeof rows);
    rows[3] = rows[4] = 0.0;
    expect("cast, (ux, uy) = 0", snerf_shadow_cast(dsm, 3, 4, rows, 2, 0.0, inf, lit, nullptr, nullptr), SNERF_ERR_BAD_DESC, "sun 1: (ux, uy)");
    memcpy(rows, good, sizeof rows);
    rows[5] = 0.0;
    expect("cast, rise = 0", snerf_shadow_cast(dsm, 3, 4, rows, 2, 0.0, inf, lit, nullptr, nullptr), SNERF_ERR_BAD_DESC, "sun 1: rise");
    rows[5] = -0.25;
    expect("cast, rise < 0", snerf_shadow_cast(dsm, 3, 4, rows, 2, 0.0, inf, lit, nullptr, nullptr), SNERF_ERR_BAD_DESC, "sun 1: rise");
  }

  expect("agreement, null sun", snerf_shadow_agreement(nullptr, lit, valid, 12, 1, 0.5, acc, nullptr), SNERF_ERR_NULL, "null");
  expect("agreement, null lit", snerf_shadow_agreement(sun, nullptr, valid, 12, 1, 0.5, acc, nullptr), SNERF_ERR_NULL, "null");
  expect("agreement, null acc", snerf_shadow_agreement(sun, lit, nullptr, 12, 1, 0.5, nullptr, nullptr), SNERF_ERR_NULL, "null");
  expect("agreement, cells = 0", snerf_shadow_agreement(sun, lit, nullptr, 0, 1, 0.5, acc, nullptr), SNERF_ERR_BAD_DESC, "cells");
  expect("agreement, cells = -3", snerf_shadow_agreement(sun, lit, nullptr, -3, 1, 0.5, acc, nullptr), SNERF_ERR_BAD_DESC, "cells");
  expect("agreement, n_suns = 0", snerf_shadow_agreement(sun, lit, nullptr, 12, 0, 0.5, acc, nullptr), SNERF_ERR_BAD_DESC, "n_suns = 0");
  expect("agreement, n_suns = 65", snerf_shadow_agreement(sun, lit, nullptr, 12, 65, 0.5, acc, nullptr), SNERF_ERR_BAD_DESC, "n_suns = 65");
  expect("agreement, threshold = NaN", snerf_shadow_agreement(sun, lit, nullptr, 12, 1, NAN, acc, nullptr), SNERF_ERR_BAD_DESC, "threshold");
  expect("agreement, threshold = inf", snerf_shadow_agreement(sun, lit, nullptr, 12, 1, inf, acc, nullptr), SNERF_ERR_BAD_DESC, "threshold");

  for (int k = 0; k < 8; ++k) if (acc[k]) { printf("acc was written\n"); ++failures; break; }
  for (int k = 0; k < 12; ++k) if (lit[k] || dist[k] != 0.f) { printf("outputs were written\n"); ++failures; break; }
  return verdict("shadow");
}
