// The refusal paths of snerf_dsm_segment_hit (raycast.hip): see refusals_main.h.
#include "refusals_main.h"
#include "../../include/snerf_raycast.h"

static SnerfDsmGrid grid_of(double res, int xsize, int ysize, int ioff, int joff, int out_w, int out_h) {
  SnerfDsmGrid g = {1000.0, 2000.0, res, xsize, ysize, ioff, joff, out_w, out_h};
  return g;
}

int main() {
  g_prefix = "snerf_dsm_segment_hit: ";
  // never dereferenced as device memory: every call is refused before a launch
  static double p0[6], p1[6], s[2];
  static float dsm[12];
  static unsigned char state[2];
  static int cell[2];
  const SnerfDsmGrid good = grid_of(0.5, 4, 3, 0, 0, 4, 3);

  expect("null p0", snerf_dsm_segment_hit(nullptr, p1, 2, &good, dsm, 0.0, s, state, cell, nullptr), SNERF_ERR_NULL, "null");
  expect("null p1", snerf_dsm_segment_hit(p0, nullptr, 2, &good, dsm, 0.0, s, state, cell, nullptr), SNERF_ERR_NULL, "null");
  expect("null grid", snerf_dsm_segment_hit(p0, p1, 2, nullptr, dsm, 0.0, s, state, cell, nullptr), SNERF_ERR_NULL, "null");
  expect("null dsm", snerf_dsm_segment_hit(p0, p1, 2, &good, nullptr, 0.0, s, state, cell, nullptr), SNERF_ERR_NULL, "null");
  expect("null s_out", snerf_dsm_segment_hit(p0, p1, 2, &good, dsm, 0.0, nullptr, state, cell, nullptr), SNERF_ERR_NULL, "null");
  expect("null state_out", snerf_dsm_segment_hit(p0, p1, 2, &good, dsm, 0.0, s, nullptr, nullptr, nullptr), SNERF_ERR_NULL, "null");
  expect("n = -1", snerf_dsm_segment_hit(p0, p1, -1, &good, dsm, 0.0, s, state, cell, nullptr), SNERF_ERR_BAD_DESC, "n = -1");
  expect("n = 2^31 + 1", snerf_dsm_segment_hit(p0, p1, 2147483649LL, &good, dsm, 0.0, s, state, cell, nullptr), SNERF_ERR_BAD_DESC,
         "n = 2147483649");
  {
    SnerfDsmGrid g = grid_of(0.0, 4, 3, 0, 0, 4, 3);
    expect("res = 0", snerf_dsm_segment_hit(p0, p1, 2, &g, dsm, 0.0, s, state, cell, nullptr), SNERF_ERR_BAD_DESC, "res > 0");
    g = grid_of(NAN, 4, 3, 0, 0, 4, 3);
    expect("res = NaN", snerf_dsm_segment_hit(p0, p1, 2, &g, dsm, 0.0, s, state, cell, nullptr), SNERF_ERR_BAD_DESC, "res > 0");
    g = grid_of(-0.5, 4, 3, 0, 0, 4, 3);
    expect("res < 0", snerf_dsm_segment_hit(p0, p1, 2, &g, dsm, 0.0, s, state, cell, nullptr), SNERF_ERR_BAD_DESC, "res > 0");
    g = grid_of(0.5, 4, 3, 0, 0, 4, 0);
    expect("out_h = 0", snerf_dsm_segment_hit(p0, p1, 2, &g, dsm, 0.0, s, state, cell, nullptr), SNERF_ERR_BAD_DESC, "positive sizes");
    g = grid_of(0.5, 4, 3, 0, 0, -4, 3);
    expect("out_w = -4", snerf_dsm_segment_hit(p0, p1, 2, &g, dsm, 0.0, s, state, cell, nullptr), SNERF_ERR_BAD_DESC, "positive sizes");
    g = grid_of(0.5, 0, 3, 0, 0, 4, 3);
    expect("xsize = 0", snerf_dsm_segment_hit(p0, p1, 2, &g, dsm, 0.0, s, state, cell, nullptr), SNERF_ERR_BAD_DESC, "positive sizes");
    g = grid_of(0.5, 4, 3, 0, 2147483645, 4, 3);
    expect("joff + out_h > int32", snerf_dsm_segment_hit(p0, p1, 2, &g, dsm, 0.0, s, state, cell, nullptr), SNERF_ERR_BAD_DESC, "int32");
    g = grid_of(0.5, 4, 3, 2147483644, 0, 4, 3);
    expect("ioff + out_w > int32", snerf_dsm_segment_hit(p0, p1, 2, &g, dsm, 0.0, s, state, cell, nullptr), SNERF_ERR_BAD_DESC, "int32");
    g = grid_of(0.5, 4, 3, 0, 0, 1 << 16, 1 << 15);
    expect("out_h * out_w = 2^31", snerf_dsm_segment_hit(p0, p1, 2, &g, dsm, 0.0, s, state, cell, nullptr), SNERF_ERR_BAD_DESC, "2^31");
    g = good;
    g.xoff = INFINITY;
    expect("xoff = inf", snerf_dsm_segment_hit(p0, p1, 2, &g, dsm, 0.0, s, state, cell, nullptr), SNERF_ERR_BAD_DESC, "res > 0");
  }
  expect("bias = inf", snerf_dsm_segment_hit(p0, p1, 2, &good, dsm, INFINITY, s, state, cell, nullptr), SNERF_ERR_BAD_DESC, "bias");
  expect("bias = NaN", snerf_dsm_segment_hit(p0, p1, 2, &good, dsm, NAN, s, state, cell, nullptr), SNERF_ERR_BAD_DESC, "bias");
  // n == 0 is accepted and launches nothing; a bad argument beside it is still refused
  expect("n = 0", snerf_dsm_segment_hit(p0, p1, 0, &good, dsm, 0.0, s, state, nullptr, nullptr), SNERF_OK, nullptr, nullptr);
  expect("n = 0, bias = NaN", snerf_dsm_segment_hit(p0, p1, 0, &good, dsm, NAN, s, state, cell, nullptr), SNERF_ERR_BAD_DESC, "bias");

  for (int k = 0; k < 2; ++k) if (s[k] != 0.0 || state[k] || cell[k]) { printf("outputs were written\n"); ++failures; break; }
  return verdict("raycast");
}
