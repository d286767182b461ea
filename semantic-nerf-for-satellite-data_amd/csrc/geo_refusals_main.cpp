// The refusal paths of snerf_geo_cloud / snerf_geo_points (geo.hip geo_launch): see refusals_main.h.
#include "refusals_main.h"

int main() {
  what_width = 52;
  // never dereferenced: every call is refused before a launch
  static double points[24], out[24], lla[24];
  static float rays[64], depth[8];
  unsigned long long stats[8] = {~0ull, 0, ~0ull, 0, 0, 0, 0, 0};
  const SnerfGeoParams good = {{795629.9, -5453830.0, 3199137.0}, 58.875, -1.413716694115407, 0, SNERF_GEO_TO_WORLD};
  SnerfGeoParams p = good;

  p.direction = 2;
  expect("points, direction = 2", snerf_geo_points(points, 8, &p, out, lla, stats, nullptr), SNERF_ERR_BAD_DESC, "direction = 2");
  expect("points, direction = 2, n = 0", snerf_geo_points(points, 0, &p, out, lla, stats, nullptr), SNERF_ERR_BAD_DESC, "direction");
  expect("cloud, direction = 2", snerf_geo_cloud(rays, 8, depth, 8, &p, out, lla, stats, nullptr), SNERF_ERR_BAD_DESC, "direction = 2");
  p.direction = -1;
  expect("points, direction = -1", snerf_geo_points(points, 8, &p, out, lla, stats, nullptr), SNERF_ERR_BAD_DESC, "direction = -1");
  p.direction = SNERF_GEO_TO_SCENE;
  expect("cloud, direction = 1", snerf_geo_cloud(rays, 8, depth, 8, &p, out, lla, stats, nullptr), SNERF_ERR_BAD_DESC, "direction = 1");
  expect("cloud, direction = 1, n = 0", snerf_geo_cloud(rays, 8, depth, 0, &p, out, lla, stats, nullptr), SNERF_ERR_BAD_DESC, "direction");

  for (int direction = 0; direction < 2; ++direction) {
    p = good;
    p.direction = direction;
    expect("points, null input", snerf_geo_points(nullptr, 8, &p, out, lla, stats, nullptr), SNERF_ERR_NULL, "null");
    expect("points, null params", snerf_geo_points(points, 8, nullptr, out, lla, stats, nullptr), SNERF_ERR_NULL, "null");
    expect("points, null stats", snerf_geo_points(points, 8, &p, out, lla, nullptr, nullptr), SNERF_ERR_NULL, "null");
    expect("points, null output", snerf_geo_points(points, 8, &p, nullptr, lla, stats, nullptr), SNERF_ERR_NULL, "null");
    expect("points, n = -1", snerf_geo_points(points, -1, &p, out, lla, stats, nullptr), SNERF_ERR_BAD_DESC, "n = -1");
    expect("points, n = 2^31 + 1", snerf_geo_points(points, (1ll << 31) + 1, &p, out, lla, stats, nullptr), SNERF_ERR_BAD_DESC, "outside");
    p.range = 0.0;
    expect("points, range = 0", snerf_geo_points(points, 8, &p, out, lla, stats, nullptr), SNERF_ERR_BAD_DESC, "range");
    p.range = NAN;
    expect("points, range = NaN", snerf_geo_points(points, 8, &p, out, lla, stats, nullptr), SNERF_ERR_BAD_DESC, "range");
    p = good;
    p.direction = direction;
    p.centre[1] = INFINITY;
    expect("points, centre[1] = inf", snerf_geo_points(points, 8, &p, out, lla, stats, nullptr), SNERF_ERR_BAD_DESC, "centre[1]");
    p = good;
    p.direction = direction;
    p.lon0 = 3.2;
    expect("points, lon0 = 3.2", snerf_geo_points(points, 8, &p, out, lla, stats, nullptr), SNERF_ERR_BAD_DESC, "meridian");
    p = good;
    p.direction = direction;
    p.south = 2;
    expect("points, south = 2", snerf_geo_points(points, 8, &p, out, lla, stats, nullptr), SNERF_ERR_BAD_DESC, "south = 2");
    p = good;
    p.direction = direction;
    expect("points, n = 0", snerf_geo_points(nullptr, 0, &p, nullptr, nullptr, stats, nullptr), SNERF_OK, nullptr);
  }
  p = good;
  expect("cloud, ray_stride = 5", snerf_geo_cloud(rays, 5, depth, 8, &p, out, lla, stats, nullptr), SNERF_ERR_BAD_DESC, "ray_stride");
  expect("cloud, null rays", snerf_geo_cloud(nullptr, 8, depth, 8, &p, out, lla, stats, nullptr), SNERF_ERR_NULL, "null");
  expect("cloud, null depth", snerf_geo_cloud(rays, 8, nullptr, 8, &p, out, lla, stats, nullptr), SNERF_ERR_NULL, "null");
  expect("cloud, n = 0", snerf_geo_cloud(nullptr, 8, nullptr, 0, &p, nullptr, nullptr, stats, nullptr), SNERF_OK, nullptr);

  const unsigned long long init[8] = {~0ull, 0, ~0ull, 0, 0, 0, 0, 0};
  if (memcmp(stats, init, sizeof init) != 0) { printf("stats were written\n"); ++failures; }
  for (int k = 0; k < 24; ++k) if (out[k] != 0.0 || lla[k] != 0.0) { printf("outputs were written\n"); ++failures; break; }
  return verdict("geo");
}
