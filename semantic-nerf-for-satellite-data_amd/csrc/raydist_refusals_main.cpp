// The refusal paths of snerf_ray_distortion (raydist.hip): see refusals_main.h.
#include "refusals_main.h"

int main() {
  g_prefix = "snerf_ray_distortion: ";
  // never dereferenced as device memory: every call is refused before a launch
  static float w[12], z[12], rays[16], dw[12];
  static double per_ray[2];
  static unsigned long long acc[4];

  expect("null weights", snerf_ray_distortion(nullptr, z, rays, 8, 2, 6, dw, per_ray, acc, nullptr), SNERF_ERR_NULL, "weights is NULL");
  expect("null z_vals", snerf_ray_distortion(w, nullptr, rays, 8, 2, 6, dw, per_ray, acc, nullptr), SNERF_ERR_NULL, "z_vals is NULL");
  expect("null rays", snerf_ray_distortion(w, z, nullptr, 8, 2, 6, dw, per_ray, acc, nullptr), SNERF_ERR_NULL, "rays is NULL");
  expect("null d_weights", snerf_ray_distortion(w, z, rays, 8, 2, 6, nullptr, per_ray, acc, nullptr), SNERF_ERR_NULL, "d_weights is NULL");
  expect("null acc", snerf_ray_distortion(w, z, rays, 8, 2, 6, dw, per_ray, nullptr, nullptr), SNERF_ERR_NULL, "acc is NULL");
  expect("null acc, per_ray too", snerf_ray_distortion(w, z, rays, 8, 2, 6, dw, nullptr, nullptr, nullptr), SNERF_ERR_NULL, "acc is NULL");
  expect("n_rays = 0", snerf_ray_distortion(w, z, rays, 8, 0, 6, dw, per_ray, acc, nullptr), SNERF_ERR_BAD_DESC, "n_rays = 0");
  expect("n_rays = -7", snerf_ray_distortion(w, z, rays, 8, -7, 6, dw, per_ray, acc, nullptr), SNERF_ERR_BAD_DESC, "n_rays = -7");
  expect("n_rays = 2^22 + 1", snerf_ray_distortion(w, z, rays, 8, 4194305, 6, dw, per_ray, acc, nullptr), SNERF_ERR_BAD_DESC,
         "n_rays = 4194305");
  expect("n_rays = 2^31 - 1", snerf_ray_distortion(w, z, rays, 8, 2147483647, 6, dw, per_ray, acc, nullptr), SNERF_ERR_BAD_DESC,
         "n_rays = 2147483647");
  expect("n_samples = 0", snerf_ray_distortion(w, z, rays, 8, 2, 0, dw, per_ray, acc, nullptr), SNERF_ERR_BAD_DESC, "n_samples = 0");
  expect("n_samples = -1", snerf_ray_distortion(w, z, rays, 8, 2, -1, dw, per_ray, acc, nullptr), SNERF_ERR_BAD_DESC, "n_samples = -1");
  expect("n_samples = 1025", snerf_ray_distortion(w, z, rays, 8, 2, 1025, dw, per_ray, acc, nullptr), SNERF_ERR_BAD_DESC,
         "n_samples = 1025");
  expect("ray_stride = 7", snerf_ray_distortion(w, z, rays, 7, 2, 6, dw, per_ray, acc, nullptr), SNERF_ERR_BAD_DESC, "ray_stride = 7");
  expect("ray_stride = -8", snerf_ray_distortion(w, z, rays, -8, 2, 6, dw, per_ray, acc, nullptr), SNERF_ERR_BAD_DESC, "ray_stride = -8");

  for (int k = 0; k < 12; ++k) if (dw[k] != 0.f) { printf("d_weights was written\n"); ++failures; break; }
  for (int k = 0; k < 2; ++k) if (per_ray[k] != 0.0) { printf("per_ray was written\n"); ++failures; break; }
  for (int k = 0; k < 4; ++k) if (acc[k] != 0ull) { printf("acc was written\n"); ++failures; break; }
  return verdict("raydist");
}
