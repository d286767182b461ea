// The refusal paths of snerf_resample_z (resample.hip): see refusals_main.h.
#include "refusals_main.h"

int main() {
  g_prefix = "snerf_resample_z: ";
  // never dereferenced as device memory: every call is refused before a launch
  static float z[12], w[12], u[8], out[20], fine[8];

  expect("null z", snerf_resample_z(nullptr, w, u, out, fine, 2, 6, 4, nullptr), SNERF_ERR_NULL, "z is NULL");
  expect("null weights", snerf_resample_z(z, nullptr, u, out, fine, 2, 6, 4, nullptr), SNERF_ERR_NULL, "weights is NULL");
  expect("null z_out", snerf_resample_z(z, w, u, nullptr, fine, 2, 6, 4, nullptr), SNERF_ERR_NULL, "z_out is NULL");
  expect("null z_out, u and z_fine too", snerf_resample_z(z, w, nullptr, nullptr, nullptr, 2, 6, 4, nullptr), SNERF_ERR_NULL, "z_out is NULL");
  expect("n_rays = 0", snerf_resample_z(z, w, u, out, fine, 0, 6, 4, nullptr), SNERF_ERR_BAD_DESC, "n_rays = 0");
  expect("n_rays = -7", snerf_resample_z(z, w, u, out, fine, -7, 6, 4, nullptr), SNERF_ERR_BAD_DESC, "n_rays = -7");
  expect("n_samples = 2", snerf_resample_z(z, w, u, out, fine, 2, 2, 4, nullptr), SNERF_ERR_BAD_DESC, "n_samples = 2");
  expect("n_samples = -1", snerf_resample_z(z, w, u, out, fine, 2, -1, 4, nullptr), SNERF_ERR_BAD_DESC, "n_samples = -1");
  expect("n_importance = 0", snerf_resample_z(z, w, u, out, fine, 2, 6, 0, nullptr), SNERF_ERR_BAD_DESC, "n_importance = 0");
  expect("n_importance = -3", snerf_resample_z(z, w, nullptr, out, nullptr, 2, 6, -3, nullptr), SNERF_ERR_BAD_DESC, "n_importance = -3");
  expect("n_samples + n_importance = 1025", snerf_resample_z(z, w, u, out, fine, 2, 512, 513, nullptr), SNERF_ERR_BAD_DESC,
         "n_samples + n_importance = 1025");
  expect("n_samples + n_importance = 2^32 - 2", snerf_resample_z(z, w, u, out, fine, 2, 2147483647, 2147483647, nullptr), SNERF_ERR_BAD_DESC,
         "n_samples + n_importance = 4294967294");

  for (int k = 0; k < 20; ++k) if (out[k] != 0.f) { printf("z_out was written\n"); ++failures; break; }
  for (int k = 0; k < 8; ++k) if (fine[k] != 0.f) { printf("z_fine was written\n"); ++failures; break; }
  return verdict("resample");
}
