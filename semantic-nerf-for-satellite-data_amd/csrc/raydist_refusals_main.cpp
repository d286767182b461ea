// Stand-alone host program over the refusal paths of snerf_ray_distortion (raydist.hip): every call below is refused by the argument
// checks, so no kernel launch is reached and no GPU is needed.  Built with ASAN + UBSAN on the host code
// (`make raydist-refusals`); exits 0 when every call came back with the expected code and message.  CPU machines only.
#include "../../include/snerf_raydist.h"

#include <cstdarg>
#include <cstdio>
#include <cstring>

static char g_error[512];

namespace snerf {
// the library's set_error (api.hip), which this program does not link
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_error, sizeof g_error, fmt, ap);
  va_end(ap);
}
}  // namespace snerf

static int failures = 0;

static void expect(const char* what, int rc, int want, const char* needle) {
  const bool ok = rc == want && strstr(g_error, needle) != nullptr && strstr(g_error, "snerf_ray_distortion: ") == g_error;
  printf("%-44s rc = %d  \"%s\"%s\n", what, rc, g_error, ok ? "" : "   <-- UNEXPECTED");
  if (!ok) ++failures;
  g_error[0] = 0;
}

int main() {
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
  printf("%s\n", failures ? "raydist refusals: FAILED" : "raydist refusals: ok");
  return failures ? 1 : 0;
}
