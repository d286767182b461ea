// Stand-alone host program over the refusal paths of snerf_resample_z (resample.hip): every call below is refused by the argument
// checks, so no kernel launch is reached and no GPU is needed.  Built with ASAN + UBSAN on the host code
// (`make resample-refusals`); exits 0 when every call came back with the expected code and message.  CPU machines only.
#include "../../include/snerf_resample.h"

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
  const bool ok = rc == want && strstr(g_error, needle) != nullptr && strstr(g_error, "snerf_resample_z: ") == g_error;
  printf("%-44s rc = %d  \"%s\"%s\n", what, rc, g_error, ok ? "" : "   <-- UNEXPECTED");
  if (!ok) ++failures;
  g_error[0] = 0;
}

int main() {
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
  printf("%s\n", failures ? "resample refusals: FAILED" : "resample refusals: ok");
  return failures ? 1 : 0;
}
