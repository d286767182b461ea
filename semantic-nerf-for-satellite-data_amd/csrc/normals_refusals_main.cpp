// The refusal paths of snerf_density_grad and snerf_normals_scratch_bytes (normals.hip), as the programs of refusals_main.h: every call
// is refused by the host-side checks, so no launch is reached and no GPU is needed; built with ASAN + UBSAN on the host code
// (`make normals-refusals`), exits 0 when every call came back with the expected code and message.  CPU machines only.
// Unlike the other programs this one links the whole library: the entries plan through make_plan (api.hip) and queue through
// density_grad_bsp (bsp_pass.hip).  The messages therefore come through snerf_last_error(), not through a set_error of its own.
#include "../../include/snerf_normals.h"

#include <cstdio>
#include <cstring>

static int failures = 0;

static void expect(const char* what, int rc, int want, const char* needle, const char* prefix) {
  const char* msg = snerf_last_error();
  const bool ok = rc == want && strstr(msg, needle) != nullptr && strstr(msg, prefix) == msg;
  printf("%-44s rc = %d  \"%s\"%s\n", what, rc, msg, ok ? "" : "   <-- UNEXPECTED");
  if (!ok) ++failures;
}

static SnerfDesc desc(unsigned flags) {
  SnerfDesc d;
  memset(&d, 0, sizeof d);
  d.n_rays = 8; d.n_samples = 16; d.fc_units = 64; d.fc_layers = 8; d.feat_last = 32; d.skip_mask = 1u << 4;
  d.n_freq = 10; d.siren = 1; d.t_dim = 4; d.n_classes = 5; d.sem_sigmoid = 1; d.flags = flags;
  return d;
}

int main() {
  // never dereferenced as device memory: every call is refused before a launch
  alignas(256) static float packed[64], coef[128], ws[64], scratch[64], sun[24];
  static double grad_ray[24];
  SnerfInputs in;
  memset(&in, 0, sizeof in);
  in.sun_d = sun; in.sun_stride = 3;
  const char* who = "snerf_density_grad: ";
  SnerfDesc d = desc(SNERF_FLAG_TRAIN);

  expect("null desc", snerf_density_grad(nullptr, packed, &in, coef, grad_ray, nullptr, ws, scratch, nullptr), SNERF_ERR_NULL, "desc is NULL", who);
  expect("null packed_params", snerf_density_grad(&d, nullptr, &in, coef, grad_ray, nullptr, ws, scratch, nullptr), SNERF_ERR_NULL, "packed_params is NULL", who);
  expect("null inputs", snerf_density_grad(&d, packed, nullptr, coef, grad_ray, nullptr, ws, scratch, nullptr), SNERF_ERR_NULL, "inputs is NULL", who);
  expect("null coef", snerf_density_grad(&d, packed, &in, nullptr, grad_ray, nullptr, ws, scratch, nullptr), SNERF_ERR_NULL, "coef is NULL", who);
  expect("null grad_ray", snerf_density_grad(&d, packed, &in, coef, nullptr, nullptr, ws, scratch, nullptr), SNERF_ERR_NULL, "grad_ray is NULL", who);
  expect("null workspace", snerf_density_grad(&d, packed, &in, coef, grad_ray, nullptr, nullptr, scratch, nullptr), SNERF_ERR_NULL, "workspace is NULL", who);
  expect("null scratch", snerf_density_grad(&d, packed, &in, coef, grad_ray, nullptr, ws, nullptr, nullptr), SNERF_ERR_NULL, "scratch is NULL", who);

  const struct { const char* what; unsigned flags; const char* needle; } flagged[] = {
      {"no SNERF_FLAG_TRAIN", 0u, "lacks SNERF_FLAG_TRAIN"},
      {"SNERF_FLAG_SC_PASS", SNERF_FLAG_TRAIN | SNERF_FLAG_SC_PASS, "SNERF_FLAG_SC_PASS is not a flag of this pass"},
      {"SNERF_FLAG_RELIGHT", SNERF_FLAG_TRAIN | SNERF_FLAG_RELIGHT, "SNERF_FLAG_RELIGHT is not a flag of this pass"},
      {"SNERF_FLAG_GEOMETRY", SNERF_FLAG_TRAIN | SNERF_FLAG_GEOMETRY, "SNERF_FLAG_GEOMETRY is not a flag of this pass"},
      {"SNERF_FLAG_EMBED_GRAD", SNERF_FLAG_TRAIN | SNERF_FLAG_EMBED_GRAD, "SNERF_FLAG_EMBED_GRAD is not a flag of this pass"},
      {"SNERF_FLAG_DEPTH_MEDIAN", SNERF_FLAG_TRAIN | SNERF_FLAG_DEPTH_MEDIAN, "SNERF_FLAG_DEPTH_MEDIAN is not a flag of this pass"},
      {"SNERF_FLAG_F16X1", SNERF_FLAG_TRAIN | SNERF_FLAG_F16X1, "SNERF_FLAG_F16X1 is not supported"}};
  for (const auto& f : flagged) {
    SnerfDesc e = desc(f.flags);
    expect(f.what, snerf_density_grad(&e, packed, &in, coef, grad_ray, nullptr, ws, scratch, nullptr), SNERF_ERR_BAD_DESC, f.needle, who);
    size_t n = 77;
    expect(f.what, snerf_normals_scratch_bytes(&e, &n), SNERF_ERR_BAD_DESC, f.needle, "snerf_normals_scratch_bytes: ");
    if (n != 77) { printf("bytes was written\n"); ++failures; }
  }

  { SnerfDesc e = d; e.n_rays = 0;
    expect("n_rays = 0", snerf_density_grad(&e, packed, &in, coef, grad_ray, nullptr, ws, scratch, nullptr), SNERF_ERR_BAD_DESC, "n_rays and n_samples must be positive", who); }
  { SnerfDesc e = d; e.n_rays = 1 << 20; e.n_samples = 1 << 11;
    expect("n_rays * n_samples = 2^31", snerf_density_grad(&e, packed, &in, coef, grad_ray, nullptr, ws, scratch, nullptr), SNERF_ERR_BAD_DESC, "too large for one pass", who); }
  { SnerfDesc e = d; e.fc_units = 40;
    expect("fc_units = 40", snerf_density_grad(&e, packed, &in, coef, grad_ray, nullptr, ws, scratch, nullptr), SNERF_ERR_BAD_DESC, "fc_units", who); }
  { SnerfDesc e = d; e.fc_layers = 17;
    expect("fc_layers = 17", snerf_density_grad(&e, packed, &in, coef, grad_ray, nullptr, ws, scratch, nullptr), SNERF_ERR_BAD_DESC, "fc_layers out of range", who); }
  { SnerfDesc e = d; e.n_freq = 17;
    expect("n_freq = 17", snerf_density_grad(&e, packed, &in, coef, grad_ray, nullptr, ws, scratch, nullptr), SNERF_ERR_BAD_DESC, "n_freq out of range", who); }
  { SnerfInputs nosun = in; nosun.sun_d = nullptr;
    expect("inputs without sun_d", snerf_density_grad(&d, packed, &nosun, coef, grad_ray, nullptr, ws, scratch, nullptr), SNERF_ERR_NULL, "inputs->sun_d", who); }
  expect("workspace off 256 bytes", snerf_density_grad(&d, packed, &in, coef, grad_ray, nullptr, ws + 1, scratch, nullptr), SNERF_ERR_WORKSPACE, "256-byte aligned", who);
  expect("scratch off 256 bytes", snerf_density_grad(&d, packed, &in, coef, grad_ray, nullptr, ws, scratch + 4, nullptr), SNERF_ERR_WORKSPACE, "256-byte aligned", who);
  expect("packed_params off 256 bytes", snerf_density_grad(&d, packed + 8, &in, coef, grad_ray, nullptr, ws, scratch, nullptr), SNERF_ERR_WORKSPACE, "256-byte aligned", who);

  size_t n = 0;
  expect("scratch_bytes: null desc", snerf_normals_scratch_bytes(nullptr, &n), SNERF_ERR_NULL, "desc is NULL", "snerf_normals_scratch_bytes: ");
  expect("scratch_bytes: null bytes", snerf_normals_scratch_bytes(&d, nullptr), SNERF_ERR_NULL, "bytes is NULL", "snerf_normals_scratch_bytes: ");
  const int rc = snerf_normals_scratch_bytes(&d, &n);
  printf("%-44s rc = %d  bytes = %zu%s\n", "scratch_bytes: 8 x 16, W = 64, F = 10", rc, n, (rc == SNERF_OK && n == 3072 + 30720 + 256) ? "" : "   <-- UNEXPECTED");
  if (rc != SNERF_OK || n != 3072 + 30720 + 256) ++failures;

  for (int k = 0; k < 24; ++k) if (grad_ray[k] != 0.0) { printf("grad_ray was written\n"); ++failures; break; }
  printf("normals refusals: %s\n", failures ? "FAILED" : "ok");
  return failures ? 1 : 0;
}
