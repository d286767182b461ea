// The density-gradient pass (include/snerf_normals.h): what bsp_pass.hip's launch sequence and normals.hip's kernels share.
#pragma once
#include "common.h"
#include "plan.h"

namespace snerf {

// One encoding-gradient launch: a layer that reads the encoding, while its dz is live.
struct EncGradArgs {
  const char* dz = nullptr; const int* Edz = nullptr; int ld_dz = 0;   // d(pre-activation) of the layer: two-plane tensor [P][W]
  const char* pe = nullptr; const int* Epe = nullptr; int Ep = 0;      // the stored encoding: two-plane tensor [P][Ep]
  const double* wd = nullptr; int ldw = 0;                             // fp64 copy of the layer's encoding columns [W][ldw], zero beyond column E
  double* G = nullptr;                                                 // [P][3]
  int P = 0, W = 0, F = 0;                                             // F = 0: identity encoding (3 columns)
  int first = 0;                                                       // store (the first launch of a pass) or add
};

// The scratch buffer of snerf_density_grad, byte offsets (256-byte aligned regions)
struct NormalsScratch { size_t o_G = 0, o_wd = 0, o_part = 0, bytes = 0; int ldw = 0; };
NormalsScratch normals_scratch(const Plan& p);

int launch_encgrad_weights(const float* w, int ld, int W, int E, double* wd, int ldw, hipStream_t st);   // wd[j][e] = (double)w[j][e], 0.0 for e >= E
int launch_encgrad(const EncGradArgs& a, hipStream_t st);
int launch_ray_fold3(const double* G, int N, int S, double* grad_ray, float* grad_sample, hipStream_t st);
void encgrad_set_grid_override(int n);
// test hook: device buffers every pass also decodes its encoding-gradient operands into (null: off)
struct NormalsDump { float* dz = nullptr; float* enc = nullptr; };
NormalsDump normals_dump();

// bsp_pass.hip: the launch sequence
int density_grad_bsp(const Plan& p, const float* pk, const SnerfInputs* in, const float* coef, double* grad_ray, float* grad_sample,
                     void* workspace, void* scratch, hipStream_t st);

}  // namespace snerf
