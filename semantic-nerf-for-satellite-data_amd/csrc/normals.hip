// The gradient of the density with respect to the sample position (include/snerf_normals.h): the two kernels the
// pass adds to the launches it shares with snerf_backward (bsp_pass.hip: density_grad_bsp), and its entry points.  tests/normals_numpy.py
// restates both kernels operation for operation.
//   - encgrad_kernel: at a layer that reads the encoding, T = dz^T W[:, :E] per point and its contraction with the encoding's Jacobian
//     into three values.  ONE THREAD PER POINT: a point's sums are formed by one thread in an order that E and W alone fix (j ascending
//     in one accumulator per column, then k ascending), so no result depends on the grid.  The weights are wave-uniform: an fp64 copy of
//     the layer's encoding columns (launch_encgrad_weights, a few hundred KB) is read through the scalar cache and every fp64 FMA takes
//     its weight from scalar registers; the lanes stream their own rows of dz, 64 bytes at a time.  A product of two fp32 values is
//     exact in fp64, so the FMA rounds once, exactly as a separate multiply and add would: the FMA is used for its rate, not its
//     rounding.  The Jacobian comes from the stored encoding (d sin(f x) = f cos(f x), d cos(f x) = -f sin(f x), f = 2^k): no
//     transcendental.  Its products are not exact, so the tail is plain operators under `fp contract(off)`, one rounding each.
//   - ray_fold3_kernel: one wave per ray (ray_wave.h); the lanes load 64 samples at a time, every lane then adds them in ascending order.
//   - every store is a vector store (the only scalar memory instructions are the loads of the fp64 weights); no atomics, no LDS, no
//     allocation, no host synchronisation.
#include "normals.h"

#include <string.h>

#include "bsp.h"
#include "ray_wave.h"
#include "../../include/snerf_normals.h"

#pragma clang fp contract(off)

namespace snerf {

namespace {
int g_encgrad_grid = 0;
NormalsDump g_dump;

// element `col` of row `row` of a two-plane tensor as from_planes_kernel (bsp_aux.hip) decodes it
__device__ __forceinline__ float plane_elem(const char* row, int col, int e) {
  const char* p = row + bsp::g16_off(col, 2);
  const float hi = (float)*reinterpret_cast<const _Float16*>(p), lo = (float)*reinterpret_cast<const _Float16*>(p + 32);
  return __builtin_amdgcn_ldexpf(hi + lo, -e);
}
}  // namespace

void encgrad_set_grid_override(int n) { g_encgrad_grid = n > 0 ? n : 0; }
NormalsDump normals_dump() { return g_dump; }

// frequencies a chunk of the encoding-gradient kernel keeps accumulators for (6 each); 0: the identity encoding
static inline int encgrad_nf(int F) { return F == 0 ? 0 : (F <= 5 ? 5 : 10); }

NormalsScratch normals_scratch(const Plan& p) {
  NormalsScratch s;
  const int nf = encgrad_nf(p.F);
  s.ldw = nf ? round_up(6 * p.F, 6 * nf) : 4;
  size_t o = 0;
  auto take = [&](size_t bytes) { const size_t at = o; o += round_up_sz(bytes, 256); return at; };
  s.o_G = take((size_t)p.P * 3 * sizeof(double));
  s.o_wd = take((size_t)p.W * s.ldw * sizeof(double));
  s.o_part = take((size_t)((p.P + 255) / 256) * NARROW * sizeof(float));
  s.bytes = o;
  return s;
}

__global__ __launch_bounds__(256) void encgrad_weights_kernel(const float* __restrict__ w, int ld, int W, int E, double* __restrict__ wd, int ldw) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= W * ldw) return;
  const int j = i / ldw, e = i - j * ldw;
  wd[i] = e < E ? (double)w[(size_t)j * ld + e] : 0.0;
}

int launch_encgrad_weights(const float* w, int ld, int W, int E, double* wd, int ldw, hipStream_t st) {
  hipLaunchKernelGGL(encgrad_weights_kernel, dim3((unsigned)((W * ldw + 255) / 256)), dim3(256), 0, st, w, ld, W, E, wd, ldw);
  SNERF_LAUNCH_CHECK();
  return SNERF_OK;
}

template <int NF>
__global__ __launch_bounds__(256) void encgrad_kernel(const EncGradArgs a) {
  constexpr int EC = NF > 0 ? 6 * NF : 3;
  const int nblk = (a.P + 255) / 256, ncb = bsp::ncb_of(a.ld_dz);
  const int nchunk = NF > 0 ? (a.F + NF - 1) / NF : 1;
  // the fp64 weights through the constant address space: written by an earlier launch, never by this one, and addressed by
  // workgroup-uniform indices only, so every load of them is a scalar load
  typedef const double __attribute__((address_space(4))) cdouble;
  cdouble* wd = (cdouble*)(uintptr_t)a.wd;
  for (int blk = blockIdx.x; blk < nblk; blk += gridDim.x) {        // workgroup-uniform: the weight addresses below stay scalar
    const int p = blk * 256 + (int)threadIdx.x;
    const int pr = p < a.P ? p : a.P - 1;                           // a lane beyond P reads the last point's rows and stores nothing
    const char* dzrow = a.dz + (size_t)pr * a.ld_dz * 4;
    const int* Erow = a.Edz + (size_t)(pr >> 7) * ncb;
    double q[3] = {0.0, 0.0, 0.0};
    for (int ch = 0; ch < nchunk; ++ch) {
      double acc[EC];
#pragma unroll
      for (int e = 0; e < EC; ++e) acc[e] = 0.0;
      for (int g = 0; g < (a.W >> 4); ++g) {
        const bsp::u32x4* src = reinterpret_cast<const bsp::u32x4*>(dzrow + (size_t)g * 64);
        const bsp::f16x8 h0 = __builtin_bit_cast(bsp::f16x8, src[0]), h1 = __builtin_bit_cast(bsp::f16x8, src[1]);
        const bsp::f16x8 l0 = __builtin_bit_cast(bsp::f16x8, src[2]), l1 = __builtin_bit_cast(bsp::f16x8, src[3]);
        const int ex = -Erow[g >> 3];
        cdouble* wrow = wd + (size_t)(g * 16) * a.ldw + ch * EC;
#pragma unroll
        for (int jj = 0; jj < 16; ++jj) {
          const float hi = (float)(jj < 8 ? h0[jj & 7] : h1[jj & 7]), lo = (float)(jj < 8 ? l0[jj & 7] : l1[jj & 7]);
          const double d = (double)__builtin_amdgcn_ldexpf(hi + lo, ex);
          cdouble* w = wrow + (size_t)jj * a.ldw;
#pragma unroll
          for (int e = 0; e < EC; ++e) acc[e] = __builtin_fma(d, w[e], acc[e]);
        }
      }
      if (NF == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) q[c] = acc[c];
      } else {
        const char* perow = a.pe + (size_t)pr * a.Ep * 4;
        const int epe = a.Epe[pr >> 7];                               // Ep <= 128: one column block
#pragma unroll
        for (int kk = 0; kk < (NF > 0 ? NF : 1); ++kk) {
          const int k = ch * NF + kk;
          if (k < a.F) {
            const double f = (double)(1 << k);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
              const double es = (double)plane_elem(perow, 6 * k + c, epe), ec = (double)plane_elem(perow, 6 * k + 3 + c, epe);
              const double ta = acc[(6 * kk + c) % EC] * ec;
              const double tb = acc[(6 * kk + 3 + c) % EC] * es;
              const double df = ta - tb;
              const double sf = df * f;
              q[c] = q[c] + sf;
            }
          }
        }
      }
    }
    if (p < a.P) {
      double* o = a.G + (size_t)p * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) o[c] = a.first ? q[c] : o[c] + q[c];
    }
  }
}

int launch_encgrad(const EncGradArgs& a, hipStream_t st) {
  const int nf = encgrad_nf(a.F);
  if (!a.dz || !a.Edz || !a.pe || !a.Epe || !a.wd || !a.G || a.P <= 0 || a.W <= 0 || (a.W & 15) || (a.ld_dz & 15) || a.W > a.ld_dz ||
      a.F < 0 || a.F > 16 || a.Ep > 128 || (a.Ep & 15) || (nf ? 6 * a.F : 3) > a.Ep || a.ldw < (nf ? round_up(6 * a.F, 6 * nf) : 3)) {
    set_error("encoding gradient: bad argument");
    return SNERF_ERR_BAD_DESC;
  }
  const int nblk = (a.P + 255) / 256;
  const dim3 grid((unsigned)(g_encgrad_grid > 0 && g_encgrad_grid < nblk ? g_encgrad_grid : nblk));
  if (nf == 0) hipLaunchKernelGGL(encgrad_kernel<0>, grid, dim3(256), 0, st, a);
  else if (nf == 5) hipLaunchKernelGGL(encgrad_kernel<5>, grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(encgrad_kernel<10>, grid, dim3(256), 0, st, a);
  SNERF_LAUNCH_CHECK();
  return SNERF_OK;
}

// grad_ray[ray][c] = 0.0 + G[ray S][c] + G[ray S + 1][c] + ...; grad_sample = (float)G where asked for
__global__ __launch_bounds__(RAY_WAVE * RAY_WAVE_MAX_RAYS_PER_BLOCK) void ray_fold3_kernel(
    const double* __restrict__ G, int n_rays, int S, double* __restrict__ grad_ray, float* __restrict__ grad_sample) {
  const auto [lane, wave, ray] = ray_wave_id();
  if (ray >= n_rays) return;                                   // wave-uniform: see ray_wave.h
  double acc[3] = {0.0, 0.0, 0.0};
  for (int s0 = 0; s0 < S; s0 += RAY_WAVE) {
    const int s = s0 + lane;
    double v[3] = {0.0, 0.0, 0.0};
    if (s < S) {
      const size_t pt = (size_t)ray * S + s;
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c] = G[pt * 3 + c];
      if (grad_sample) {
#pragma unroll
        for (int c = 0; c < 3; ++c) grad_sample[pt * 3 + c] = (float)v[c];
      }
    }
    const int n = S - s0 < RAY_WAVE ? S - s0 : RAY_WAVE;       // wave-uniform
    for (int l = 0; l < n; ++l) {
#pragma unroll
      for (int c = 0; c < 3; ++c) acc[c] = acc[c] + __shfl(v[c], l, RAY_WAVE);
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < 3; ++c) grad_ray[ray * 3 + c] = acc[c];
  }
}

int launch_ray_fold3(const double* G, int N, int S, double* grad_ray, float* grad_sample, hipStream_t st) {
  const RayWaveLaunch l = ray_wave_launch(N, 0);               // no LDS: four rays per workgroup
  hipLaunchKernelGGL(ray_fold3_kernel, l.grid, l.block, l.lds_bytes, st, G, N, S, grad_ray, grad_sample);
  SNERF_LAUNCH_CHECK();
  return SNERF_OK;
}

namespace {
// every refusal of the two entries that reads the descriptor alone; `who` begins the message
int plan_for(const char* who, const SnerfDesc* d, Plan* p) {
  const unsigned f = d->flags;
  if (!(f & SNERF_FLAG_TRAIN)) {
    set_error("%s: the descriptor lacks SNERF_FLAG_TRAIN (the pass reads the activations a training forward keeps)", who);
    return SNERF_ERR_BAD_DESC;
  }
  const struct { unsigned bit; const char* name; } no[] = {
      {SNERF_FLAG_SC_PASS, "SNERF_FLAG_SC_PASS"}, {SNERF_FLAG_RELIGHT, "SNERF_FLAG_RELIGHT"}, {SNERF_FLAG_GEOMETRY, "SNERF_FLAG_GEOMETRY"},
      {SNERF_FLAG_EMBED_GRAD, "SNERF_FLAG_EMBED_GRAD"}, {SNERF_FLAG_DEPTH_MEDIAN, "SNERF_FLAG_DEPTH_MEDIAN"}};
  for (const auto& b : no)
    if (f & b.bit) {
      set_error("%s: %s is not a flag of this pass (it follows the training forward of a main pass)", who, b.name);
      return SNERF_ERR_BAD_DESC;
    }
  if (f & SNERF_FLAG_F16X1) {
    set_error("%s: the one-plane arithmetic SNERF_FLAG_F16X1 is not supported (its gradient bars are a question of their own); use the default arithmetic", who);
    return SNERF_ERR_BAD_DESC;
  }
  const int rc = make_plan(d, p);
  if (rc) {
    char why[400];
    strncpy(why, snerf_last_error(), sizeof(why) - 1);
    why[sizeof(why) - 1] = 0;
    set_error("%s: %s", who, why);
  }
  return rc;
}
}  // namespace

}  // namespace snerf

using namespace snerf;

extern "C" {

int snerf_normals_scratch_bytes(const SnerfDesc* desc, size_t* bytes) {
  if (!desc) { set_error("snerf_normals_scratch_bytes: desc is NULL"); return SNERF_ERR_NULL; }
  if (!bytes) { set_error("snerf_normals_scratch_bytes: bytes is NULL"); return SNERF_ERR_NULL; }
  Plan p;
  RC(plan_for("snerf_normals_scratch_bytes", desc, &p));
  *bytes = normals_scratch(p).bytes;
  return SNERF_OK;
}

int snerf_density_grad(const SnerfDesc* desc, const float* packed_params, const SnerfInputs* inputs, const float* coef,
                       double* grad_ray, float* grad_sample, void* workspace, void* scratch, void* stream) {
  const struct { const void* ptr; const char* name; } need[] = {
      {desc, "desc"}, {packed_params, "packed_params"}, {inputs, "inputs"}, {coef, "coef"}, {grad_ray, "grad_ray"},
      {workspace, "workspace"}, {scratch, "scratch"}};
  for (const auto& n : need)
    if (!n.ptr) { set_error("snerf_density_grad: %s is NULL", n.name); return SNERF_ERR_NULL; }
  Plan p;
  RC(plan_for("snerf_density_grad", desc, &p));
  if (!inputs->sun_d || inputs->sun_stride < 3) { set_error("snerf_density_grad: inputs->sun_d (N,3) with stride >= 3 is required (the inputs of the forward)"); return SNERF_ERR_NULL; }
  if (((uintptr_t)workspace & 255) || ((uintptr_t)packed_params & 255) || ((uintptr_t)scratch & 255)) {
    set_error("snerf_density_grad: workspace, scratch and packed params must be 256-byte aligned");
    return SNERF_ERR_WORKSPACE;
  }
  return density_grad_bsp(p, packed_params, inputs, coef, grad_ray, grad_sample, workspace, scratch, (hipStream_t)stream);
}

int snerf_test_normals_grid(int n) { encgrad_set_grid_override(n); return SNERF_OK; }
int snerf_test_normals_dump(float* dz, float* enc) { g_dump.dz = dz; g_dump.enc = enc; return SNERF_OK; }

}  // extern "C"
