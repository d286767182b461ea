/* Extension of the C-ABI of libsnerf_hip.so: the gradient of the density with respect to the sample position -- the backward of a
 * training pass that runs only the launches between a cotangent on sigma and xyz, as SNERF_FLAG_EMBED_GRAD does for the transient
 * embedding.  Its weight-averaged direction along a ray is the surface normal  n = -sum_i w_i grad sigma(x_i) / |.|  (Ref-NeRF).  The
 * reference has no counterpart; DESIGN.md section 5za, the two new kernels restated in numpy by tests/normals_numpy.py.
 *
 * include/snerf_hip.h is the ABI-6 surface and its list of entry points is frozen; an entry added at the same ABI version is
 * declared in a header of its own (as include/snerf_roofs.h), which includes it for the error codes and SnerfDesc / SnerfInputs.
 * Same conventions: plain pointers + sizes, device pointers unless stated, `stream` is a hipStream_t, 0 = SNERF_OK, a message for
 * every other return through snerf_last_error(); no entry allocates or synchronises with the host.  snerf_version() stays 6 and no
 * size snerf_workspace_bytes reports changes: what the pass needs beyond a training workspace lives in a scratch buffer of its own.
 * The Python binding is this header's group of rows in _lib.HEADER_SIGNATURES (tests/test_normals_cpu.py compares it with this file). */
#ifndef SNERF_NORMALS_H
#define SNERF_NORMALS_H

#include "snerf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* snerf_normals_scratch_bytes: *bytes = the size of the `scratch` buffer snerf_density_grad needs for this descriptor (256-byte
 * aligned regions: the per-sample gradients (P, 3) fp64, the fp64 copy of one layer's encoding columns, the discarded bias sums).
 * Refused (SNERF_ERR_NULL / SNERF_ERR_BAD_DESC, *bytes untouched): a null desc or bytes, and every descriptor snerf_density_grad
 * refuses. */
int snerf_normals_scratch_bytes(const SnerfDesc* desc, size_t* bytes);

/* snerf_density_grad: g[n][s] = coef[n][s] * d sigma(x_ns) / d x_ns in normalised scene coordinates, sigma being the density the pass
 * handed out (after the softplus), x_ns = o_n + d_n z_ns the sample position the pass encoded.
 *   desc, packed_params, inputs: those of the snerf_forward(SNERF_FLAG_TRAIN) that wrote `workspace` (the contract of snerf_backward;
 *     the pass reads inputs->sun_d only to satisfy the composite backward it shares with snerf_backward);
 *   coef (N, S) fp32;  workspace: that forward's workspace;  scratch: snerf_normals_scratch_bytes bytes, 256-byte aligned;
 *   grad_ray (N, 3) fp64: sum_s g[n][s], s ascending;  grad_sample (N, S, 3) fp32 or NULL: (float)g[n][s].
 * Every word of grad_ray (and grad_sample) is written; nothing of scratch is read before it is written.
 * The pass: composite backward with g_sigmas = coef alone -> d sigma's pre-activation; its planes; the dX launch into the last trunk
 * layer from those planes alone (K = 32 against the sigma rows of the transposed pack); the trunk's dX launches L - 1 ... 1 as in
 * snerf_backward, no dW launch, no reduction.  At every layer i that reads the encoding (every skip layer, then layer 0), while that
 * layer's dz is live, per point p with W_i the layer's fp32 master weights, E = 6 F encoding columns (3 for the identity encoding):
 *     T[e] = sum_{j = 0 .. W - 1, ascending} (double)dz[p][j] * (double)W_i[j][e]          one fp64 accumulator from 0.0, each product
 *                                                                                           exact, one rounding per addition
 *     F > 0, with enc = the stored encoding decoded to fp32, column 6 k + c = sin(2^k x_c), 6 k + 3 + c = cos(2^k x_c):
 *       q[c] = 0.0;  for k = 0 .. F - 1 ascending:  q[c] = q[c] + ((T[6k+c] * enc[6k+3+c]) - (T[6k+3+c] * enc[6k+c])) * 2^k
 *     F = 0 (identity encoding): q[c] = T[c]
 *     G[p][c] = q[c] at the first such layer (the highest skip layer), G[p][c] + q[c] at each later one
 * every operation fp64, rounded on its own (no contraction).  dz and enc are the plane tensors as the pass left them, decoded
 * (float)hi + (float)lo scaled by the block's power of two.  Then grad_ray[n][c] = 0.0 + G[n S][c] + G[n S + 1][c] + ... in that
 * order.  No order depends on the launch geometry.  No transcendental is evaluated: the Jacobian of the encoding is taken from the
 * stored encoding.
 * snerf_backward on the same workspace afterwards gives what it gives without this call; the outputs of the forward are untouched.
 * Refused before any launch, each with a message that begins "snerf_density_grad: ":
 *   SNERF_ERR_NULL      a null desc, packed_params, inputs, coef, grad_ray, workspace or scratch;
 *   SNERF_ERR_BAD_DESC  a descriptor the plan refuses (sizes); one without SNERF_FLAG_TRAIN; one with SNERF_FLAG_SC_PASS,
 *                       SNERF_FLAG_RELIGHT, SNERF_FLAG_GEOMETRY, SNERF_FLAG_EMBED_GRAD or SNERF_FLAG_DEPTH_MEDIAN; the one-plane
 *                       arithmetic SNERF_FLAG_F16X1;
 *   SNERF_ERR_WORKSPACE a workspace, scratch or packed_params that is not 256-byte aligned. */
int snerf_density_grad(const SnerfDesc* desc, const float* packed_params, const SnerfInputs* inputs, const float* coef,
                       double* grad_ray, float* grad_sample, void* workspace, void* scratch, void* stream);

/* Test hooks (tests/test_gpu_normals.py), never on the product path.
 * snerf_test_normals_grid: the encoding-gradient kernel runs on n workgroups (0: the default grid).
 * snerf_test_normals_dump: while dz is non-NULL, every snerf_density_grad also writes what its encoding-gradient launches read, decoded
 * to fp32: dz (n_enc_layers, P, W) in launch order (skip layers descending, then layer 0) and enc (P, Ep).  (NULL, NULL) ends it. */
int snerf_test_normals_grid(int n);
int snerf_test_normals_dump(float* dz, float* enc);

#ifdef __cplusplus
}
#endif
#endif
