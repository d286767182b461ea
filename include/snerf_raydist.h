/* Extension of the C-ABI of libsnerf_hip.so: the distortion loss on a ray's weights, value and gradient in one launch.
 *
 * include/snerf_hip.h is the ABI-6 surface and its list of entry points is frozen (tests/test_embed_grad_cpu.py pins it symbol by
 * symbol); an entry added at the same ABI version is declared in a header of its own, which includes it for the error codes and
 * limits.  Same conventions: plain pointers + sizes, device pointers, `stream` is a hipStream_t, 0 = SNERF_OK, a message for every
 * other return through snerf_last_error().  snerf_version() stays 6.
 * The Python binding is the table _lib.EXTENSION_SIGNATURES (tests/test_raydist_cpu.py compares it with this file). */
#ifndef SNERF_RAYDIST_H
#define SNERF_RAYDIST_H

#include "snerf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The distortion regulariser of mip-NeRF 360 on the weights (N,S) a pass composited along the depths z_vals (N,S):
 *     L = sum_i sum_j w_i w_j |m_i - m_j| + 1/3 sum_i w_i^2 delta_i
 * over the normalised interval midpoints m and widths delta of a ray, as the per-ray value L_r and d L_r / d weights, in O(S) per
 * ray.  The depths carry no gradient.  `rays` (N, ray_stride) gives a ray's bounds: near = column 6, far = column 7.
 *
 * The arithmetic, per ray -- fp64, every operation rounded on its own (no fused multiply-add), every sum over exact int64
 * integers, so no result depends on how a scan is spread over lanes and tests/raydist_numpy.py reproduces every bit.  Q = 2^50.
 *   1. t_i = ((double)z_i - near) / (far - near);  delta_i = t_{i+1} - t_i for i < S-1, delta_{S-1} = 0;  m_i = t_i + 0.5 * delta_i
 *   2. w'_i = min(max((double)w_i, 0), 1), a zero of either sign giving +0;  a_i = llrint(w'_i * Q);  b_i = llrint((w'_i * m_i) * Q)
 *   3. exclusive prefixes in int64: A_i = sum_{j<i} a_j, B_i = sum_{j<i} b_j; the totals A_T, B_T;  Abar = (double)A / Q, Bbar alike
 *   4. e_i = 2 * (w'_i * (m_i * Abar_i - Bbar_i)) + ((w'_i * w'_i) * delta_i) / 3;  q_i = llrint(e_i * Q);
 *      L_int = sum_i q_i (int64, two's complement);  L_r = (double)L_int / Q
 *   5. g_k = 2 * ((m_k * Abar_k - Bbar_k) + (Bbar'_k - m_k * Abar'_k)) + ((2/3) * w'_k) * delta_k, where
 *      Abar'_k = (double)(A_T - A_k - a_k) / Q and Bbar'_k alike (the mass behind sample k), 2/3 the double 2.0 / 3.0;
 *      d_weights[k] = (float)g_k; +0 where w_k < 0 or w_k > 1 (the clamp's derivative); an exact w_k = 0 keeps the formula
 *   6. a ray is BAD when some w_i or z_i is not finite, z_{i+1} < z_i somewhere, near or far is not finite, !(far > near), or some
 *      t_i lies outside [-1, 2].  A bad ray has a d_weights row of +0, a per-ray value of NaN (0x7ff8000000000000) and adds
 *      nothing to the sum.
 *   7. acc: 4 u64 words which the CALLER zeroes, accumulated with integer atomics (calls into one acc add up: the words of a batch
 *      cut into shards equal the whole batch's):
 *        [0] += llrint(L_r * 2^40) over the good rays (int64, two's complement)   [1] += rays of the call   [2] += bad rays
 *        [3] reserved, not written
 * With real weights (sum <= 1, t in [0, 1]) L_r <= 4/3, so word 0 cannot wrap below about 6e6 rays per accumulator.  The bounds
 * on t keep every integer of one ray within int64 for any weights: |b_i| <= 2 Q, |q_i| < 2^13 Q, |A|, |B| <= 2^11 Q.
 * d_weights (N,S) and per_ray (N, optional) are pure outputs: every element is written.
 * One launch on `stream`; no allocation, no copy, no host synchronisation.  Refused on the host before any launch: a NULL weights,
 * z_vals, rays, d_weights or acc (SNERF_ERR_NULL); n_rays < 1 or > 2^22, n_samples < 1 or > SNERF_VIS_MAX_SAMPLES, ray_stride < 8
 * (SNERF_ERR_BAD_DESC). */
int snerf_ray_distortion(const float* weights, const float* z_vals, const float* rays, int ray_stride, int n_rays, int n_samples,
                         float* d_weights, double* per_ray, unsigned long long* acc, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SNERF_RAYDIST_H */
