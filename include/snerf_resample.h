/* Extension of the C-ABI of libsnerf_hip.so: importance resampling of the depths.
 *
 * include/snerf_hip.h is the ABI-6 surface and its list of entry points is frozen (tests/test_embed_grad_cpu.py pins it symbol by
 * symbol); an entry added at the same ABI version is declared in a header of its own, which includes it for the error codes and
 * limits.  Same conventions: plain pointers + sizes, device pointers unless a parameter is called *_host, `stream` is a
 * hipStream_t, 0 = SNERF_OK, a message for every other return through snerf_last_error().  snerf_version() stays 6.
 * The Python binding is the table _lib.EXTENSION_SIGNATURES (tests/test_resample_cpu.py compares it with this file). */
#ifndef SNERF_RESAMPLE_H
#define SNERF_RESAMPLE_H

#include "snerf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Importance resampling of the depths (sample_pdf, framework/components/rendering.py:8-51, and the sort of the merged depths its
 * callers do): n_importance fine samples per ray, drawn from the pdf that a proposal pass's weights (N,S) define over the S - 1
 * midpoints of the coarse depths z (N,S; fp32, non-decreasing along a ray, no NaN), merged with z into z_out (N, S + Ni).  NeRF's
 * convention: the bins are the interval midpoints, the pdf is over the S - 2 interior weights.  u (N,Ni) are the uniforms; NULL is
 * the reference's det=True.  z_fine (N,Ni), optional, receives the fine samples alone, in u's order.
 *
 * The arithmetic, per ray -- fp64, every operation rounded on its own (no fused multiply-add), sums in exact integers, so the
 * result has no summation order and tests/resample_numpy.py reproduces every bit:
 *   1. b[j] = 0.5 * ((double)z[j] + (double)z[j+1]),  j = 0 .. S-2
 *   2. w' = w where w is finite and > 0, else 0; w' = min(w', 1);  m[j] = llrint((w'[j+1] + 1e-5) * 2^50) as int64,  j = 0 .. S-3
 *      (the reference's eps = 1e-5; 2^50 keeps every prefix of real weights, sum <= 1, exactly representable in a double)
 *   3. P[0] = 0, P[j+1] = P[j] + m[j] in int64;  T = P[S-2]
 *   4. u_i = (double)u[n][i] where that is > 0, else +0 (NaN included), at most 1;  with u == NULL: u_i = (double)i / (double)(Ni-1),
 *      and 0 when Ni = 1
 *   5. t = u_i * (double)T;  k = the largest j in [0, S-3] with (double)P[j] <= t  (t == T lands in the last bin)
 *   6. f = (t - (double)P[k]) / (double)m[k];  fine_i = (float)(b[k] + f * (b[k+1] - b[k]))
 *   7. z_out = concatenate([z, fine]) reordered by numpy's STABLE argsort of its values: among equal values (+0 and -0 are equal)
 *      coarse before fine, then index order.
 * Every mass is at least 1e-5 * 2^50: no zero denominator and no special case.  This is the one deliberate difference from the
 * reference, which sets a denominator below eps to 1 and so pins a sample that falls into a near-empty bin to the bin's left edge;
 * here it is interpolated.  Both stay inside the same bin.
 * One launch on `stream`; no allocation, no copy, no host synchronisation.  Refused on the host before any launch: a NULL z,
 * weights or z_out (SNERF_ERR_NULL); n_rays < 1, n_samples < 3, n_importance < 1, n_samples + n_importance > SNERF_VIS_MAX_SAMPLES
 * (SNERF_ERR_BAD_DESC; the limit SNERF_VIS_MAX_SAMPLES of snerf_hip.h already puts on a ray). */
int snerf_resample_z(const float* z, const float* weights, const float* u, float* z_out, float* z_fine, int n_rays, int n_samples,
                     int n_importance, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SNERF_RESAMPLE_H */
