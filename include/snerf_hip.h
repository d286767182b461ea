/*
 * snerf_hip.h -- C-ABI of libsnerf_hip.so: the MI355X (gfx950) implementation of the semantic
 * Sat-NeRF ray-marching hot path (encode -> SIREN/ReLU MLP + heads -> irradiance alpha-composite
 * -> losses, forward and backward).
 *
 * The reference (wagnva/semantic-nerf-for-satellite-data) is pure Python/PyTorch and has no FFI of
 * its own; each entry point below names the reference interface it replaces (paths relative to the
 * reference repository).  INTEGRATION.md shows the ctypes binding a maintainer adds on the
 * reference side.
 *
 * Conventions
 *   - plain C: pointers + sizes only, no torch types; every pointer is a DEVICE pointer on the
 *     current HIP device unless stated otherwise; row-major fp32 unless stated otherwise;
 *   - return 0 on success, non-zero error code otherwise; snerf_last_error() gives the message;
 *     no exceptions cross the ABI;
 *   - no allocation and no synchronisation inside the hot calls: the caller provides the workspace
 *     (size from snerf_workspace_bytes) and a stream; calls are asynchronous on that stream
 *     (hipGraph-capturable);
 *   - one caller thread per device/stream (the reference drives everything from one Python thread,
 *     framework/pipelines.py:306-320); re-entrant across devices (one process per GPU).
 */
#ifndef SNERF_HIP_H
#define SNERF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SNERF_ABI_VERSION 6
#define SNERF_MAX_LAYERS 16

/* error codes */
#define SNERF_OK 0
#define SNERF_ERR_BAD_DESC 1
#define SNERF_ERR_WORKSPACE 2
#define SNERF_ERR_NULL 3
#define SNERF_ERR_HIP 4

/* SnerfDesc.flags */
#define SNERF_FLAG_TRAIN 1u   /* keep every activation needed by snerf_backward in the workspace */
#define SNERF_FLAG_SC_PASS 2u /* solar-correction variant: sample points on o + sun_d*z, evaluate only the
                                 trunk + sigma + sun-visibility branch and return weights/transparency/sun
                                 (semantic/components/rendering.py:59-78) */
#define SNERF_FLAG_RELIGHT 4u /* relight: re-render the chunk a finished inference main pass left in `workspace` under another sun
                                 (and t / t_s) WITHOUT re-running positions, encoding, the trunk, sigma or the rgb / semantic / beta
                                 heads -- only the extras columns [sun | t | t_s], the sun block of the first head layer, the
                                 sun-visibility layers, the sky colour and the composite are run again (about a tenth of a pass's
                                 matrix work).  Every result has the bits a full pass under that sun gives.  Not with SNERF_FLAG_TRAIN or
                                 SNERF_FLAG_SC_PASS (SNERF_ERR_BAD_DESC).  Contract: see snerf_forward */
#define SNERF_FLAG_EMBED_GRAD  16u /* embedding-only backward: snerf_backward writes d_t / d_t_s and NOTHING else -- it stops where the
                                 gradient of the transient embedding is complete (no weight-gradient launch, no sun-visibility chain,
                                 no trunk), and packed_grads may be NULL.  Valid only together with SNERF_FLAG_TRAIN and never with
                                 SNERF_FLAG_RELIGHT (SNERF_ERR_BAD_DESC); combines with SNERF_FLAG_SC_PASS and either arithmetic flag.
                                 snerf_forward and every size ignore the bit.  Contract: see snerf_backward */
#define SNERF_FLAG_GEOMETRY  32u /* geometry-only inference pass: depths (sampled, in->z_vals or in->xyz), the encoding, the trunk, sigma and
                                 the composite -- no head launch at all.  Produces depth, weights, transparency, sigmas and z_vals with the
                                 bits of the plain inference pass of the same descriptor and inputs; any other non-NULL SnerfOutputs
                                 pointer is refused by name before any launch.  in->sun_d, in->t and in->t_s are not read and may be NULL.
                                 Not with SNERF_FLAG_TRAIN, SNERF_FLAG_SC_PASS, SNERF_FLAG_RELIGHT or SNERF_FLAG_EMBED_GRAD
                                 (SNERF_ERR_BAD_DESC); either arithmetic flag.  snerf_workspace_bytes plans only what the pass writes
                                 (strictly less than the plain inference pass); a larger workspace is accepted.  A workspace a geometry
                                 pass wrote last holds no head tensors: a relight on it is refused */
#define SNERF_FLAG_DEPTH_MEDIAN  128u /* median depth: snerf_forward runs the pass exactly as without the bit, then ONE further launch on the same
                                 stream overwrites out->depth (N) with the MEDIAN depth of each ray -- the depth at which half of the ray's
                                 weight lies in front -- computed from the out->weights and out->z_vals the pass just wrote.  Every other
                                 result keeps the bits of the pass without the bit.  Per ray, with w_i, z_i the fp32 values in memory
                                 (i in [0, S)), every operation fp64 and rounded on its own, every sum in int64:
                                   1. a w_i or z_i that is not finite, or z_{i+1} < z_i for some i: depth = quiet NaN; likewise, where
                                      out->sigmas is non-NULL, a sigma_i the pass wrote there that is not finite (the composite maps such a
                                      density -- a ray with a NaN origin or direction -- to zero weights, which alone would read as an empty ray);
                                   2. wc_i = min(max((double)w_i, 0), 1), a zero of either sign giving +0;  a_i = llrint(wc_i * 2^50);
                                   3. A_i = sum_{k<i} a_k, AT = sum a_k (<= 2^60);  AT == 0: depth = z_{S-1} (nothing on the ray: the far end);
                                   4. j = the first index with 2 (A_j + a_j) >= AT;  j == S-1: depth = z_{S-1} (the last interval is the
                                      reference's open-ended 1e10 one: its mass sits at its near edge);
                                   5. else frac = (double)(AT - 2 A_j) / (double)(2 a_j), span = (double)z_{j+1} - (double)z_j,
                                      depth = (float)((double)z_j + frac * span).  A tie gives frac = 1, i.e. z_{j+1}.
                                 The weight is normalised by the ray's own total (a ray that does not saturate still has a median), and
                                 each w_j is spread uniformly over [z_j, z_{j+1}], the interval whose opacity produced it
                                 (framework/util/rendering.py convert_sigmas): the result sits about half an interval deeper than a mean
                                 that puts w_j at z_j.  The result does not depend on how the sums are spread over the lanes.
                                 Valid with the plain inference pass, SNERF_FLAG_GEOMETRY, SNERF_FLAG_RELIGHT (the relight's composite
                                 rewrites weights and depth; the median launch follows it) and either arithmetic flag.  Not with
                                 SNERF_FLAG_TRAIN, SNERF_FLAG_SC_PASS or SNERF_FLAG_EMBED_GRAD, and n_samples must be in
                                 [1, SNERF_VIS_MAX_SAMPLES]: SNERF_ERR_BAD_DESC from the plan, hence from the size entries and both hot
                                 calls, before any pointer is looked at; snerf_backward refuses the bit.  Needs out->depth, out->weights
                                 and out->z_vals: a NULL one is refused by name (SNERF_ERR_NULL) before any launch.
                                 snerf_workspace_bytes, snerf_packed_floats and snerf_grad_floats ignore the bit, and so does what a pass
                                 leaves in its workspace: a relight, with or without the bit, may follow a base pass with or without it.
                                 No allocation, no copy, no host synchronisation; one extra launch with the bit, none without */

/* Arithmetic of the dense contractions.  With NONE of the arithmetic bits set a pass runs the default, SNERF_FLAG_F16X2
 * (the same for C and Python callers); the two bits exclude each other. */
#define SNERF_FLAG_F16X2 64u   /* DEFAULT (flags = 0 means this): fp32-class arithmetic on the fp16 matrix cores.  Every activation
                                  tensor of the workspace is two fp16 planes (22 significant bits) with one power-of-two exponent
                                  per 128 x 128 block, written once by the producing kernel; a product is hi*hi + hi*lo + lo*hi on
                                  v_mfma_f32_32x32x16_f16 with fp32 accumulation; the dropped lo*lo term is 2^-22 relative, below
                                  an fp32 GEMM's own rounding (normwise).  Needs fc_units % 32 == 0, feat_last % 16 == 0 and
                                  3 + t_dim (x2 with a separate t_s) <= 16: other shapes return SNERF_ERR_BAD_DESC */
#define SNERF_FLAG_F16X1 8u    /* REDUCED precision (the reference's `precision = 16` runs, baseline/pipelines/nerf.py:65; BASELINE.json
                                  configs[2], [4]): the same block-scaled tensors with ONE fp16 plane -- 11 significant bits relative
                                  to the block's maximum, 2 bytes per element -- weights packed as one plane, one MFMA product per
                                  contraction step (a third of the default's matrix work, half its operand bytes), fp32 accumulate.
                                  Same kernels, templated on the plane count.  Judged on PSNR / mIoU, not on the 1e-4 parity bar.
                                  Needs fc_units % 64 == 0, feat_last % 32 == 0 and n_freq > 0 on top of the default's shape rules
                                  (raw xyz, n_freq = 0, would enter the w0 = 30 first layer rounded to 11 bits: SNERF_ERR_BAD_DESC) */

/* Model + batch description.  Field names follow the reference config
 * (configs/pipelines/rs_semantic.toml:13-67, semantic/pipelines/rs_semantic.py:125-141). */
typedef struct SnerfDesc {
  int32_t n_rays;      /* N */
  int32_t n_samples;   /* S (n_samples) */
  int32_t fc_units;    /* W */
  int32_t fc_layers;   /* L <= SNERF_MAX_LAYERS */
  int32_t feat_last;   /* H = W/2, or W with fc_use_full_features */
  uint32_t skip_mask;  /* bit i set <=> i in fc_skips */
  int32_t n_freq;      /* mapping_pos_n_freq; 0 = identity encoding (baseline SatNeRF, satnerf.py:140-141) */
  int32_t siren;       /* activation_function == "siren" */
  int32_t t_dim;       /* t_embedding_tau */
  int32_t n_classes;   /* semantic classes C; 0 = baseline SatNeRF without semantic head */
  int32_t sem_sigmoid; /* semantic_activation_function == "sigmoid" */
  int32_t use_tj_instead_of_beta;
  int32_t use_tj_for_s;
  int32_t use_separate_beta_for_s;
  int32_t use_separate_tj_for_semantic;
  uint32_t flags;
} SnerfDesc;

/* Raw device pointers to the parameter tensors, in the reference's state_dict layout
 * (fc_net.{2i}.{weight,bias}, sigma_from_xyz.0.*, feats_from_xyz.*, rgb_from_xyzdir.{0,2}.*,
 * semantic_prediction.{0,2}.*, sun_v_net.{0,2,4,6}.*, sky_color.{0,2}.*, beta_from_xyz.{0,2}.*,
 * semantic_beta_from_xyz.{0,2}.*).  torch Linear layout: weight (out,in) row-major contiguous, bias (out).
 * The library never owns them.  Used both for parameters (read) and for their gradients (written). */
typedef struct SnerfParams {
  float* fc_w[SNERF_MAX_LAYERS];
  float* fc_b[SNERF_MAX_LAYERS];
  float* sigma_w; float* sigma_b;
  float* feats_w; float* feats_b;
  float* rgb_w0; float* rgb_b0; float* rgb_w2; float* rgb_b2;
  float* sem_w0; float* sem_b0; float* sem_w2; float* sem_b2;       /* NULL when n_classes == 0 */
  float* sun_w[4]; float* sun_b[4];
  float* sky_w0; float* sky_b0; float* sky_w2; float* sky_b2;
  float* beta_w0; float* beta_b0; float* beta_w2; float* beta_b2;
  float* sbeta_w0; float* sbeta_b0; float* sbeta_w2; float* sbeta_b2; /* NULL unless use_separate_beta_for_s */
} SnerfParams;

/* Ray batch.  Either (rays [+ z_vals | z_steps [+ u]]) -- the renderer seam,
 * framework/components/rendering.py:84-157 -- or explicit (xyz, z_vals) -- the inference() seam,
 * semantic/models/rs_semantic.py:8-19. */
typedef struct SnerfInputs {
  const float* rays;    /* (N,8): origin 0:3, dir 3:6, near 6, far 7 (framework/components/rays.py:7-38) */
  const float* xyz;     /* (N,S,3) explicit sample positions, or NULL */
  const float* z_vals;  /* (N,S) explicit depths, or NULL => stratified sampling from rays */
  const float* z_steps; /* (S) = linspace(0,1,S) from the host; needed when z_vals == NULL */
  const float* u;       /* (N,S) uniform [0,1) jitter, or NULL => no perturbation */
  const float* sun_d;   /* (N,3) with row stride sun_stride floats (4 when pointing into extras (N,4)) */
  int32_t sun_stride;
  int32_t _pad;
  const float* t;       /* (N,tau) transient embedding rows (models["t"](ts)) */
  const float* t_s;     /* (N,tau) or NULL */
} SnerfInputs;

/* Result tensors = the dict returned by inference() (rs_semantic.py:111-128); any pointer may be NULL.
 * With SNERF_FLAG_SC_PASS only weights / transparency / sun are produced; with SNERF_FLAG_GEOMETRY only depth / weights /
 * transparency / sigmas / z_vals may be asked for. */
typedef struct SnerfOutputs {
  float* rgb;             /* (N,3)  */
  float* depth;           /* (N)    */
  float* weights;         /* (N,S)  */
  float* transparency;    /* (N,S)  */
  float* albedo;          /* (N,S,3)*/
  float* sun;             /* (N,S,1)*/
  float* sky;             /* (N,S,3)*/
  float* beta;            /* (N,S,1)*/
  float* sigmas;          /* (N,S)  */
  float* beta_semantic;   /* (N,S,1) if use_separate_beta_for_s */
  float* semantic_logits; /* (N,C)  */
  int64_t* semantic_label;/* (N)    */
  float* z_vals;          /* (N,S) depths actually used (sampled or copied) */
} SnerfOutputs;

/* Gradients of the scalar loss w.r.t. the result tensors (same shapes; NULL = zero). */
typedef struct SnerfOutGrads {
  const float* rgb; const float* depth; const float* weights; const float* transparency;
  const float* albedo; const float* sun; const float* sky; const float* beta; const float* sigmas;
  const float* beta_semantic; const float* semantic_logits;
} SnerfOutGrads;

/* ---- library info ------------------------------------------------------------------------------ */
int snerf_version(void);
const char* snerf_last_error(void);

/* ---- sizes (host-side, no GPU work) -------------------------------------------------------------- */
/* number of floats of the packed parameter / packed gradient buffer */
size_t snerf_packed_floats(const SnerfDesc* desc);
/* floats of a packed GRADIENT buffer: the leading fp32 region of the packed layout -- all that snerf_backward accumulates
 * into and snerf_unpack_grads reads (the weight-operand packs behind it exist for parameters only) */
size_t snerf_grad_floats(const SnerfDesc* desc);
/* workspace bytes for one pass (activations + scratch) under desc->flags; the same buffer must be
 * handed to snerf_backward for that pass */
size_t snerf_workspace_bytes(const SnerfDesc* desc);

/* ---- parameter packing ------------------------------------------------------------------------- */
/* Gather the state_dict tensors into the padded, MFMA-friendly packed layout (DESIGN.md "Data layout").
 * Replaces nothing in the reference (torch.nn.Linear owns its layout there); run once per optimiser step.
 * The weight operands inside the buffer follow desc->flags' arithmetic (fragment-ordered fp16 planes + one exponent per matrix:
 * two planes in the default arithmetic, one under SNERF_FLAG_F16X1): pack, forward and backward must use the same arithmetic flag. */
int snerf_pack_params(const SnerfDesc* desc, const SnerfParams* params, float* packed, void* stream);
/* Scatter packed gradients back into tensors shaped like the parameters (overwrite, or add if accumulate). */
int snerf_unpack_grads(const SnerfDesc* desc, const float* packed_grads, const SnerfParams* grads,
                       int accumulate, void* stream);

/* ---- hot path ---------------------------------------------------------------------------------- */
/* One rendering pass: sample -> encode -> MLP -> composite.
 * Replaces BaseRenderer.render_rays/sample_rays (framework/components/rendering.py:84-157),
 * RSSemanticRendering._model_rendering (semantic/components/rendering.py:18-80; one call per pass),
 * inference + RSSemanticNeRF.forward (semantic/models/rs_semantic.py:8-128,260-340;
 * baseline/models/satnerf.py:8-98,203-255) and convert_sigmas (framework/util/rendering.py:4-34).
 *
 * With SNERF_FLAG_RELIGHT the call is a RELIGHT of a base pass.  The base pass is the last library call that wrote `workspace`
 * (the same pointer); it must have been an inference main pass (neither SNERF_FLAG_TRAIN nor SNERF_FLAG_SC_PASS) with the
 * identical descriptor apart from the RELIGHT bit -- hence the same n_rays, n_samples and arithmetic -- and the same packed
 * parameters.  The relight reads in->sun_d, in->sun_stride, in->t and in->t_s (t_s where the descriptor needs it) and ignores
 * rays, xyz, z_vals, z_steps and u.  It may fill any SnerfOutputs pointer a main pass can fill; out->z_vals is copied from the
 * workspace.  snerf_workspace_bytes(desc | RELIGHT) == snerf_workspace_bytes(desc).  It overwrites only the extras columns, the sun
 * block of the first head layer, the sun-visibility activations and pre-activations and the tile counters: any number of relights
 * may follow one base pass, each as if it were the first.
 * Refused on the host before any launch (SNERF_ERR_BAD_DESC): a workspace the library has not seen a pass write; one whose last
 * pass was a training, solar-correction or backward pass; a base pass with another descriptor; out->beta when the base pass was
 * asked for no beta (it may then have skipped the beta block of the first head layer).  The library remembers per workspace
 * ADDRESS which pass it queued last (host side, the 256 addresses noted last): this guards against mis-sequenced calls.  It cannot
 * know that the caller overwrote, freed or reallocated the buffer in between -- keeping the bytes intact is the caller's part.
 *
 * With SNERF_FLAG_DEPTH_MEDIAN (inference main pass, SNERF_FLAG_GEOMETRY or SNERF_FLAG_RELIGHT) one launch follows the pass's composite
 * on `stream` and overwrites out->depth with each ray's median depth, read off the out->weights and out->z_vals the pass wrote (spec
 * and refusals at the flag).  out->depth, out->weights and out->z_vals must all be non-NULL (SNERF_ERR_NULL, by name, before any
 * launch); out->sigmas is optional: where given, a ray with a sigma that is not finite gets a NaN depth instead of an empty ray's; every other result, the workspace and all sizes are those of the call without the bit. */
int snerf_forward(const SnerfDesc* desc, const float* packed_params, const SnerfInputs* in,
                  const SnerfOutputs* out, void* workspace, size_t workspace_bytes, void* stream);

/* Stratified depths only (sample_rays, framework/components/rendering.py:95-110): z (N,S) from rays (N,8),
 * z_steps (S) and an optional jitter tensor u (N,S).  Lets a caller share one z between passes on different streams. */
int snerf_sample_z(const float* rays, const float* z_steps, const float* u, float* z, int n_rays, int n_samples, void* stream);

/* The per-ray embedding rows (nn.Embedding(50, tau) indexed by the rays' image index `ts`:
 * semantic/components/rendering.py:35-46, baseline/components/rendering.py:29-40).
 * snerf_embedding_rows: rows[n][:] = table[idx[n]][:]  (forward; idx is int64 as torch hands it over).
 * snerf_embedding_backward: grad_table[v][:] += sum over the rays n with idx[n] == v of d_rows[n][:], summed in a fixed
 * order (no atomics: the gradient is bitwise reproducible, like every other one of the path).  Indices outside
 * [0, n_embed) give NaN rows in the forward and are skipped in the backward (torch's nn.Embedding asserts on the device). */
int snerf_embedding_rows(const float* table, int n_embed, int tau, const long long* idx, int n, float* rows, void* stream);
int snerf_embedding_backward(const long long* idx, const float* d_rows, int n, int tau, int n_embed, float* grad_table, void* stream);

/* Backward of one pass (what autograd does in the reference for the ops above): consumes the
 * activations that snerf_forward(SNERF_FLAG_TRAIN) left in `workspace`, ACCUMULATES parameter
 * gradients into packed_grads (caller zeroes it once per step) and writes d loss / d t (N,tau)
 * [and d t_s] when those pointers are non-NULL.
 *
 * With SNERF_FLAG_EMBED_GRAD the call computes d_t / d_t_s ALONE (fitting the embedding of an unseen image with the network frozen).
 * packed_grads may be NULL; it is never read or written, and no parameter gradient is computed.  At least one of d_t, d_t_s must be
 * non-NULL (SNERF_ERR_NULL).  What is written into d_t / d_t_s equals, element for element, what the full backward of the same
 * forward under the same cotangents writes there: the main pass runs the composite backward, the plane conversion of the final
 * layers' gradient, the one dX launch into the first head layer's pre-activation gradient and the narrow launch into the extras
 * columns with its per-ray sums -- the full pass's launches with the full pass's operands -- and stops; the solar-correction pass
 * (SNERF_FLAG_SC_PASS) zeroes d_t / d_t_s and launches nothing else.  The bit need not have been set in the forward:
 * snerf_forward(TRAIN | EMBED_GRAD) is snerf_forward(TRAIN) bit for bit, snerf_workspace_bytes is the same with and without it, and the
 * host may decide at backward time.  As after any backward, the workspace's activations are spent. */
int snerf_backward(const SnerfDesc* desc, const float* packed_params, const SnerfInputs* in,
                   const SnerfOutGrads* gout, float* packed_grads, float* d_t, float* d_t_s,
                   void* workspace, size_t workspace_bytes, void* stream);

/* ---- fused losses ---------------------------------------------------------------------------------
 * Replaces SNerfLoss / SatNerfLoss / uncertainty_aware_loss / solar_correction / DepthLoss
 * (baseline/components/loss.py:4-94), SemanticLoss / SemanticUncertaintyLoss / SemanticCarRegLoss
 * (semantic/components/loss.py:6-157) and their autograd backward.  Two phases because the means have
 * data-dependent denominators (CE over non-ignored rays, L_t over car rays): phase 1 reduces per-ray
 * sums and counts into totals[SNERF_LOSS_NTOT]; under data parallelism the host all-reduces that small
 * vector; phase 2 turns totals into the loss_dict values and d loss / d result tensors. */
#define SNERF_LOSS_NTOT 16
#define SNERF_LOSS_NTERMS 8
/* indices into terms[]: the reference's loss_dict keys */
#define SNERF_TERM_COLOR 0            /* coarse_color */
#define SNERF_TERM_LOGBETA 1          /* coarse_logbeta */
#define SNERF_TERM_SC2 2              /* coarse_sc_term2 */
#define SNERF_TERM_SC3 3              /* coarse_sc_term3 */
#define SNERF_TERM_SEMANTIC 4         /* coarse_semantic */
#define SNERF_TERM_SEMANTIC_LOGBETA 5 /* coarse_semantic_logbeta */
#define SNERF_TERM_CAR_REG 6          /* coarse_car_reg_loss */
#define SNERF_TERM_DS 7               /* coarse_ds */

typedef struct SnerfLossCfg {
  int32_t n_rays, n_samples, n_classes;
  int32_t color_mode;        /* 0 none, 1 SNerfLoss (plain MSE), 2 SatNerfLoss (beta-weighted + log beta) */
  int32_t has_sc;            /* solar-correction terms (needs the *_sc inputs) */
  int32_t sem_mode;          /* 0 none, 1 SemanticLoss, 2 SemanticUncertaintyLoss */
  int32_t ignore_index;      /* CrossEntropyLoss ignore_index: car index, or -100 */
  int32_t use_sbeta;         /* beta_semantic given (use_separate_beta_for_s) */
  int32_t detach_beta_for_s;
  int32_t car_reg;           /* SemanticCarRegLoss */
  int32_t car_label;
  int32_t has_depth;         /* DepthLoss on `depth` */
  float sc_lambda, lambda_s, lambda_c, ds_lambda;
} SnerfLossCfg;

typedef struct SnerfLossIn {
  const float* rgb; const float* weights; const float* beta; const float* beta_semantic;
  const float* semantic_logits;
  const float* sun_sc; const float* transparency_sc; const float* weights_sc;
  const float* depth;
  const float* gt_rgb;            /* (N,3) */
  const int64_t* labels;          /* (N) */
  const uint8_t* mask;            /* (N) bool, NULL = all rays (semantic_sparsity_mask) */
  const float* gt_depth;          /* (N) */
  const float* depth_weights;     /* (N) or NULL = 1 (ds_noweights) */
} SnerfLossIn;

typedef struct SnerfLossGrads { /* any may be NULL */
  float* rgb; float* weights; float* beta; float* beta_semantic; float* semantic_logits; float* sun_sc; float* depth;
} SnerfLossGrads;

size_t snerf_loss_workspace_bytes(const SnerfLossCfg* cfg);
int snerf_loss_partial(const SnerfLossCfg* cfg, const SnerfLossIn* in, float* totals, void* workspace,
                       size_t workspace_bytes, void* stream);
/* n_rays_global = number of rays the means run over (sum over ranks), or 0 = use the ray count that snerf_loss_partial
 * summed into `totals` (all-reduced with the other sums, so unequal shards are handled); grads are scaled by grad_scale, as the
 * last multiplication (terms are not).  Data parallelism: partial on every rank with n_rays > 0, totals summed over the ranks, finish
 * with n_rays_global = 0 on each of them == the single-GPU terms and each rank's rows of its gradients; a rank without rays makes no
 * call (n_rays <= 0 is refused) and adds zeros.  NULL members of SnerfLossGrads are skipped.
 * A label outside [0, n_classes) that is not ignore_index makes the CE term NaN (torch raises there). */
int snerf_loss_finish(const SnerfLossCfg* cfg, const SnerfLossIn* in, const float* totals, float n_rays_global,
                      float grad_scale, float* terms, const SnerfLossGrads* grads, void* stream);

/* ---- optimiser --------------------------------------------------------------------------------------
 * One fused Adam step over flat fp32 buffers (parameters, gradients, exp_avg, exp_avg_sq), replacing the reference's
 * torch.optim.Adam(lr=cfgs.pipeline.learnrate, weight_decay=0) over ~60 tensors
 * (baseline/pipelines/base_ray_pipeline.py:246-269; StepLR(gamma=0.9) is the caller's `lr`).  `step` counts from 1
 * (bias corrections 1 - beta^step, computed in double like torch does on the host); gradients are multiplied by
 * `grad_scale` first (1.0 normally).  n must be a multiple of 4, all buffers 16-byte aligned device memory. */
int snerf_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, unsigned long long n,
                    float lr, float beta1, float beta2, float eps, int step, float grad_scale, void* stream);

/* ---- DSM evaluation (altitude MAE of a digital surface model; eval/utils/dsm.py:112-266, eval/utils/dsmr.py) ----------------
 * Rasterisation is plyflatten(radius, sigma = inf) as the reference calls it (dsm.py:75-77): a point (x, y, z) has the lattice
 * cell i = floor((x - xoff)/res), j = floor((yoff - y)/res) (fp64, row 0 at the north edge) and adds z, weight 1, to every cell
 * (i+kx, j+ky), |kx|, |ky| <= radius, inside the lattice extent [0, xsize) x [0, ysize); a cell is the mean of what it received.
 * Output cell (ii, jj) of an (out_h, out_w) window is lattice cell (ioff + ii, joff + jj): the cloud-bounds grid has
 * ioff = joff = 0 and out = extent, an ROI on the same lattice a non-zero offset (= the bounds grid cropped, bit for bit). */
typedef struct SnerfDsmGrid {
  double xoff, yoff, res;
  int32_t xsize, ysize;      /* lattice extent: cells outside it receive nothing */
  int32_t ioff, joff;        /* output window origin on the lattice */
  int32_t out_w, out_h;      /* output window size */
} SnerfDsmGrid;
/* snerf_dsm_accumulate ADDS the points' contributions into count[out_h*out_w] (u32) and sum[out_h*out_w] (int64 of
 * round((z - z0)/q)): integer sums commute, so the result is bit-reproducible and data-parallel ranks combine by a SUM
 * all-reduce of both.  stats[4] (u64, zeroed by the caller, accumulated): [0] = max |round((z - z0)/q)| of the points that
 * reached the window, [1] = points whose quantised altitude is not finite or >= 2^62 in magnitude (they add nothing).
 * snerf_dsm_finish writes dsm[c] = f32(z0 + q*sum/count), NaN where count = 0, and [2] = the largest count.  The sums cannot
 * have wrapped iff stats[1] == 0 and stats[0] * stats[2] < 2^63: the caller checks this on the host. */
int snerf_dsm_accumulate(const double* xyz, int n, const SnerfDsmGrid* grid, int radius, double z0, double q,
                         unsigned* count, long long* sum, unsigned long long* stats, void* stream);
int snerf_dsm_finish(const unsigned* count, const long long* sum, long long cells, double z0, double q, float* dsm,
                     unsigned long long* stats, void* stream);
/* dsmr.downsample2x of an (h, w) image (fp32 if u_f64 == 0, else fp64) into out[ceil(h/2)][ceil(w/2)] (fp64): out[J][I] is the
 * NaN-aware mean of u[j:j+2, i:i+2] at j = min(2J+1, h-1), i = min(2I+1, w-1) -- the reference loop's last write wins */
int snerf_dsm_downsample2x(const void* u, int u_f64, int h, int w, double* out, void* stream);
/* workspace of snerf_dsm_ncc_search / snerf_dsm_shift_diff for an (h, w) image; 0 on bad arguments (radius in [0, 7]) */
size_t snerf_dsm_workspace_bytes(int h, int w, int radius);
/* dsmr.mean_std for every shift (cx + kx, cy + ky), |kx|, |ky| <= radius, of v against u (both (h, w), fp32 if f64 == 0),
 * over the pixels where u[j][i] and v[j+dy][i+dx] are both finite (out of range = NaN), all in fp64:
 * stats[s][6] = (count, sum u, sum v, sum (u-muu)^2, sum (v-muv)^2, sum (u-muu)(v-muv)), s = (ky+radius)*(2 radius+1) + kx+radius,
 * with mu = sum/count (two passes, never E[x^2] - E[x]^2); fixed-order reductions (deterministic). */
int snerf_dsm_ncc_search(const void* u, const void* v, int f64, int h, int w, int cx, int cy, int radius,
                         double* stats, void* workspace, size_t workspace_bytes, void* stream);
/* dsmr.apply_shift_ with a = 1 and compute_mae's difference: rdsm[j][i] = f32(pred[j+dy][i+dx] + b) (NaN out of range),
 * diff = rdsm - g with g = gt, or 0 where gt < -500; totals[2] = (sum |diff|, count) over the finite diff, fp64, fixed order.
 * rdsm and diff may be null (not written). */
int snerf_dsm_shift_diff(const float* pred, const float* gt, int h, int w, int dx, int dy, double b, float* rdsm,
                         float* diff, double* totals, void* workspace, size_t workspace_bytes, void* stream);

/* ---- ortho products (geo-referenced maps on the DSM lattice; eval/utils/ortho.py) ------------------------
 * The top-surface z-buffer of a UTM (east, north, alt) cloud with the colour, label or any scalar of the winning point, and
 * per-cell label votes.  The reference has no counterpart; the spec is this section and DESIGN.md section 5j, and
 * tests/ortho_numpy.py restates it in numpy integer arithmetic.
 *
 * Lattice: exactly snerf_dsm_accumulate's (SnerfDsmGrid).  A point (x, y, z) has the cell i = floor((x - xoff)/res),
 * j = floor((yoff - y)/res) in fp64 and OFFERS itself to every cell (i+kx, j+ky), |kx|, |ky| <= radius, that lies inside the
 * lattice extent [0, xsize) x [0, ysize) AND inside the output window (ioff, joff, out_w, out_h) -- also when its own cell lies
 * outside.  A point whose x or y is not finite offers nothing.  radius lies in [0, 7].  cells = out_h * out_w, row-major, row 0
 * at the north edge.
 *
 * Everything is integer arithmetic on the device (integer atomic max / add only, no float atomics), so every result is
 * bit-reproducible and independent of launch order, of how a cloud is cut into calls, of the order of the calls and of ranks.
 *
 * Refused by every entry without touching the device: null required pointers, n outside [0, 2^31], radius outside [0, 7],
 * n_classes outside [1, 255], a grid without res > 0 and positive sizes, a window that reaches beyond int32 cell indices, q not
 * positive and finite, z0 not finite, index0 < 0 or index0 + n > 2^32 - 1, cells < 1, a payload pair given by halves.
 * n = 0 is legal and launches nothing. */
#define SNERF_ORTHO_MAX_RADIUS 7
#define SNERF_ORTHO_MAX_CLASSES 255
#define SNERF_ORTHO_NO_LABEL 255   /* label_out of a cell without a winner / vote, and of a label outside [0, 254] */

/* Top-surface z-buffer.  xyz (n, 3) fp64; top[cells] (u64, ZEROED by the caller before the first call, accumulated).
 * Per point p: k = llrint((z - z0)/q) (ties to even), which must lie in [-2^31, 2^31); the key
 *   ((u64)(k + 2^31) << 32) | (0xFFFFFFFF - (index0 + p))
 * enters every offered cell by an integer atomic max: the highest quantised altitude wins and, on a tie, the LOWEST global
 * point index.  0 = no point (no valid key is 0: index0 + n <= 2^32 - 1).  Keys commute; ranks combine by a MAX all-reduce.
 * stats[4] (u64, zeroed by the caller, accumulated): [0] += points whose quantised altitude is not finite or out of range (they
 * offer nothing, whatever their x, y); [1] += points that reached at least one cell; [2], [3] reserved. */
int snerf_ortho_top(const double* xyz, long long n, long long index0, const SnerfDsmGrid* grid, int radius, double z0, double q,
                    unsigned long long* top, unsigned long long* stats, void* stream);

/* One thread per cell.  alt_out[c] = f32(z0 + q*k) (NaN when top[c] = 0) and idx_out[c] = the winner's global index (int64, -1
 * when empty) are written for every cell.  The payload outputs are written ONLY where the winner's index lies in
 * [index0, index0 + n), from row (index - index0) of the payload inputs: a fused map gathers once per image into buffers the
 * caller pre-filled.  rgb (n, 3) fp32 -> rgb_out (3, cells) fp32; labels (n) int64 -> label_out (cells) u8, a label outside
 * [0, 254] written as 255; scalar (n) fp32 -> scalar_out (cells) fp32.  Each payload pair may be NULL (both pointers). */
int snerf_ortho_gather(const unsigned long long* top, long long cells, long long index0, long long n, double z0, double q,
                       const float* rgb, const long long* labels, const float* scalar, float* alt_out, long long* idx_out,
                       float* rgb_out, unsigned char* label_out, float* scalar_out, void* stream);

/* Label votes: votes[label * cells + cell] (u32, zeroed by the caller, accumulated) += 1 for every offered cell of every point
 * whose label (int64) lies in [0, n_classes) and whose x, y are finite; z is not read.  stats[4] (u64, zeroed by the caller):
 * [0] += points with a label outside [0, n_classes) or a non-finite x or y (they vote nowhere). */
int snerf_ortho_votes(const double* xyz, const long long* labels, long long n, const SnerfDsmGrid* grid, int radius, int n_classes,
                      unsigned* votes, unsigned long long* stats, void* stream);

/* One thread per cell: label_out[c] (u8) = the class with the most votes, the LOWEST class on a tie, 255 when the cell has no
 * vote; share_out[c] = f32((double)max / (double)total), NaN when empty; stats[1] = max(stats[1], the largest total of a cell).
 * A class count cannot have wrapped iff stats[1] < 2^32: the caller checks this on the host. */
int snerf_ortho_votes_finish(const unsigned* votes, int n_classes, long long cells, unsigned char* label_out, float* share_out,
                             unsigned long long* stats, void* stream);

/* ---- SSIM (eval/utils/metrics.py: kornia's ssim map with window 3, and ssim_inria) ------------------------------------------
 * x, y: (b, c, h, w) fp32, contiguous; every (image, plane) is filtered on its own (depthwise cross-correlation) with the
 * ws x ws fp32 table weights2d (row-major, device memory), ws odd in [1, 31].  Border: SNERF_SSIM_REFLECT pads by ws / 2
 * without repeating the edge (index -1 reads 1; needs ws / 2 < h and < w, as torch's reflect pad), SNERF_SSIM_ZERO pads with
 * zeros.  In fp64 (inputs and weights exact, products exact): mu1 = K*x, mu2 = K*y, s1 = K*(x^2) - mu1^2, s2 = K*(y^2) - mu2^2,
 * s12 = K*(xy) - mu1 mu2, value = (2 mu1 mu2 + c1)(2 s12 + c2) / ((mu1^2 + mu2^2 + c1)(s1 + s2 + c2) + eps).
 * map_or_null (may be null): the values as fp32, (b, c, h, w).  per_image_sum[b] (fp64): the sum of each image's c*h*w values,
 * in a fixed order that does not depend on b (bit-reproducible; an image gives the same bits alone or in a batch). */
#define SNERF_SSIM_REFLECT 0
#define SNERF_SSIM_ZERO 1
/* fp64 partials of one launch; 0 on bad arguments (zero or too large sizes, even / out-of-range window) */
size_t snerf_ssim_workspace_bytes(int b, int c, int h, int w, int ws);
int snerf_ssim(const float* x, const float* y, int b, int c, int h, int w, int ws, int border, const float* weights2d,
               double c1, double c2, double eps, float* map_or_null, double* per_image_sum, void* workspace,
               size_t workspace_bytes, void* stream);

/* ---- semantic evaluation (eval/eval_semantic.py:65-152, semantic/components/metrics.py:11-87) -------------------------------
 * snerf_semeval_accumulate ADDS one chunk of n rays into *acc (device memory, zeroed by the caller before the first chunk):
 *   pred[n] (int64, the predicted label), gt[n] (the "semantic" target), and the optional targets gt_no_cars[n] and
 *   gt_non_corrupted[n] (NULL: that term is not accumulated); targets are uint8 (SNERF_SEMEVAL_U8) or int64 (SNERF_SEMEVAL_I64);
 *   conf[g][p] += rows with gt = g and pred = p, both in [0, n_classes) -- other rows add to out_of_range instead;
 *   errors[0] += rows with gt != pred, [1] += gt_no_cars != pred, [2] += gt_non_corrupted != pred, [3] += gt_non_corrupted != pred
 *   and gt_non_corrupted != car_idx (the reference's filter_idx: the car rows count as correct);
 *   rays += n; car_rays += rows with gt = car_idx (car_idx = -1: no car class);
 *   weights[n][n_samples], beta[n][n_samples] (fp32, given together or both NULL): beta_car_sum += the sum over the car rays
 *   of sum_s w_s beta_s, in fp64 (the fp32 products are exact) in a fixed order: one partial per workgroup in the workspace,
 *   summed by a second launch -- bit-reproducible at a fixed chunking.
 * The counts are 64-bit integer sums (exact, order-independent); data-parallel ranks combine them by a SUM all-reduce.
 * Refused: n_classes outside [1, SNERF_SEMEVAL_MAX_CLASSES], car_idx outside [-1, n_classes), n < 0, n_samples < 1 with beta,
 * a workspace smaller than snerf_semeval_workspace_bytes (needed only with beta). */
#define SNERF_SEMEVAL_MAX_CLASSES 16
#define SNERF_SEMEVAL_U8 0
#define SNERF_SEMEVAL_I64 1
typedef struct SnerfSemevalAcc {
  unsigned long long conf[SNERF_SEMEVAL_MAX_CLASSES * SNERF_SEMEVAL_MAX_CLASSES];   /* [gt][pred], row pitch 16 */
  unsigned long long errors[4];
  unsigned long long rays, car_rays, out_of_range;
  double beta_car_sum;
} SnerfSemevalAcc;
/* fp64 partials of one call; 0 on bad arguments (n_rays < 0, n_samples < 1) */
size_t snerf_semeval_workspace_bytes(int n_rays, int n_samples);
int snerf_semeval_accumulate(const long long* pred, const void* gt, const void* gt_no_cars, const void* gt_non_corrupted,
                             int label_dtype, int n, int n_classes, int car_idx, const float* weights, const float* beta,
                             int n_samples, SnerfSemevalAcc* acc, void* workspace, size_t workspace_bytes, void* stream);

/* ---- per-image visualisation maps (framework/visualize.py, baseline/components/visualize.py, semantic/components/visualize.py,
 * framework/util/other.py visualize_image_numpy) -------------------------------------------------------------------------------
 * snerf_vis_fold takes one render chunk of m rays and writes columns [row0, row0 + m) of the frame's planes; planes are planar
 * (bands, n) with frame stride n.  Every pointer of SnerfVisIn / SnerfVisOut may be NULL: its products are skipped (an output
 * given without its input is refused).
 *   per sample: weights (m, S), albedo (m, S, 3), sun (m, S, 1), sky (m, S, 3), beta (m, S, 1), beta_semantic (m, S, 1), fp32 ->
 *     albedo_map (3, n), sun_map (n), sky_map (3, n), beta_map (n), beta_semantic_map (n) = sum_s fl32(w_s f_s): the product
 *     rounded to fp32 (torch's weights.unsqueeze(-1) * factor), the sum in fp64, rounded once to fp32.  One wave per ray: lane l
 *     adds the row's floats l, l + 64, ... in ascending order, then a fixed xor butterfly over the 64 lanes.  The order depends on
 *     S alone: a ray's value does not depend on its place in the chunk, on m or on row0.  Each tensor is read once, flat.
 *   per ray: depth (m) -> depth_map (n), a copy; rgb, rgbs_gt (m, 3) -> rgb_diff (3, n) = |gt - rgb| and rgb_diff_distance (n) =
 *     sqrt((d0^2 + d1^2) + d2^2), every step fp32 and rounded once; label (m) int64 and palette (n_palette, 3) uint8 ->
 *     sem_color (3, n) uint8 = palette[label] and sem_shaded (3, n) uint8 = the fp32 product float(palette[label]) * sun_map
 *     truncated (through int32, low eight bits: plain truncation in [0, 256)); label and semantic_gt (m) uint8 (SNERF_VIS_U8) or
 *     int64 (SNERF_VIS_I64) -> sem_error (n) fp32 = clamp(|gt - label|, 0, 1).  A label outside [0, n_palette) is coloured
 *     (0, 0, 0) and adds 1 to stats->bad_labels; the palette is not read for it.
 *   stats (device memory, ZEROED by the caller before an image's first chunk): per scalar plane (SNERF_VIS_SLOT_*) the exact
 *     minimum and maximum of the values as numpy.nan_to_num makes them (NaN -> 0, +-inf -> +-FLT_MAX; -0.0 counts as +0.0), as
 *     order-preserving 64-bit keys of the value widened to fp64 (bits with the sign bit set for v >= 0, all bits inverted for
 *     v < 0), folded with integer atomic max: minmax[slot][1] = max key, minmax[slot][0] = max of the INVERTED key (= the minimum);
 *     0 = no value yet.  Exact and independent of the launch order; ranks combine them by an unsigned max.
 * snerf_vis_minmax folds the same bounds of any plane (fp32: SNERF_VIS_F32, fp64: SNERF_VIS_F64; +-inf -> +-DBL_MAX there) into
 * a slot: the fp64 altitude plane uses SNERF_VIS_SLOT_USER.
 * snerf_vis_colormap is visualize_image_numpy: x = nan_to_num(x); x = (x - mi) / (ma - mi + 1e-8); index = (255 * x) truncated to
 * uint8 (as above); out (3, n) uint8 = table[index] for a (256, 3) uint8 table.  Every step in the plane's own precision with one
 * rounding per operation.  slot >= 0: mi, ma are that slot's bounds, read on the device (an empty slot: 0, 0), and the
 * denominator is fl(fl(ma - mi) + fl(1e-8)) in the plane's type -- numpy >= 2 (NEP 50: the Python float takes the array scalars'
 * type); slot < 0: the explicit bounds lo, hi (cmap_bounds, Python floats): mi = fl(lo), denominator = fl(hi - lo + 1e-8)
 * with the sum formed in fp64.
 * All three launch on `stream`, allocate nothing and do not synchronise.  Refused without touching the device: null in / out /
 * stats / plane / table, rows outside the frame, per-sample inputs without weights, n_samples outside [1,
 * SNERF_VIS_MAX_SAMPLES], rgb without rgbs_gt or the reverse, semantic_gt / palette without label, sem_shaded without sun and
 * palette, unknown dtypes, a slot outside [0, SNERF_VIS_SLOTS), NaN explicit bounds. */
#define SNERF_VIS_MAX_SAMPLES 1024
#define SNERF_VIS_SLOTS 8
#define SNERF_VIS_SLOT_DEPTH 0
#define SNERF_VIS_SLOT_SUN 1
#define SNERF_VIS_SLOT_BETA 2
#define SNERF_VIS_SLOT_BETA_SEMANTIC 3
#define SNERF_VIS_SLOT_RGB_DIFF_DISTANCE 4
#define SNERF_VIS_SLOT_SEM_ERROR 5
#define SNERF_VIS_SLOT_USER 6
#define SNERF_VIS_U8 0
#define SNERF_VIS_I64 1
#define SNERF_VIS_F32 0
#define SNERF_VIS_F64 1
typedef struct SnerfVisIn {
  const float *weights, *albedo, *sun, *sky, *beta, *beta_semantic;
  const float *depth, *rgb, *rgbs_gt;
  const long long* label;
  const void* semantic_gt;
  const unsigned char* palette;
  int gt_dtype, n_palette;
} SnerfVisIn;
typedef struct SnerfVisOut {
  float *albedo_map, *sun_map, *sky_map, *beta_map, *beta_semantic_map;
  float *depth_map, *rgb_diff, *rgb_diff_distance;
  unsigned char *sem_color, *sem_shaded;
  float* sem_error;
} SnerfVisOut;
typedef struct SnerfVisStats {
  unsigned long long minmax[SNERF_VIS_SLOTS][2];
  unsigned long long bad_labels;
  unsigned long long reserved[7];
} SnerfVisStats;
int snerf_vis_fold(const SnerfVisIn* in, const SnerfVisOut* out, int m, int n_samples, long long row0, long long n,
                   SnerfVisStats* stats, void* stream);
int snerf_vis_minmax(const void* plane, int plane_dtype, long long n, SnerfVisStats* stats, int slot, void* stream);
int snerf_vis_colormap(const void* plane, int plane_dtype, long long n, const SnerfVisStats* stats, int slot, double lo, double hi,
                       const unsigned char* table, unsigned char* out, void* stream);

/* ---- scenes on disk: RPC rays (baseline/components/rays.py satnerf_construct, rpcm RPCModel, framework/util/conversions.py,
 * baseline/components/normalization.py StandardNormalization) --------------------------------------------------------------
 * SnerfRpc: rpcm's RPCModel as fp64 (offsets, scales; 20-term numerators / denominators in the RPC00B order
 * 1, L, P, H, LP, LH, PH, L^2, P^2, H^2, PLH, L^3, LP^2, LH^2, L^2P, P^3, PH^2, L^2H, P^2H, H^3 with L = lon, P = lat, H = alt
 * (normalised); has_inverse = 1: lat/lon_num/den hold the inverse model, evaluated with (L, P, H) = (ncol, nrow, nalt)).
 * Localisation: the inverse model when present, else rpcm's iterative inversion (start at lon = lat = -1, neighbours offset by 2
 * on the first update and 0.1 after; rpcm tests (x0 - col)^2 + (y0 - row)^2 < 1e-18 in normalised image units for ALL points of
 * a call and updates every point until the last one passes).  Reproduced in two launches: one counts the updates each point
 * needs and keeps the call's maximum, the next runs every point of the call exactly that many updates.  A point still above
 * the tolerance where rpcm raises (after 101 updates) is counted as failed; the outputs of such a call are not defined. */
typedef struct SnerfRpc {
  double row_offset, col_offset, lat_offset, lon_offset, alt_offset;
  double row_scale, col_scale, lat_scale, lon_scale, alt_scale;
  double row_num[20], row_den[20], col_num[20], col_den[20];
  double lat_num[20], lat_den[20], lon_num[20], lon_den[20];
  int has_inverse, reserved;
} SnerfRpc;
/* one image of a ray-construction launch: rays row0 .. row0 + n_rays - 1 of the output; grid mode needs w * h == n_rays */
typedef struct SnerfRayImage {
  SnerfRpc rpc;
  double min_alt, max_alt;
  long long row0, n_rays;
  int w, h;
} SnerfRayImage;
/* Rays of every image of a split in one launch.  images_host (host memory) is checked; images_dev is the same table in device
 * memory.  pixels == NULL: the image's w x h grid, ray i at row = i / w, col = i % w; else (n_rows, 2) fp64 (col, row) per output
 * row.  Per ray: localise at max_alt and at min_alt, both to custom ECEF (fp64), write the fp32 row
 * [o = near point (3), d = (far - near) / |far - near| (3), 0, |far - near|] -- un-normalised.  One rpcm call per image and
 * altitude.  counters[3 * n_images] (int, device, zeroed by the caller): [k] += points of image k whose localisation did not
 * converge; [n_images + 2k], [n_images + 2k + 1]: the update count of image k at max_alt, min_alt.
 * Refused without touching the device: null pointers, n_images outside [1, 65535], n_rows < 1, an image with no rays, rows that
 * are not contiguous in table order, a grid whose w * h overflows or differs from n_rays, min_alt >= max_alt, a zero scale, a
 * table that does not sum to n_rows. */
int snerf_rpc_rays(const SnerfRayImage* images_host, const SnerfRayImage* images_dev, int n_images, const double* pixels,
                   long long n_rows, float* rays, int* counters, void* stream);
/* rpcm localization of n points as one call (fp64 col, row, alt); normalized = 1 returns normalised lon / lat; counters[2] (int,
 * device, zeroed by the caller): [0] += failed points, [1]: the call's update count */
int snerf_rpc_localize(const SnerfRpc* rpc_host, const SnerfRpc* rpc_dev, const double* col, const double* row, const double* alt,
                       long long n, int normalized, double* lon, double* lat, int* counters, void* stream);
/* rpcm projection of n points (fp64 lon, lat, alt) to (col, row) */
int snerf_rpc_project(const SnerfRpc* rpc_host, const SnerfRpc* rpc_dev, const double* lon, const double* lat, const double* alt,
                      long long n, double* col, double* row, void* stream);
/* the depth set's keypoint errors (baseline/dataset/satnerf_depth_dataset.py:136-166): ECEF points xyz_ecef (n, 3) fp64 through
 * ecef_to_latlon_custom and the projection; err[i] = |pts2d[i] - (col, row)| (fp64); col_row (n, 2) may be NULL */
int snerf_rpc_reprojection_error(const SnerfRpc* rpc_host, const SnerfRpc* rpc_dev, const double* xyz_ecef, const double* pts2d,
                                 long long n, double* col_row, double* err, void* stream);
/* Normalisation parameters of a bank set: over the n_arrays (n_rows[a], 8) fp32 ray arrays (rays and n_rows are HOST arrays of
 * device pointers / counts), per axis the min and max of every origin and every fp32 far point o + far * d (two roundings).
 * out[13] (fp32, device): min[3], max[3], scale[3] = (max - min) / 2, offset[3] = min + scale, range = max(scale).  Exact and
 * independent of the grid (min / max commute).  workspace: snerf_ray_bounds_workspace_bytes (0 on bad arguments). */
size_t snerf_ray_bounds_workspace_bytes(const long long* n_rows, int n_arrays);
int snerf_ray_bounds(const float* const* rays, const long long* n_rows, int n_arrays, float* out, void* workspace,
                     size_t workspace_bytes, void* stream);
/* In place, fp32, correctly rounded: row[0..2] = (row[0..2] - c) / range and, with bounds = 1, row[6] /= range, row[7] /= range.
 * center_range (device): c[3], range -- out + 9 of snerf_ray_bounds.  stride >= 8 with bounds, >= 3 without. */
int snerf_normalize_rows(float* rows, long long n, int stride, int bounds, const float* center_range, void* stream);

/* ---- world clouds: rays + depth -> UTM (east, north, alt), and UTM points back into the scene (eval/utils/dsm.py get_utm_cloud, baseline/dataset/satnerf_dataset.py
 * get_latlonalt_from_nerf_prediction, StandardNormalization.denormalize, framework/util/conversions.py) ----------------------
 * One launch, one thread per point, every step fp64 with one rounding per operation (no contraction):
 *   1. xyz_n = o + d * depth, the fp32 ray columns 0..2 / 3..5 and the fp32 depth widened first (rays.double());
 *   2. ECEF = xyz_n * range + centre (denormalize on an fp64 tensor; centre and range carry fp32 values);
 *   3. ecef_to_latlon_custom -> lat, lon (degrees), alt;
 *   4. the utm package's from_latlon series (K0 = 0.9996, E = 0.00669438, R = 6378137) about the central meridian lon0 (radians),
 *      + 1e7 on the northing when south = 1.  The package is not part of this build: parity with it is UNPINNED.
 * enu_out (n, 3) fp64: (east, north, alt); lla_out (n, 3) fp64 or NULL: (lat deg, lon deg, alt).
 * stats: 8 64-bit words the CALLER initialises to {~0, 0, ~0, 0, 0, 0, 0, 0}: [0] / [1] the minimum / maximum east and [2] / [3]
 * the minimum / maximum north over the finite points as an order-preserving key of the double (bits with the sign bit set for
 * v >= 0, all bits inverted for v < 0), folded with integer atomics -- exact and independent of the launch order; a word left
 * at its initial value means no finite point; [4] += points whose east, north or alt is not finite (written as they come,
 * left out of the bounds); [5..7] reserved.  n = 0 is legal and launches nothing.
 * Refused without touching the device: null pointers (lla_out excepted), n outside [0, 2^31], ray_stride < 6, a range that is not
 * positive and finite, a centre that is not finite, lon0 outside [-pi, pi], south other than 0 / 1, a direction other than the
 * two below, and SNERF_GEO_TO_SCENE given to snerf_geo_cloud.
 *
 * params->direction selects the way through the same steps:
 *   SNERF_GEO_TO_WORLD (0): scene -> world, the steps above.
 *   SNERF_GEO_TO_SCENE (1): world -> scene, snerf_geo_points only.  Its input array (`xyz_n` in the prototype) holds (n, 3) fp64
 *     (east, north, alt) in the zone of lon0 / south; per point
 *       1. the utm package's to_latlon series (the same constants; restated, parity with the package UNPINNED) -> lat, lon (degrees);
 *       2. latlon_to_ecef_custom(lat, lon, alt);
 *       3. xyz_n = (ECEF - centre) / range, two roundings per component (normalize_xyz on an fp64 tensor).
 *     enu_out receives xyz_n (n, 3) fp64; lla_out, when not NULL, (lat deg, lon deg, alt).  stats as above over the OUTPUT: [0..3]
 *     the bounds of scene x and scene y, [4] += points whose xyz_n is not finite. */
#define SNERF_GEO_TO_WORLD 0
#define SNERF_GEO_TO_SCENE 1
typedef struct SnerfGeoParams {
  double centre[3];
  double range;
  double lon0;
  int south, direction;
} SnerfGeoParams;
int snerf_geo_cloud(const float* rays, int ray_stride, const float* depth, long long n, const SnerfGeoParams* params,
                    double* enu_out, double* lla_out, unsigned long long* stats, void* stream);
/* direction 0: the same kernel entered at step 2, xyz_n (n, 3) fp64 normalised points; direction 1: world -> scene, see above */
int snerf_geo_points(const double* xyz_n, long long n, const SnerfGeoParams* params, double* enu_out, double* lla_out,
                     unsigned long long* stats, void* stream);

/* ---- cast shadows on the DSM lattice: the shadow a height field casts under a sun, and the agreement of a learned shadow map
 * with it.  A map product of this project (the reference has no counterpart); DESIGN.md section 5o. ------------------------------
 * snerf_shadow_cast: one thread per (cell, sun) marches from the cell towards the sun over the height field.
 *   dsm (h, w) fp32, device memory, row 0 = the north edge (as everywhere on the lattice), NaN = a hole.
 *   suns_host (n_suns, 3) fp64 in HOST memory, one row (ux, uy, rise) per sun: ux = sin(azimuth) (towards the sun, east = +column),
 *     uy = -cos(azimuth) (north = -row), rise = tan(elevation) * res, the metres a ray climbs per cell of horizontal travel.  The
 *     rows are checked and go to the kernel BY VALUE in its arguments: no device table, no copy, nothing read after the call
 *     returns.  1 <= n_suns <= SNERF_SHADOW_MAX_SUNS.
 *   bias (metres) is added to the start altitude; z_top (metres, may be +inf) ends a march early.
 *   lit_out (n_suns, h, w) u8: 0 = shadowed, 1 = lit, SNERF_SHADOW_UNKNOWN = the start cell is NaN.
 *   dist_out (n_suns, h, w) fp32 or NULL: the horizontal distance to the blocking cell in CELLS; NaN where lit or unknown.
 * The march is an Amanatides-Woo walk in cell units; every step fp64 with one rounding per operation (no contraction), only
 * + - * / and comparisons -- the host evaluates every transcendental -- so an fp64 restatement reproduces it bit for bit:
 *   start at (i + 0.5, j + 0.5) with h0 = (double)dsm[j][i] + bias;
 *   stepx = ux > 0 ? 1 : -1, tDeltaX = 1 / |ux| (+inf when ux == 0), tMaxX = 0.5 * tDeltaX; the same for y;
 *   each step: if tMaxX <= tMaxY then t = tMaxX, i += stepx, tMaxX += tDeltaX, else the y analogue -- ON A TIE X STEPS FIRST and
 *     the next step takes y at the same t;
 *   after each step the first of these that holds ends the march:
 *     a. (i, j) outside [0, w) x [0, h)                -> lit;
 *     b. hr = h0 + rise * t, hr > z_top                -> lit;
 *     c. (double)dsm[j][i] > hr                        -> shadowed, dist = (float)t (a NaN cell never blocks: the comparison is false).
 *   The start cell is never tested.  At most h + w + 2 steps occur.  z_top is only an early exit: with z_top >= the largest finite
 *   altitude the result is the one under +inf.
 * Refused without touching the device: null dsm / suns_host / lit_out, h or w < 1 or h * w >= 2^31, n_suns outside
 * [1, SNERF_SHADOW_MAX_SUNS], a sun row that is not finite, whose ux^2 + uy^2 is more than 1e-9 from 1, or with rise <= 0, a bias that
 * is not finite, a NaN z_top. */
#define SNERF_SHADOW_MAX_SUNS 64
#define SNERF_SHADOW_UNKNOWN 255
int snerf_shadow_cast(const float* dsm, int h, int w, const double* suns_host, int n_suns, double bias, double z_top,
                      unsigned char* lit_out, float* dist_out, void* stream);

/* snerf_shadow_agreement: n_suns learned shadow maps against n_suns cast masks in one launch.
 *   sun (n_suns, cells) fp32; lit (n_suns, cells) u8 (snerf_shadow_cast's lit_out); valid (cells) u8 or NULL (0 = leave the cell out);
 *   a cell is predicted lit when sun >= threshold.
 *   acc (n_suns, 8) u64, ZEROED by the caller, accumulated; the words of a sun's row:
 *     [0] += lit and predicted lit       [1] += lit and predicted shadow
 *     [2] += shadow and predicted lit    [3] += shadow and predicted shadow
 *     [4] += cells left out: lit == SNERF_SHADOW_UNKNOWN (or any value other than 0 / 1), valid == 0, or sun not finite
 *     [5] += llrint(sun * 2^24) over the counted lit cells, [6] the same over the counted shadow cells -- int64 sums in two's
 *            complement (the DSM rasteriser's quantised sums); the product is exact, ties round to even, and it is clamped to
 *            +-2^62 first (a shadow map lies in [0, 1]: the clamp only keeps the conversion defined)
 *     [7] reserved, not written.
 * Integer atomics only: the words do not depend on launch order, on how a map is cut into calls, or on ranks (a SUM all-reduce
 * combines them).
 * Refused without touching the device: null sun / lit / acc, cells < 1, n_suns outside [1, SNERF_SHADOW_MAX_SUNS], a threshold that
 * is not finite. */
int snerf_shadow_agreement(const float* sun, const unsigned char* lit, const unsigned char* valid, long long cells, int n_suns,
                           double threshold, unsigned long long* acc, void* stream);

/* ---- per-ray kernels outside the render pass: importance resampling of the depths and the distortion
 * loss on a ray's weights (section 5r).  One wave per ray; both are exact (fp64 operations rounded one by one, integer sums) and
 * have a numpy restatement under tests/. ------------------------------------------------------------------------------------- */
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

/* ---- measurement hook ----------------------------------------------------------------------------
 * Between snerf_profile_begin and snerf_profile_end every GEMM launch is bracketed by HIP events on the
 * stream it is launched on; _end synchronises those events and returns, per kernel variant, the summed
 * device time, the algorithmic FLOPs (2*I*J*K of each launch) and the launch count.
 * variant 0: K-contiguous GEMMs (forward X.W^T and dX = dZ.(W^T)^T): gemm_kc_kernel of bsp_kc.hip (128x256 tile),
 *         1: the SIREN trunk as one persistent launch (trunk_kernel of bsp_trunk.hip; one-plane mode),
 *         2: dW = dZ^T.X (both operands read along the points, split over the points): gemm_dw_kernel (256x256 tile),
 *         3: the 32-wide head variants (gemm_kcn_kernel, gemm_dw_kernel<32>). */
#define SNERF_PROFILE_VARIANTS 4
typedef struct SnerfProfile {
  double ms[SNERF_PROFILE_VARIANTS];
  double flops[SNERF_PROFILE_VARIANTS];
  int64_t launches[SNERF_PROFILE_VARIANTS];
} SnerfProfile;
int snerf_profile_begin(void);
int snerf_profile_end(SnerfProfile* out);

/* test hooks of the block-scaled fp16-plane kernels (csrc/bsp.h): fp32 in / fp32 out around one launch; `planes` = 2 (default
 * arithmetic) or 1 (SNERF_FLAG_F16X1); synchronous and allocating -- tests only */
int snerf_test_set_kc_grid(int n_workgroups);   /* persistent grid of the K-contiguous launches (0: two per CU): forces the tile loop at test sizes */
int snerf_test_set_trunk_fusion(int on);        /* 0: launch-per-layer trunk for every pass; 1 (default): one-plane passes of the W = 512 SIREN model
                                                 * run the trunk as ONE persistent launch (csrc/bsp_trunk.hip) */
int snerf_test_bsp_roundtrip(const float* src, int rows, int cols, int ld, int col0, float* dst, int* exps_out, int planes, void* stream);
int snerf_test_bsp_kc(const float* A, const float* A2, int Ka, const float* W, const float* bias, int I, int J, int K, int a_col0,
                      int c_col0, int act, float w0, int aux_mode, const float* Hact, const unsigned* Hsign, float* C,
                      unsigned* Csign, float* colsum, const float* nd_w, float* nd_out, const int* nd_rows, int narrow, int planes, void* stream);
/* nd_w [J] / nd_out [ceil(J/256)*4][I]: the folded 1-wide projection of ACT_SIN launches; with nd_rows (HOST array, one count <= 5 per
 * 256-column tile): nd_w [sum nd_rows][J], nd_out [ceil(J/256)*4*5][I] -- the folded final head layers */
int snerf_test_bsp_dw(const float* A, int lda_src, const float* B, int ldb_src, int P, int I, int J, int a_col0, int b_col0,
                      int k_split, int narrow_i, float* C, int planes, void* stream);
/* planes = 0: no plane tensors -- one launch of the small fp32 GEMM on the WEIGHTS of the composed first head layer, with the job table
 * the pack (narrow_i = 0: compose) / a backward pass (narrow_i = 1: un-compose) builds; I = rows of the layer or of a row block of it,
 * J = FA, P = W; A, B, C: concatenated fp32 operands (csrc/test_hooks.hip lists them) */

#ifdef __cplusplus
}
#endif
#endif /* SNERF_HIP_H */
