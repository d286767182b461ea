// C-ABI of libsnerf_hip.so (include/snerf_hip.h): layout plan, parameter packing and the entry points of one rendering
// pass (its launch sequences: bsp_pass.hip; the single-kernel test hooks: test_hooks.hip).
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>

#include "aux_kernels.h"
#include "bsp.h"
#include "composite.h"
#include "gemm.h"
#include "plan.h"

namespace snerf {

// bsp_pass.hip: the pass sequences of the default arithmetic (block-scaled fp16-plane activations)
int forward_bsp(const Plan& p, const float* pk, const SnerfInputs* in, const SnerfOutputs* out, void* workspace, hipStream_t st);
int backward_bsp(const Plan& p, const float* pk, const SnerfInputs* in, const SnerfOutGrads* go, float* gp, float* d_t, float* d_t_s,
                 void* workspace, hipStream_t st);

static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

// ---------------------------------------------------------------------------------------------------
// plan
// ---------------------------------------------------------------------------------------------------
// split-K choice for the plane dW kernel: 256 x 256 tiles, one workgroup per CU -> tiles x splits ~ 256 (ONE round of
// the chip: every workgroup writes a 256 KB slab, so the slab traffic of a launch is 64 MB however the matrix is shaped;
// two rounds doubled it and the reduction that follows), splits of whole 128-point exponent blocks, <= 16384 points each
DwSplit dw_choose_bsp(int P, int rows, int cols, bool narrow_rows) {
  const int tiles = (narrow_rows ? 1 : (rows + 255) / 256) * ((cols + 255) / 256);
  int ns = (256 + tiles / 2) / tiles;
  const int ns_max = P / 1024 > 1 ? P / 1024 : 1;
  if (ns > ns_max) ns = ns_max;
  if (ns < 1) ns = 1;
  DwSplit d;
  d.k_split = round_up((P + ns - 1) / ns, 128);
  if (d.k_split > 16384) d.k_split = 16384;
  d.ns = (P + d.k_split - 1) / d.k_split;
  return d;
}

// ---- block-scaled plane layout: weight operand packs + workspace -------------------------------------------
// Weight operands: every K-contiguous GEMM's B as a WF16 pack behind the fp32 region (csrc/bsp.h).  Each operand is named ONCE here:
// its fp32 master [m_rows][m_cols] at float offset src (leading dimension ld), read as it lies or transposed.  The pack kernels
// (snerf_pack_params) and the launches (bsp_pass.hip: weights) both read this table.  A matrix and its transposes share exponent slot e.
static void plan_weights(Plan& p) {
  size_t off = 0;
  int ne = 0;
  p.wj.n = 0;
  auto op = [&](int e, size_t src, int ld, int m_rows, int m_cols, int transposed = 0) {
    bsp::WPackJob& w = p.wj.j[p.wj.n];
    w.src_off = src; w.src_ld = ld; w.transposed = transposed; w.m_rows = m_rows; w.m_cols = m_cols;
    w.rows = transposed ? m_cols : m_rows; w.K = transposed ? m_rows : m_cols;    // operand(r, k) = master(k, r) when transposed
    w.dst_off = off; w.e_idx = e;
    off += bsp::wp16_bytes(w.rows, w.K, p.pl);
    return p.wj.n++;
  };
  const int W = p.W, H = p.H;
  if (p.compose_feats) {
    // The first head layer's two operands come from the composed matrix, a pack-time fp32 scratch: W_c [N1][FA] and, behind it, the 32
    // sigma rows (columns [0, W)), so that the transposed pack serves the merged dX launch  dz_last = [dz1 | d sigma] [W_c[:, :W]; w_sigma]
    // at k = N1 (the sun block is the last of W_c: the sc pass reads k from sun_col on).  The scratch lies under the packs of the other
    // operands, which are written after these two have been packed from it.
    const int e1 = ne++, e2 = ne++;   // an exponent each: the transposed operand's matrix has the sigma rows, the plain one's has not
    p.wj_h1 = op(e1, 0, p.FA, p.N1, p.FA);
    p.wj_th1 = op(e2, 0, p.FA, p.N1 + NARROW, p.FA, 3);
    p.wj_first = p.wj.n;
    p.o_wc = p.n_fp32 + round_up_sz(off, 256) / 4;
    p.wj.j[p.wj_h1].src_off = p.wj.j[p.wj_th1].src_off = p.o_wc;
  }
  for (int i = 0; i < p.L; ++i) {   // the transpose of a skip layer [gamma | h]: its h columns only (dX of the layer below)
    const int e = ne++;
    p.wj_tr[i] = op(e, p.w_tr[i], p.k_tr[i], W, p.k_tr[i]);
    p.wj_tt[i] = i > 0 ? op(e, p.w_tr[i] + (((p.skip_mask >> i) & 1u) ? p.Ep : 0), p.k_tr[i], W, W, 1) : -1;
  }
  if (p.compose_feats) { p.wj_fs = p.wj_tfs = -1; p.wj_sig = op(ne++, p.w_fs + (size_t)W * W, W, NARROW, W); }
  else {
    { const int e = ne++; p.wj_fs = op(e, p.w_fs, W, W, W); p.wj_sig = op(e, p.w_fs + (size_t)W * W, W, NARROW, W); p.wj_tfs = op(e, p.w_fs, W, W + NARROW, W, 1); }
    { const int e = ne++; p.wj_h1 = op(e, p.w_h1, p.FA, p.N1, p.FA); p.wj_th1 = op(e, p.w_h1, p.FA, p.N1, p.FA, 1); }
  }
  { const int e = ne++; p.wj_s2 = op(e, p.w_s2, H, H, H); p.wj_ts2 = op(e, p.w_s2, H, H, H, 1); }
  { const int e = ne++; p.wj_s3 = op(e, p.w_s3, H, H, H); p.wj_ts3 = op(e, p.w_s3, H, H, H, 1); }
  { const int e = ne++; p.wj_s4 = op(e, p.w_s4, H, NARROW, H); p.wj_ts4 = op(e, p.w_s4, H, NARROW, H, 1); }
  { const int e = ne++; p.wj_fin = op(e, p.w_fin, p.KF, NARROW, p.KF); p.wj_tfin = op(e, p.w_fin, p.KF, NARROW, p.KF, 1); }
  if (p.compose_feats) {   // the scratch may reach beyond the last pack (narrow trunks under wide heads)
    const size_t end = (p.o_wc - p.n_fp32) * 4 + (size_t)(p.N1 + NARROW) * p.FA * 4;
    if (end > off) off = end;
  }
  p.wp_bytes = round_up_sz(off, 256);
  p.packed_floats = p.n_fp32 + (p.wp_bytes + 2 * bsp::WPACK_MAX * 4 + 256) / 4;
  if (p.compose_feats) { p.o_bc = p.packed_floats; p.packed_floats += round_up_sz(p.N1, 64); }
}

static void plan_bsp(Plan& p) {
  // workspace: activations as planes (4 bytes per element, like fp32; 2 with one plane) + exponent tables + sign words
  size_t wo = 0;
  auto wtake = [&](size_t bytes) { size_t o = wo; wo += round_up_sz(bytes, 256); return o; };
  const size_t Pp = p.Pp;
  auto planes = [&](int ld) { return wtake(bsp::plane_bytes(Pp, ld, p.pl)); };
  auto etab = [&](int ld) { return wtake(bsp::etab_ints(Pp, ld) * 4); };
  // one plane tensor [Pp][ld]: planes, exponent table, sign words (SIREN training passes keep them for the activations)
  auto tensor = [&](int ld, bool sign = false) {
    PlaneT t;
    t.o = planes(ld); t.e = etab(ld); t.s = sign ? wtake(bsp::sign_words(Pp, ld) * 4) : 0; t.ld = ld;
    return t;
  };
  const bool keep_c = p.train && p.siren;
  p.h1w = p.sc ? p.H : p.N1;
  // A geometry pass (SNERF_FLAG_GEOMETRY) plans only what it writes: the depths, the encoding, the two trunk buffers, sigma's partials or
  // buffer and the tile counters.  Its last trunk layer leaves into the trunk buffer whose turn it is, also in a composed plan (whose
  // full pass sends it into the [h_last | extras] tensor): there is no head to read it.
  const bool geo = p.geometry;
  p.o_z = wtake(((size_t)p.P + 4) * 4);
  if (!geo) {
    p.o_T = wtake((size_t)p.P * 4);
    p.o_rgbraw = wtake((size_t)p.N * 3 * 4);
  }
  p.pe = tensor(p.Ep);
  if (p.train) {
    for (int i = 0; i < p.L - (p.compose_feats ? 1 : 0); ++i) p.h[i] = tensor(p.W, keep_c);
  } else {   // inference keeps no layer: two buffers in turn
    PlaneT a, b;
    a.ld = b.ld = p.W;
    a.o = planes(p.W); b.o = planes(p.W); a.e = etab(p.W); b.e = etab(p.W);
    for (int i = 0; i < p.L; ++i) p.h[i] = (i & 1) ? b : a;
  }
  if (!geo) p.fa = tensor(p.FA);
  if (p.compose_feats && !geo) {
    // The last trunk layer stores its planes where feats went: columns [0, W) of the [P][FA] tensor, so that the first head layer reads
    // [h_last | extras] as it read [feats | extras] -- no pass over memory added.  h[L - 1] is that tensor at leading dimension FA
    // (its sign words, for a SIREN training pass, are laid out for FA columns).
    p.h[p.L - 1] = p.fa;
    p.h[p.L - 1].s = keep_c ? wtake(bsp::sign_words(Pp, p.FA) * 4) : 0;
  }
  if (!geo) {
    p.h1 = tensor(p.h1w, keep_c);
    p.s2 = tensor(p.H, keep_c);
    p.s3 = tensor(p.H, keep_c);
  }
  // the narrow projections: folded into the producing SIREN launch's epilogue where its width is whole 256-column tiles (partial sums
  // per wave, summed by the composite), otherwise a 32-wide fp32 buffer written by a launch of their own
  p.nd_sig = p.siren && p.W % 256 == 0 && p.W <= 1024;
  p.nd_sun = p.siren && p.H % 256 == 0 && p.H <= 1024;
  p.nd_fin = !p.sc && p.siren && p.H == 256 && p.C <= ND_FIN;   // one 256-column tile per head block, at most ND_FIN outputs per block
  {  // bsp_trunk.hip: the shapes it is written for (launch_trunk checks them again)
    bool ok = p.pl == 1 && p.siren && p.nd_sig && p.W == 512 && p.Ep == 64 && p.L >= 3 && p.L <= bsp::TR_MAXL &&
              !(p.skip_mask & 1u) && (p.skip_mask >> (p.L - 1)) == 0u && !bsp::trunk_dma_in_final_layer(p.L, p.skip_mask, /*feats_fused=*/!p.train && !geo);   // (bsp_pass.hip: fused_feats)
    for (int i = 0; ok && i < p.L; ++i) ok = p.k_tr[i] == (i == 0 ? 64 : (((p.skip_mask >> i) & 1u) ? 576 : 512));
    p.fuse_trunk = ok;
  }
  if (p.nd_sig) p.o_sigpart = wtake((size_t)4 * (p.W / 256) * Pp * 4); else p.o_sigo = wtake(Pp * NARROW * 4);
  if (!geo) {
    if (p.nd_sun) p.o_sunpart = wtake((size_t)4 * (p.H / 256) * Pp * 4); else p.o_suno = wtake(Pp * NARROW * 4);
    if (p.nd_fin) p.o_finpart = wtake((size_t)4 * (p.KF / 256) * ND_FIN * Pp * 4); else if (!p.sc) p.o_fino = wtake(Pp * NARROW * 4);
  }
  p.o_kcq = wtake((size_t)KCQ_SLOTS * 64);
  p.comp_blocks = composite_bwd_blocks(p.N);
  if (p.train) {
    int maxw = p.W > p.FA ? p.W : p.FA;   // widest gradient tensor: dza / dzb hold [h1w], [W] and [FA] ones in turn
    if (p.h1w > maxw) maxw = p.h1w;
    auto scratch = [&](int w) { PlaneScratch t; t.o = planes(w); t.e = etab(w); t.maxw = w; return t; };
    p.dza = scratch(maxw);
    p.dzb = scratch(maxw);
    p.dsa = tensor(p.H);
    p.dsb = tensor(p.H);
    p.o_dsig = wtake(Pp * NARROW * 4); p.o_dfin = wtake(Pp * NARROW * 4); p.o_dsun = wtake(Pp * NARROW * 4);
    p.pdsig = tensor(NARROW);
    p.pdfin = tensor(NARROW);
    p.pdsun = tensor(NARROW);
    p.rq_floats = bsp_rq_floats(p);
    p.o_rq = wtake(p.rq_floats * 4);
    p.o_skyslab = wtake((size_t)p.comp_blocks * 4 * p.sky_floats * 4);
  }
  p.ws_bytes = wo;
}

int make_plan(const SnerfDesc* d, Plan* pl) {
  if (!d || !pl) { set_error("null descriptor"); return SNERF_ERR_NULL; }
  Plan& p = *pl;
  auto bad = [&](const char* why) { set_error("bad SnerfDesc: %s", why); return SNERF_ERR_BAD_DESC; };
  if (d->n_rays <= 0 || d->n_samples <= 0) return bad("n_rays and n_samples must be positive");
  if ((long long)d->n_rays * d->n_samples > (1ll << 30)) return bad("n_rays * n_samples too large for one pass (chunk the rays)");
  if (d->fc_layers < 1 || d->fc_layers > SNERF_MAX_LAYERS) return bad("fc_layers out of range");
  if (d->fc_units < 16 || (d->fc_units & 15)) return bad("fc_units must be a positive multiple of 16");
  if (d->feat_last < 8 || (d->feat_last & 7) || d->feat_last > 64 * MAX_SKY_UNITS) return bad("feat_last must be a multiple of 8, <= 512");
  if (d->n_freq < 0 || d->n_freq > 16) return bad("n_freq out of range");
  if (d->t_dim < 1 || d->t_dim > 16) return bad("t_dim out of range");
  if (d->n_classes < 0 || d->n_classes > MAX_CLASSES) return bad("n_classes out of range");
  if (d->skip_mask & 1u) return bad("layer 0 cannot be a skip layer");
  p.N = d->n_rays; p.S = d->n_samples; p.P = p.N * p.S; p.Pp = round_up(p.P, 128);
  p.W = d->fc_units; p.H = d->feat_last; p.L = d->fc_layers; p.F = d->n_freq;
  {  // arithmetic: none of the bits = the default (SNERF_FLAG_F16X2), for C and Python callers alike
    const unsigned sel = d->flags & (SNERF_FLAG_F16X2 | SNERF_FLAG_F16X1);
    if (sel == (SNERF_FLAG_F16X2 | SNERF_FLAG_F16X1)) return bad("more than one arithmetic flag (SNERF_FLAG_F16X2 / SNERF_FLAG_F16X1)");
    p.pl = (sel & SNERF_FLAG_F16X1) ? 1 : 2;
  }
  // raw xyz (n_freq = 0: SatNeRF) as ONE fp16 plane: the coordinates enter the w0 = 30 first layer rounded to 11 bits, which alone
  // moves sigma by 4e-3 (fp64 oracle with fp16-rounded xyz) -- beyond the mode's 5e-3 output bar once the other layers' rounding adds
  // in (measured 5.0e-3).  Refused rather than computed at that accuracy (tests/test_abi_cpu.py, tests/test_gpu_geometry.py).
  if (p.pl == 1 && p.F == 0) return bad("SNERF_FLAG_F16X1 with raw xyz input (n_freq = 0) is not supported: one fp16 plane rounds the coordinates to 11 bits; use the default arithmetic");
  p.E = p.F > 0 ? 6 * p.F : 3; p.Ep = round_up(p.E, p.pl == 2 ? 32 : 64);  // LDS stages (128 bytes per row: 32 / 64 k) never straddle the [gamma | h] segments
  p.tau = d->t_dim; p.C = d->n_classes;
  p.siren = d->siren != 0; p.sem_sigmoid = d->sem_sigmoid != 0;
  p.train = (d->flags & SNERF_FLAG_TRAIN) != 0; p.sc = (d->flags & SNERF_FLAG_SC_PASS) != 0;
  p.relight = (d->flags & SNERF_FLAG_RELIGHT) != 0;
  p.embed_grad = (d->flags & SNERF_FLAG_EMBED_GRAD) != 0;
  p.geometry = (d->flags & SNERF_FLAG_GEOMETRY) != 0;
  p.depth_median = (d->flags & SNERF_FLAG_DEPTH_MEDIAN) != 0;
  // The median depth is read off the weights an INFERENCE composite wrote along the camera ray: it has no gradient (nothing of it is
  // kept for a backward), and the solar-correction pass has no depth.  One wave holds a ray's run totals: the per-ray sample limit.
  if (p.depth_median && (p.train || p.sc || p.embed_grad))
    return bad("SNERF_FLAG_DEPTH_MEDIAN cannot be combined with SNERF_FLAG_TRAIN, SNERF_FLAG_SC_PASS or SNERF_FLAG_EMBED_GRAD (it rewrites the depth of an inference, geometry or relight pass)");
  if (p.depth_median && d->n_samples > SNERF_VIS_MAX_SAMPLES)
    return bad("SNERF_FLAG_DEPTH_MEDIAN needs n_samples in [1, SNERF_VIS_MAX_SAMPLES = 1024]");
  // A geometry pass is an inference pass of its own kind: nothing of it is kept for a backward, it samples along the camera ray, and it
  // leaves no head tensor a relight could reuse.
  if (p.geometry && (p.train || p.sc || p.relight || p.embed_grad))
    return bad("SNERF_FLAG_GEOMETRY cannot be combined with SNERF_FLAG_TRAIN, SNERF_FLAG_SC_PASS, SNERF_FLAG_RELIGHT or SNERF_FLAG_EMBED_GRAD (it is an inference pass without heads)");
  // The embedding-only backward follows a training forward: it reads the activations that one keeps.  Sizes and forward are the TRAIN plan's.
  if (p.embed_grad && (p.relight || !p.train)) return bad("SNERF_FLAG_EMBED_GRAD is valid only together with SNERF_FLAG_TRAIN, and not with SNERF_FLAG_RELIGHT (it selects the backward of a training pass)");
  // A relight reuses what an INFERENCE MAIN pass left: a training workspace has another layout, the solar-correction pass samples along
  // the sun ray itself (nothing of it survives a new sun).  The plan of a relight is otherwise that of its base pass, sizes included.
  if (p.relight && (p.train || p.sc)) return bad("SNERF_FLAG_RELIGHT cannot be combined with SNERF_FLAG_TRAIN or SNERF_FLAG_SC_PASS (a relight follows an inference main pass)");
  p.skip_mask = d->skip_mask;
  const bool sem = p.C > 0;
  const bool sbeta = sem && d->use_separate_beta_for_s;
  const bool sep_ts = sem && d->use_separate_tj_for_semantic;
  p.rgb_t = sem && d->use_tj_instead_of_beta;
  p.sem_t = sem && d->use_tj_for_s && !sep_ts;
  p.sem_ts = sem && d->use_tj_for_s && sep_ts;
  p.sbeta_ts = sbeta && sep_ts;
  p.x_sun = 0; p.x_t = 3; p.x_ts = sep_ts ? 3 + p.tau : -1;
  p.Xp = round_up(3 + p.tau + (sep_ts ? p.tau : 0), 16);  // FA % 16 == 0: weight planes are stored in 16-k tiles
  if ((p.H & 15) || (p.W & 31) || p.Xp != 16) return bad("fc_units % 32 == 0, feat_last % 16 == 0 and 3 + t_dim (x2 with separate t_s) <= 16 are required");
  if (p.pl == 1 && ((p.W & 63) || (p.H & 31))) return bad("SNERF_FLAG_F16X1 needs fc_units % 64 == 0 and feat_last % 32 == 0 (LDS stages of 64 columns)");
  p.Wf = round_up(p.W, 128);         // extras block on an exponent-block boundary
  p.FA = p.Wf + p.Xp;
  int nb = 0;
  p.blk_rgb = nb++;
  p.blk_sem = sem ? nb++ : -1;
  p.blk_beta = nb++;
  p.blk_sbeta = sbeta ? nb++ : -1;
  p.blk_sun = nb++;
  p.nblk = nb;
  p.KF = (nb - 1) * p.H;
  p.KF = round_up(p.KF, 128);           // sun block on an exponent-block boundary (pad rows / columns are zero)
  p.sun_col = p.KF;
  p.N1 = p.KF + p.H;

  size_t off = 0;
  auto take = [&](size_t n) { size_t o = off; off += round_up_sz(n, 64); return o; };
  for (int i = 0; i < p.L; ++i) {
    p.k_tr[i] = (i == 0) ? p.Ep : (((p.skip_mask >> i) & 1u) ? p.Ep + p.W : p.W);
    p.w_tr[i] = take((size_t)p.W * p.k_tr[i]);
    p.b_tr[i] = take(p.W);
  }
  p.w_fs = take((size_t)(p.W + NARROW) * p.W); p.b_fs = take(p.W + NARROW);
  p.w_h1 = take((size_t)p.N1 * p.FA); p.b_h1 = take(p.N1);
  p.w_s2 = take((size_t)p.H * p.H); p.b_s2 = take(p.H);
  p.w_s3 = take((size_t)p.H * p.H); p.b_s3 = take(p.H);
  p.w_s4 = take((size_t)NARROW * p.H); p.b_s4 = take(NARROW);
  p.w_fin = take((size_t)NARROW * p.KF); p.b_fin = take(NARROW);
  p.sky_floats = 9 * p.H + 4;
  p.sky = take(p.sky_floats);
  p.n_fp32 = off;
  {  // SNERF_COMPOSE_FEATS=0: the separate feats layer.  The merged dX launch reads [dz1 | d sigma] as two A segments, the first a whole
     // number of 32-column LDS stages: h1w % 32 == 0, that is feat_last % 32 == 0 (KF is a multiple of 128), and contracts N1 + 32 columns
     // in the main pass, within the K-contiguous kernel's 2048 (its exponent table along k: feat_last = 512 with four blocks has
     // N1 = 2048).  Other shapes stay separate.  The condition reads the model's dimensions only: pack, main and sc pass decide alike.
    const char* ev = getenv("SNERF_COMPOSE_FEATS");
    p.compose_feats = p.pl == 2 && (p.H & 31) == 0 && p.N1 + NARROW <= 2048 && !(ev && ev[0] == '0' && ev[1] == 0);
  }
  if (!p.compose_feats) { plan_weights(p); plan_bsp(p); return SNERF_OK; }
  // A composed plan reports no smaller buffers than the separate plan of the same descriptor: buffers sized under either setting of the
  // switch serve both.  Both layouts are planned for that (two walks of host arithmetic over ~20 tensors and ~30 pack jobs per API
  // call, no device work): simple, and small beside the ~40 launches a call queues.
  Plan q = p;
  q.compose_feats = false;
  plan_weights(q);
  plan_bsp(q);
  plan_weights(p);
  plan_bsp(p);
  if (q.packed_floats > p.packed_floats) p.packed_floats = q.packed_floats;
  if (q.ws_bytes > p.ws_bytes) p.ws_bytes = q.ws_bytes;
  return SNERF_OK;
}

// ---------------------------------------------------------------------------------------------------
// pack / unpack tables
// ---------------------------------------------------------------------------------------------------
struct TableBuilder {
  CopyTable tabs[4];
  int nt = 0;
  bool missing = false;
  TableBuilder() { memset(tabs, 0, sizeof(tabs)); nt = 1; }
  void add(float* user, int user_ld, int rows, int cols, size_t dst_off, int dst_ld) {
    if (!user) { missing = true; return; }
    if (tabs[nt - 1].n == COPY_TABLE_MAX) ++nt;
    CopyEntry& e = tabs[nt - 1].e[tabs[nt - 1].n++];
    e.user = user; e.user_ld = user_ld; e.rows = rows; e.cols = cols; e.dst_off = dst_off; e.dst_ld = dst_ld;
  }
};

static void build_tables(const Plan& p, const SnerfParams* w, TableBuilder& tb) {
  const int W = p.W, H = p.H, E = p.E;
  for (int i = 0; i < p.L; ++i) {
    const bool skip = (p.skip_mask >> i) & 1u;
    if (i == 0) {
      tb.add(w->fc_w[0], E, W, E, p.w_tr[0], p.k_tr[0]);
    } else if (skip) {  // [gamma | h] columns: gamma -> [0,E), h -> [Ep, Ep+W)
      tb.add(w->fc_w[i], E + W, W, E, p.w_tr[i], p.k_tr[i]);
      tb.add(w->fc_w[i] ? w->fc_w[i] + E : nullptr, E + W, W, W, p.w_tr[i] + p.Ep, p.k_tr[i]);
    } else {
      tb.add(w->fc_w[i], W, W, W, p.w_tr[i], p.k_tr[i]);
    }
    tb.add(w->fc_b[i], W, 1, W, p.b_tr[i], W);
  }
  tb.add(w->feats_w, W, W, W, p.w_fs, W);
  tb.add(w->sigma_w, W, 1, W, p.w_fs + (size_t)W * W, W);
  tb.add(w->feats_b, W, 1, W, p.b_fs, W);
  tb.add(w->sigma_b, 1, 1, 1, p.b_fs + W, 1);
  auto head1 = [&](int blk, float* w0, float* b0, int extra, int xcol) {
    const int in = W + extra;
    const size_t r0 = blk == p.blk_sun ? (size_t)p.sun_col : (size_t)blk * H;
    const size_t row0 = p.w_h1 + r0 * p.FA;
    tb.add(w0, in, H, W, row0, p.FA);
    if (extra > 0) tb.add(w0 ? w0 + W : nullptr, in, H, extra, row0 + p.Wf + xcol, p.FA);
    tb.add(b0, H, 1, H, p.b_h1 + r0, H);
  };
  head1(p.blk_rgb, w->rgb_w0, w->rgb_b0, p.rgb_t ? p.tau : 0, p.x_t);
  if (p.blk_sem >= 0) head1(p.blk_sem, w->sem_w0, w->sem_b0, (p.sem_t || p.sem_ts) ? p.tau : 0, p.sem_ts ? p.x_ts : p.x_t);
  head1(p.blk_beta, w->beta_w0, w->beta_b0, p.tau, p.x_t);
  if (p.blk_sbeta >= 0) head1(p.blk_sbeta, w->sbeta_w0, w->sbeta_b0, p.tau, p.sbeta_ts ? p.x_ts : p.x_t);
  head1(p.blk_sun, w->sun_w[0], w->sun_b[0], 3, p.x_sun);
  tb.add(w->sun_w[1], H, H, H, p.w_s2, H); tb.add(w->sun_b[1], H, 1, H, p.b_s2, H);
  tb.add(w->sun_w[2], H, H, H, p.w_s3, H); tb.add(w->sun_b[2], H, 1, H, p.b_s3, H);
  tb.add(w->sun_w[3], H, 1, H, p.w_s4, H); tb.add(w->sun_b[3], 1, 1, 1, p.b_s4, 1);
  auto fin = [&](int blk, int col, int rows, float* w2, float* b2) {
    tb.add(w2, H, rows, H, p.w_fin + (size_t)col * p.KF + (size_t)blk * H, p.KF);
    tb.add(b2, rows, 1, rows, p.b_fin + col, rows);
  };
  fin(p.blk_rgb, Plan::col_rgb, 3, w->rgb_w2, w->rgb_b2);
  fin(p.blk_beta, Plan::col_beta, 1, w->beta_w2, w->beta_b2);
  if (p.blk_sbeta >= 0) fin(p.blk_sbeta, Plan::col_sbeta, 1, w->sbeta_w2, w->sbeta_b2);
  if (p.blk_sem >= 0) fin(p.blk_sem, Plan::col_sem, p.C, w->sem_w2, w->sem_b2);
  tb.add(w->sky_w0, 3, H, 3, p.sky, 4);
  tb.add(w->sky_b0, H, 1, H, p.sky + 4 * (size_t)H, H);
  tb.add(w->sky_w2, H, 3, H, p.sky + 5 * (size_t)H, H);
  tb.add(w->sky_b2, 3, 1, 3, p.sky + 9 * (size_t)H, 3);
}

// Pack, forward and backward of one step must be planned under the same setting of SNERF_COMPOSE_FEATS: the packed buffer holds either
// the separate or the composed operands, the workspace either layout.  The library remembers, per buffer address, which plan wrote it
// last (host side, at call time -- also under stream capture) and refuses a reader planned the other way.  A buffer it has not seen
// (a copy made by the caller) is taken on trust.
// Limits, by construction: the table is process-wide, holds the 256 addresses noted last and never learns that a buffer was freed.  So the
// check is best effort in both directions -- a mismatch on an address evicted since goes unnoticed, and a buffer the CALLER filled (a
// clone of packed parameters) at an address last noted under the other setting is refused wrongly.  Both need the switch to change inside
// one process, which only tests do; a process that keeps one setting never sees either.
// A workspace's note also says WHICH pass wrote it last: a relight (SNERF_FLAG_RELIGHT) reuses the tensors of an inference main pass and
// is refused on anything else -- a geometry pass (SNERF_FLAG_GEOMETRY) included, which is noted as a kind of its own: it leaves no head
// tensor.  The note is taken when a call is queued, so it guards against mis-sequenced calls; it cannot know that
// the caller overwrote the buffer itself.
namespace {
enum PassKind { PASS_NONE = 0, PASS_MAIN_INFER, PASS_TRAIN, PASS_SC, PASS_BACKWARD, PASS_GEOMETRY };   // PASS_NONE: a packed parameter buffer
struct BufNote { const void* p; bool composed; int kind; SnerfDesc desc; bool no_beta; };
constexpr int NOTE_MAX = 256;
BufNote g_notes[NOTE_MAX];
int g_n_notes = 0, g_note_next = 0;
std::mutex g_note_mu;
void note_plan(const void* buf, bool composed, int kind = PASS_NONE, const SnerfDesc* desc = nullptr, bool no_beta = false) {
  std::lock_guard<std::mutex> lk(g_note_mu);
  BufNote n{buf, composed, kind, desc ? *desc : SnerfDesc{}, no_beta};
  for (int i = 0; i < g_n_notes; ++i) if (g_notes[i].p == buf) { g_notes[i] = n; return; }
  if (g_n_notes < NOTE_MAX) g_notes[g_n_notes++] = n;
  else { g_notes[g_note_next] = n; g_note_next = (g_note_next + 1) % NOTE_MAX; }   // oldest first
}
int check_plan_note(const void* buf, bool composed, const char* who, const char* what) {
  std::lock_guard<std::mutex> lk(g_note_mu);
  for (int i = 0; i < g_n_notes; ++i)
    if (g_notes[i].p == buf && g_notes[i].composed != composed) {
      set_error("%s: the %s was written under SNERF_COMPOSE_FEATS=%d, this call is planned with %d (pack, forward and backward must agree)",
                who, what, g_notes[i].composed ? 1 : 0, composed ? 1 : 0);
      return SNERF_ERR_BAD_DESC;
    }
  return SNERF_OK;
}
// the descriptor fields that make two passes the same pass: everything, bar the RELIGHT bit, the spelling of the default arithmetic and
// the EMBED_GRAD bit (which only selects how much of the backward runs: it may be set at backward time alone).  The GEOMETRY bit IS part
// of the identity: such a pass leaves another workspace.  The DEPTH_MEDIAN bit is not: it changes nothing a pass leaves behind.
bool same_pass_desc(SnerfDesc a, SnerfDesc b) {
  const unsigned ignore = SNERF_FLAG_RELIGHT | SNERF_FLAG_F16X2 | SNERF_FLAG_EMBED_GRAD | SNERF_FLAG_DEPTH_MEDIAN;
  a.flags &= ~ignore; b.flags &= ~ignore;
  return a.n_rays == b.n_rays && a.n_samples == b.n_samples && a.fc_units == b.fc_units && a.fc_layers == b.fc_layers &&
         a.feat_last == b.feat_last && a.skip_mask == b.skip_mask && a.n_freq == b.n_freq && a.siren == b.siren && a.t_dim == b.t_dim &&
         a.n_classes == b.n_classes && a.sem_sigmoid == b.sem_sigmoid && a.use_tj_instead_of_beta == b.use_tj_instead_of_beta &&
         a.use_tj_for_s == b.use_tj_for_s && a.use_separate_beta_for_s == b.use_separate_beta_for_s &&
         a.use_separate_tj_for_semantic == b.use_separate_tj_for_semantic && a.flags == b.flags;
}
// A relight's base pass: the workspace's last noted pass must be an inference main pass of the same descriptor, and one that computed
// the beta block if this relight hands out beta.
int check_relight_note(const void* workspace, const SnerfDesc* d, bool want_beta) {
  std::lock_guard<std::mutex> lk(g_note_mu);
  const BufNote* n = nullptr;
  for (int i = 0; i < g_n_notes; ++i) if (g_notes[i].p == workspace) n = &g_notes[i];
  if (!n || n->kind == PASS_NONE) {
    set_error("snerf_forward(SNERF_FLAG_RELIGHT): no base pass -- the library has not seen an inference main pass write this workspace");
    return SNERF_ERR_BAD_DESC;
  }
  if (n->kind != PASS_MAIN_INFER) {
    set_error("snerf_forward(SNERF_FLAG_RELIGHT): the workspace's last pass was a %s pass, not an inference main pass",
              n->kind == PASS_TRAIN ? "training (SNERF_FLAG_TRAIN)" : n->kind == PASS_SC ? "solar-correction (SNERF_FLAG_SC_PASS)" :
              n->kind == PASS_GEOMETRY ? "geometry (SNERF_FLAG_GEOMETRY)" : "backward");
    return SNERF_ERR_BAD_DESC;
  }
  if (!same_pass_desc(n->desc, *d)) {
    set_error("snerf_forward(SNERF_FLAG_RELIGHT): the descriptor differs from the base pass's (base %d rays x %d samples, flags %u; this call %d x %d, flags %u)",
              n->desc.n_rays, n->desc.n_samples, n->desc.flags, d->n_rays, d->n_samples, d->flags);
    return SNERF_ERR_BAD_DESC;
  }
  if (want_beta && n->no_beta) {
    set_error("snerf_forward(SNERF_FLAG_RELIGHT): beta is asked of a base pass that was asked for no beta and skipped the beta block of the first head layer");
    return SNERF_ERR_BAD_DESC;
  }
  return SNERF_OK;
}
}  // namespace

static int check_inputs(const Plan& p, const SnerfInputs* in) {
  if (!in) { set_error("null inputs"); return SNERF_ERR_NULL; }
  if (!p.geometry) {   // (a geometry pass reads none of the three: they may be NULL)
    if (!in->sun_d || in->sun_stride < 3) { set_error("sun_d (N,3) with stride >= 3 is required"); return SNERF_ERR_NULL; }
    if (!in->t) { set_error("t (N,tau) is required"); return SNERF_ERR_NULL; }
    if (p.x_ts >= 0 && !in->t_s) { set_error("t_s is required with use_separate_tj_for_semantic"); return SNERF_ERR_NULL; }
  }
  if (p.relight) return SNERF_OK;   // positions and depths are the base pass's
  if (in->xyz) {
    if (!in->z_vals) { set_error("explicit xyz needs explicit z_vals"); return SNERF_ERR_NULL; }
  } else {
    if (!in->rays) { set_error("rays or xyz is required"); return SNERF_ERR_NULL; }
    if (!in->z_vals && !in->z_steps) { set_error("z_steps is required when z_vals is not given"); return SNERF_ERR_NULL; }
  }
  return SNERF_OK;
}

}  // namespace snerf

// =====================================================================================================
using namespace snerf;

extern "C" {

int snerf_version(void) { return SNERF_ABI_VERSION; }
const char* snerf_last_error(void) { return g_err; }

size_t snerf_packed_floats(const SnerfDesc* desc) {
  Plan p;
  if (make_plan(desc, &p)) return 0;
  return p.packed_floats;
}

size_t snerf_grad_floats(const SnerfDesc* desc) {
  Plan p;
  if (make_plan(desc, &p)) return 0;
  return p.n_fp32;
}

size_t snerf_workspace_bytes(const SnerfDesc* desc) {
  Plan p;
  if (make_plan(desc, &p)) return 0;
  return p.ws_bytes;
}

int snerf_pack_params(const SnerfDesc* desc, const SnerfParams* params, float* packed, void* stream) {
  Plan p;
  RC(make_plan(desc, &p));
  if (!params || !packed) { set_error("null params/packed"); return SNERF_ERR_NULL; }
  TableBuilder tb;
  build_tables(p, params, tb);
  if (tb.missing) { set_error("snerf_pack_params: a parameter tensor required by this SnerfDesc is NULL"); return SNERF_ERR_NULL; }
  hipStream_t st = (hipStream_t)stream;
  RC(launch_zero_bytes(packed, p.n_fp32 * sizeof(float), st));
  for (int i = 0; i < tb.nt; ++i) RC(launch_copy_table(tb.tabs[i], packed, 0, st));
  // every weight operand (matrix or its transpose) as a fragment-ordered fp16-plane pack with one exponent per matrix -- two
  // launches over a job table (|max| pass, pack pass)
  char* planes = reinterpret_cast<char*>(packed + p.n_fp32);
  int* exps = reinterpret_cast<int*>(planes + p.wp_bytes);
  unsigned* maxbits = reinterpret_cast<unsigned*>(exps + bsp::WPACK_MAX);
  note_plan(packed, p.compose_feats);
  if (!p.compose_feats) return bsp::launch_wpack(p.wj, packed, planes, exps, maxbits, p.pl, st);
  // Compose: W_c = [A W_f | W_h1[:, W:]] with A = W_h1[:, :W], the sigma rows behind it, b_c = b_h1 + A b_f -- once per pack, for the main
  // and the sc pass alike (the sc pass reads the sun block's rows).  One launch of the small fp32 GEMM; then the two operands packed
  // from the scratch, then every other operand (their packs overwrite the scratch).
  {
    bsp::SgTable tb;
    bsp::compose_jobs(tb, packed + p.w_h1, packed + p.w_fs, packed + p.b_fs, packed + p.b_h1, packed + p.o_wc, packed + p.o_bc, p.W, p.FA, p.N1);
    RC(bsp::launch_sgemm(tb, 64, st));
  }
  bsp::WPackTable first, rest;
  first.n = rest.n = 0;
  for (int i = 0; i < p.wj.n; ++i) (i < p.wj_first ? first.j[first.n++] : rest.j[rest.n++]) = p.wj.j[i];
  RC(bsp::launch_wpack(first, packed, planes, exps, maxbits, p.pl, st));
  return bsp::launch_wpack(rest, packed, planes, exps, maxbits, p.pl, st);
}

int snerf_unpack_grads(const SnerfDesc* desc, const float* packed_grads, const SnerfParams* grads, int accumulate,
                       void* stream) {
  Plan p;
  RC(make_plan(desc, &p));
  if (!grads || !packed_grads) { set_error("null grads"); return SNERF_ERR_NULL; }
  TableBuilder tb;
  build_tables(p, grads, tb);
  if (tb.missing) { set_error("snerf_unpack_grads: a gradient tensor required by this SnerfDesc is NULL"); return SNERF_ERR_NULL; }
  hipStream_t st = (hipStream_t)stream;
  for (int i = 0; i < tb.nt; ++i) RC(launch_copy_table(tb.tabs[i], const_cast<float*>(packed_grads), accumulate ? 2 : 1, st));
  return SNERF_OK;
}

int snerf_forward(const SnerfDesc* desc, const float* packed_params, const SnerfInputs* in, const SnerfOutputs* out,
                  void* workspace, size_t workspace_bytes, void* stream) {
  Plan p;
  RC(make_plan(desc, &p));
  if (!packed_params || !out || !workspace) { set_error("snerf_forward: null argument"); return SNERF_ERR_NULL; }
  if (p.geometry) {   // no head runs: a result of one cannot be handed out
    const struct { const void* ptr; const char* name; } heads[] = {
        {out->rgb, "rgb"}, {out->albedo, "albedo"}, {out->sun, "sun"}, {out->sky, "sky"}, {out->beta, "beta"},
        {out->beta_semantic, "beta_semantic"}, {out->semantic_logits, "semantic_logits"}, {out->semantic_label, "semantic_label"}};
    for (const auto& h : heads)
      if (h.ptr) {
        set_error("snerf_forward(SNERF_FLAG_GEOMETRY): out->%s is not a result of a geometry pass (depth, weights, transparency, sigmas, z_vals)", h.name);
        return SNERF_ERR_BAD_DESC;
      }
  }
  if (p.depth_median) {   // the launch behind the composite reads the weights and depths that pass hands out
    if (!out->weights) { set_error("snerf_forward(SNERF_FLAG_DEPTH_MEDIAN): out->weights is NULL (the median is computed from the weights the pass writes)"); return SNERF_ERR_NULL; }
    if (!out->z_vals) { set_error("snerf_forward(SNERF_FLAG_DEPTH_MEDIAN): out->z_vals is NULL (the median is computed from the depths the pass writes)"); return SNERF_ERR_NULL; }
    if (!out->depth) { set_error("snerf_forward(SNERF_FLAG_DEPTH_MEDIAN): out->depth is NULL -- nothing to compute"); return SNERF_ERR_NULL; }
  }
  if (workspace_bytes < p.ws_bytes) { set_error("snerf_forward: workspace too small (%zu < %zu)", workspace_bytes, p.ws_bytes); return SNERF_ERR_WORKSPACE; }
  if (((uintptr_t)workspace & 255) || ((uintptr_t)packed_params & 255)) { set_error("workspace and packed params must be 256-byte aligned"); return SNERF_ERR_WORKSPACE; }
  RC(check_inputs(p, in));
  RC(check_plan_note(packed_params, p.compose_feats, "snerf_forward", "packed parameter buffer"));
  if (p.relight) {   // every refusal before any launch; the note stays the base pass's, so relights chain
    RC(check_plan_note(workspace, p.compose_feats, "snerf_forward", "workspace"));
    RC(check_relight_note(workspace, desc, out->beta != nullptr));
  } else {
    note_plan(workspace, p.compose_feats, p.train ? PASS_TRAIN : p.sc ? PASS_SC : p.geometry ? PASS_GEOMETRY : PASS_MAIN_INFER, desc, skips_beta_block(p, out->beta != nullptr));
  }
  RC(forward_bsp(p, packed_params, in, out, workspace, (hipStream_t)stream));
  if (p.depth_median) RC(launch_ray_median(out->weights, out->z_vals, out->sigmas, out->depth, p.N, p.S, (hipStream_t)stream));
  return SNERF_OK;
}

int snerf_backward(const SnerfDesc* desc, const float* packed_params, const SnerfInputs* in, const SnerfOutGrads* gout,
                   float* packed_grads, float* d_t, float* d_t_s, void* workspace, size_t workspace_bytes, void* stream) {
  Plan p;
  RC(make_plan(desc, &p));
  if (p.depth_median) { set_error("snerf_backward: SNERF_FLAG_DEPTH_MEDIAN is a bit of inference passes (the median depth has no gradient)"); return SNERF_ERR_BAD_DESC; }
  if (!p.train) { set_error("snerf_backward needs the SnerfDesc used for the SNERF_FLAG_TRAIN forward"); return SNERF_ERR_BAD_DESC; }
  // (SNERF_FLAG_EMBED_GRAD: packed_grads is neither read nor written and may be NULL)
  if (!packed_params || !gout || (!packed_grads && !p.embed_grad) || !workspace) { set_error("snerf_backward: null argument"); return SNERF_ERR_NULL; }
  if (p.embed_grad && !d_t && !d_t_s) { set_error("snerf_backward(SNERF_FLAG_EMBED_GRAD): d_t and d_t_s are both NULL -- nothing to compute"); return SNERF_ERR_NULL; }
  if (workspace_bytes < p.ws_bytes) { set_error("snerf_backward: workspace too small (%zu < %zu)", workspace_bytes, p.ws_bytes); return SNERF_ERR_WORKSPACE; }
  if (((uintptr_t)workspace & 255) || ((uintptr_t)packed_params & 255) || ((uintptr_t)packed_grads & 255)) { set_error("workspace and packed buffers must be 256-byte aligned"); return SNERF_ERR_WORKSPACE; }
  RC(check_inputs(p, in));
  RC(check_plan_note(packed_params, p.compose_feats, "snerf_backward", "packed parameter buffer"));
  RC(check_plan_note(workspace, p.compose_feats, "snerf_backward", "workspace"));
  note_plan(workspace, p.compose_feats, PASS_BACKWARD, desc);
  return backward_bsp(p, packed_params, in, gout, packed_grads, d_t, d_t_s, workspace, (hipStream_t)stream);
}

int snerf_sample_z(const float* rays, const float* z_steps, const float* u, float* z, int n_rays, int n_samples, void* stream) {
  if (!rays || !z_steps || !z || n_rays <= 0 || n_samples <= 0) { set_error("snerf_sample_z: bad argument"); return SNERF_ERR_NULL; }
  return launch_sample_z(rays, z_steps, u, z, n_rays, n_samples, (hipStream_t)stream);
}

int snerf_embedding_rows(const float* table, int n_embed, int tau, const long long* idx, int n, float* rows, void* stream) {
  if (!table || !idx || !rows || n_embed <= 0 || tau <= 0 || n <= 0) { set_error("snerf_embedding_rows: bad argument"); return SNERF_ERR_NULL; }
  return launch_embedding_rows(table, n_embed, tau, idx, n, rows, (hipStream_t)stream);
}

int snerf_embedding_backward(const long long* idx, const float* d_rows, int n, int tau, int n_embed, float* grad_table, void* stream) {
  if (!idx || !d_rows || !grad_table || n_embed <= 0 || tau <= 0 || n <= 0) { set_error("snerf_embedding_backward: bad argument"); return SNERF_ERR_NULL; }
  return launch_embedding_backward(idx, d_rows, n, tau, n_embed, grad_table, (hipStream_t)stream);
}

int snerf_profile_begin(void) { return profile_begin(); }
int snerf_profile_end(SnerfProfile* out) { return profile_end(out); }

}  // extern "C"
