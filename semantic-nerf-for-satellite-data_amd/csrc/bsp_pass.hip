// Forward / backward launch sequences of one rendering pass: every activation tensor lives as block-scaled fp16 planes
// (bsp.h; two planes in the default arithmetic, one under SNERF_FLAG_F16X1 -- Plan::pl, the kernels are templated on it),
// every dense layer is one launch of bsp_kc.hip / bsp_gemm.hip, weights come pre-packed in fragment order.
// Reference: semantic/models/rs_semantic.py:260-340 (forward), its autograd backward.
#include "aux_kernels.h"
#include "bsp.h"
#include "composite.h"
#include "normals.h"
#include "plan.h"

namespace snerf {

namespace {
// The workspace: resolves offsets to pointers and binds a plane tensor (plan.h: PlaneT -- planes, exponent table and leading
// dimension in one piece) to its role in a launch.
struct Ws {
  char* base;
  char* c(size_t off) const { return base + off; }
  float* f(size_t off) const { return reinterpret_cast<float*>(base + off); }
  int* i(size_t off) const { return reinterpret_cast<int*>(base + off); }
  unsigned* u(size_t off) const { return reinterpret_cast<unsigned*>(base + off); }
  // K-contiguous launch: input columns [col0, col0 + k) of t; a second input segment (k from Ka on: all of t); output at column col0
  // (+ the sign words of cos where t keeps them); the stored activation whose derivative a dX epilogue multiplies by
  void a(bsp::KcArgs& g, const PlaneT& t, int k, int col0 = 0) const { g.A = c(t.o); g.EA = i(t.e); g.lda = t.ld; g.a_col0 = col0; g.Ka = k; }
  void a2(bsp::KcArgs& g, const PlaneT& t) const { g.A2 = c(t.o); g.EA2 = i(t.e); g.lda2 = t.ld; }
  void out(bsp::KcArgs& g, const PlaneT& t, int col0 = 0) const { g.C = c(t.o); g.EC = i(t.e); g.ldc = t.ld; g.c_col0 = col0; g.Csign = t.s ? u(t.s) : nullptr; }
  void h(bsp::KcArgs& g, const PlaneT& t, int col0 = 0) const { g.H = c(t.o); g.EH = i(t.e); g.ldh = t.ld; g.h_col0 = col0; g.Hsign = t.s ? u(t.s) : nullptr; }
  // dW launch: dZ (all of it from column 0) and X from column col0
  void dz(bsp::DwArgs& g, const PlaneT& t) const { g.A = c(t.o); g.EA = i(t.e); g.lda = t.ld; g.a_col0 = 0; }
  void x(bsp::DwArgs& g, const PlaneT& t, int col0) const { g.B = c(t.o); g.EB = i(t.e); g.ldb = t.ld; g.b_col0 = col0; }
};
// weight operand `job` of the plan's table (Plan::wj), resolved in the packed buffer
struct WOp { const char* W; const int* EW; int rb32; unsigned bytes; int K; };
WOp wop(const Plan& p, const float* pk, int job) {
  const char* planes = reinterpret_cast<const char*>(pk + p.n_fp32);
  const bsp::WPackJob& w = p.wj.j[job];
  return {planes + w.dst_off, reinterpret_cast<const int*>(planes + p.wp_bytes) + w.e_idx, (w.rows + 31) / 32,
          (unsigned)bsp::wp16_bytes(w.rows, w.K, p.pl), w.K};
}
// ... as the B of a K-contiguous launch (rows [row0, ..), k >= k0 of it)
void weights(bsp::KcArgs& g, const Plan& p, const float* pk, int job, int row0 = 0, int k0 = 0) {
  const WOp w = wop(p, pk, job);
  g.W = w.W; g.EW = w.EW; g.w_rb32 = w.rb32; g.w_bytes = w.bytes;
  g.w_row0 = row0; g.w_k0 = k0;
  g.pl = p.pl;
}
// sigma / sun-visibility pre-activations of SIREN passes: partial dot products of the producing launches (Plan::nd_sig / nd_sun)
void narrow_parts(CompArgs& c, const Plan& p, const float* pk, const Ws& ws) {
  c.part_stride = p.Pp;
  if (p.nd_sig) { c.sig_part = ws.f(p.o_sigpart); c.n_sig_part = 4 * (p.W / 256); c.sig_bias = pk + p.b_fs + p.W; }
  if (p.nd_sun) { c.sun_part = ws.f(p.o_sunpart); c.n_sun_part = 4 * (p.H / 256); c.sun_bias = pk + p.b_s4; }
  if (p.nd_fin) {
    c.fin_part = ws.f(p.o_finpart); c.fin_bias = pk + p.b_fin;
    c.fin_blk[0] = p.blk_rgb; c.fin_blk[1] = p.blk_sem < 0 ? 0 : p.blk_sem; c.fin_blk[2] = p.blk_beta; c.fin_blk[3] = p.blk_sbeta < 0 ? 0 : p.blk_sbeta;
  }
}
}  // namespace

int forward_bsp(const Plan& p, const float* pk, const SnerfInputs* in, const SnerfOutputs* out, void* workspace, hipStream_t st) {
  const Ws ws{(char*)workspace};
  // tile counters of the K-contiguous launches: one zeroed 64-byte slot per launch, in launch order.  (Zeroed by a kernel:
  // with hipMemsetAsync the forward's and the backward's memset of this region became two identical memset nodes of a
  // captured HIP graph, and replays on ROCm 7.2 then ran the backward's launches on counters that had not been zeroed.)  The first
  // kernel of the pass does it on the side: the encode kernel here, the composite backward in backward_bsp.
  // Every other K-contiguous launch of a pass walks its tiles backwards (tiles.h): a consumer starts with the rows its producer
  // wrote last.  Measured 372.0 -> 369.8 us per launch, 28.27 -> 28.12 ms per step (two A/B pairs on one box).
  int kcq = 0;
  auto launch_kc = [&](bsp::KcArgs& g) { g.rev = kcq & 1; g.tile_ctr = kcq < KCQ_SLOTS ? ws.i(p.o_kcq) + 16 * kcq++ : nullptr; return bsp::launch_kc(g, st); };
  const int P = p.P, W = p.W, H = p.H;
  float* z = ws.f(p.o_z);
  const int act = p.siren ? ACT_SIN : ACT_RELU;
  const bool fused = p.fuse_trunk && bsp::trunk_fusion_enabled();
  const bool feats_launch = !p.geometry && !p.compose_feats && (!fused || p.train);   // feats_from_xyz as a launch of its own
  const size_t EB = 2 * (size_t)p.pl;   // bytes per element of a plane tensor
  // The extras block [sun | t | t_s] of the [feats or h_last | extras] tensor, as both its writers take it
  EncodeArgs ea;
  ea.sun_d = in->sun_d; ea.sun_stride = in->sun_stride; ea.t = in->t; ea.t_s = in->t_s;
  ea.N = p.N; ea.S = p.S; ea.F = p.F; ea.Ep = p.Ep;
  ea.FA = p.FA; ea.W = p.Wf; ea.Xp = p.Xp; ea.x_sun = p.x_sun; ea.x_t = p.x_t; ea.x_ts = p.x_ts; ea.tau = p.tau;
  ea.zero = ws.u(p.o_kcq); ea.zero_n = KCQ_SLOTS * 16;
  if (p.relight) {
    // Relight (SNERF_FLAG_RELIGHT; api.hip has checked that the workspace holds an inference main pass of this plan): z, the
    // [feats or h_last] columns of fa, sigma's partials / buffer, the rgb / semantic / beta blocks of h1 and the final layers'
    // partials / buffer are the base pass's.  None of the launches below writes them: fa is a tensor of its own (not one of the
    // two alternating trunk buffers), the head launch writes the sun block's columns of h1 only and folds no finals.  What a new
    // sun changes is the extras block (whole: its |max|, hence the exponent of the t columns, may move), then everything from the
    // first head layer's sun block on.  Each launch keeps the tile direction (rev) and the counter slot it has in the full pass.
    if (out->z_vals) SNERF_HIP_CHECK(hipMemcpyAsync(out->z_vals, z, sizeof(float) * P, hipMemcpyDeviceToDevice, st));
    RC(bsp::launch_relight_extras(ea, ws.c(p.fa.o), ws.i(p.fa.e), p.Wf, p.pl, st));
    kcq = (fused ? 1 : p.L) + (feats_launch ? 1 : 0);
  } else {
    // 1. depths
    if (in->z_vals) SNERF_HIP_CHECK(hipMemcpyAsync(z, in->z_vals, sizeof(float) * P, hipMemcpyDeviceToDevice, st));
    else RC(launch_sample_z(in->rays, in->z_steps, in->u, z, p.N, p.S, st));
    if (out->z_vals) SNERF_HIP_CHECK(hipMemcpyAsync(out->z_vals, z, sizeof(float) * P, hipMemcpyDeviceToDevice, st));
    // 2. positions + encoding + extras, written as planes with their block exponents
    ea.rays = in->xyz ? nullptr : in->rays; ea.xyz = in->xyz; ea.z = z;
    ea.dir_is_sun = (p.sc && !in->xyz) ? 1 : 0;
    // (a geometry pass has no [. | extras] tensor: the kernel then writes the planes of pe alone -- the same bits -- and reads none of
    //  sun_d / t / t_s, which may be null; it still clears the tile counters)
    RC(bsp::launch_encode_bsp(ea, ws.c(p.pe.o), ws.i(p.pe.e), p.geometry ? nullptr : ws.c(p.fa.o), p.geometry ? nullptr : ws.i(p.fa.e), p.Wf, p.pl, st));
    if (p.Wf > W && !p.geometry)   // pad columns between feats and extras (narrow test networks only): zero planes, read against zero weights
      RC(bsp::launch_zero_cols(ws.c(p.fa.o) + (size_t)W * EB, (size_t)p.FA * EB, (size_t)(p.Wf - W) * EB, P, st));
    // 3. trunk (rs_semantic.py:325-334)
    if (fused) {   // one persistent launch, the activation tile resident in LDS (bsp_trunk.hip); inference: only the last layer's planes + sigma's partials leave
      bsp::TrunkArgs g;
      g.pe = ws.c(p.pe.o); g.Epe = ws.i(p.pe.e); g.P = P; g.W = W; g.L = p.L; g.skip_mask = p.skip_mask;
      // feats (rs_semantic.py:338) rides as one more layer of an inference pass, entry L: written into the first W columns of the
      // [feats | sun | t | t_s] tensor.  (One plane: fuse_trunk holds only with p.pl == 1.)
      // A geometry pass drops that entry: the trunk alone, whose last layer's planes leave into h[L - 1] (api.hip plans fuse_trunk for
      // that form: no fusion at L = 3, where the final layer would request the next tile's encoding).
      const bool fused_feats = !p.train && !p.geometry;
      if (!p.train && !fused_feats) { g.H[p.L - 1] = ws.c(p.h[p.L - 1].o); g.EH[p.L - 1] = ws.i(p.h[p.L - 1].e); }
      for (int i = 0; i < p.L + (fused_feats ? 1 : 0); ++i) {
        const WOp w = wop(p, pk, i < p.L ? p.wj_tr[i] : p.wj_fs);
        g.Wp[i] = w.W; g.EW[i] = w.EW; g.w_bytes[i] = w.bytes; g.K[i] = w.K;
        g.bias[i] = pk + (i < p.L ? p.b_tr[i] : p.b_fs);
        g.w0[i] = i == 0 ? 30.f : 1.f;
      }
      if (fused_feats) { g.F = ws.c(p.fa.o); g.EF = ws.i(p.fa.e); g.ldf = p.fa.ld; }
      for (int i = 0; i < p.L && p.train; ++i) {   // training (feats stays a launch of its own): every layer's planes and sign words leave for the backward pass
        g.H[i] = ws.c(p.h[i].o); g.EH[i] = ws.i(p.h[i].e); g.Hsign[i] = ws.u(p.h[i].s);
      }
      g.nd_w = pk + p.w_fs + (size_t)W * W; g.nd_out = ws.f(p.o_sigpart); g.nd_stride = p.Pp;
      g.tile_ctr = ws.i(p.o_kcq) + 16 * kcq++;
      RC(bsp::launch_trunk(g, p.train, st));
    }
    for (int i = 0; i < p.L && !fused; ++i) {
      bsp::KcArgs g;
      const bool skip = (p.skip_mask >> i) & 1u;
      if (i == 0) ws.a(g, p.pe, p.Ep);
      else if (skip) { ws.a(g, p.pe, p.Ep); ws.a2(g, p.h[i - 1]); }   // [gamma | h]
      else ws.a(g, p.h[i - 1], W);
      weights(g, p, pk, p.wj_tr[i]);
      g.I = P; g.J = W; g.K = p.k_tr[i];
      ws.out(g, p.h[i]);   // (inference: h[i] alternates between two buffers, api.hip: plan_bsp)
      g.bias = pk + p.b_tr[i]; g.act = act; g.w0 = (p.siren && i == 0) ? 30.f : 1.f;
      if (i == p.L - 1 && p.nd_sig) {   // sigma's 1-wide projection rides in this launch's epilogue (bsp_kc.hip: NDOT)
        g.nd_w = pk + p.w_fs + (size_t)W * W; g.nd_out = ws.f(p.o_sigpart); g.nd_stride = p.Pp;
      }
      RC(launch_kc(g));
    }
    const PlaneT& hl = p.h[p.L - 1];
    if (!p.nd_sig) {  // sigma pre-activation (rs_semantic.py:337) -> 32-wide fp32 buffer, column 0
      bsp::KcArgs g;
      ws.a(g, hl, W); weights(g, p, pk, p.wj_sig);
      g.I = P; g.J = NARROW; g.K = W; g.Cf = ws.f(p.o_sigo); g.bias = pk + p.b_fs + W;
      RC(bsp::launch_kc_narrow(g, st));
    }
    // Composed plans (Plan::compose_feats) run no feats layer: h[L - 1] IS columns [0, W) of the [. | sun | t | t_s] tensor, and the first
    // head layer below multiplies it by W_c = W_h1[:, :W] W_f with the bias b_c that the pack built.
    if (feats_launch) {  // feats (rs_semantic.py:338), written into the first W columns of the [feats | sun | t | t_s] tensor
      bsp::KcArgs g;
      ws.a(g, hl, W); weights(g, p, pk, p.wj_fs);
      g.I = P; g.J = W; g.K = W; ws.out(g, p.fa); g.bias = pk + p.b_fs;
      RC(launch_kc(g));
    }
  }
  if (p.geometry) {
    // Geometry pass (SNERF_FLAG_GEOMETRY): sigma's pre-activation is complete, and nothing below serves anything but a head.  The
    // launches above ARE the leading launches of the full pass, queued in its order, so each already has the counter slot and the
    // tile direction (rev) it has there -- no `kcq = ...` as in the relight branch, whose launches are the full pass's trailing ones.
    // Kept because the direction decides which rows a consumer finds in the cache when it starts (the measurement in the comment on
    // launch_kc), not for the bits: a tile's values do not depend on the order the tiles are walked in.
    // The composite reads z and sigma's partials / buffer alone; every head pointer of CompArgs stays null.
    CompArgs c;
    c.N = p.N; c.S = p.S; c.H = H; c.C = 0;
    c.z = z; c.sigo = ws.f(p.o_sigo);
    c.part_stride = p.Pp;
    if (p.nd_sig) { c.sig_part = ws.f(p.o_sigpart); c.n_sig_part = 4 * (W / 256); c.sig_bias = pk + p.b_fs + W; }
    c.o_depth = out->depth; c.o_weights = out->weights; c.o_transparency = out->transparency; c.o_sigmas = out->sigmas;
    return launch_composite_fwd(c, st, /*geometry=*/true);
  }
  const int r0 = (p.sc || p.relight) ? p.sun_col : 0;
  {  // first layer of every head in one GEMM (sc pass, relight: sun-visibility block only; a relight writes it at its column of the main pass's h1)
    bsp::KcArgs g;
    ws.a(g, p.fa, p.FA); weights(g, p, pk, p.wj_h1, r0);
    g.I = P; g.J = p.relight ? H : p.h1w; g.K = p.FA; ws.out(g, p.h1, p.relight ? p.sun_col : 0);
    g.bias = pk + (p.compose_feats ? p.o_bc : p.b_h1) + r0; g.act = act; g.w0 = 1.f;
    if (p.nd_fin && !p.relight) {   // (a relight folds no finals: the base pass's partials are what its composite reads)   // the heads' final layers (block-diagonal [32][KF]: block b's rows read only block b's 256 columns) in this launch's epilogue
      g.nd_w = pk + p.w_fin; g.nd_ldw = p.KF; g.nd_omax = ND_FIN; g.nd_out = ws.f(p.o_finpart); g.nd_stride = p.Pp;
      auto blk = [&](int b, int col, int n) { if (b >= 0) { g.nd_rows[b] = n; g.nd_row0[b] = col; } };
      blk(p.blk_rgb, Plan::col_rgb, 3); blk(p.blk_sem, Plan::col_sem, p.C); blk(p.blk_beta, Plan::col_beta, 1); blk(p.blk_sbeta, Plan::col_sbeta, 1);
      if (skips_beta_block(p, out->beta != nullptr)) g.tj_skip = p.blk_beta;   // (plan.h)
    }
    RC(launch_kc(g));
  }
  const int sun_col = p.sc ? 0 : p.sun_col;
  {  // sun visibility layers 2, 3 (rs_semantic.py:217-227)
    bsp::KcArgs g;
    ws.a(g, p.h1, H, sun_col); weights(g, p, pk, p.wj_s2);
    g.I = P; g.J = H; g.K = H; ws.out(g, p.s2); g.bias = pk + p.b_s2; g.act = act;
    RC(launch_kc(g));
    ws.a(g, p.s2, H); weights(g, p, pk, p.wj_s3);
    ws.out(g, p.s3); g.bias = pk + p.b_s3;
    if (p.nd_sun) { g.nd_w = pk + p.w_s4; g.nd_out = ws.f(p.o_sunpart); g.nd_stride = p.Pp; }   // the sun-visibility output likewise
    RC(launch_kc(g));
  }
  if (!p.nd_sun) {  // sun visibility output pre-activation
    bsp::KcArgs g;
    ws.a(g, p.s3, H); weights(g, p, pk, p.wj_s4);
    g.I = P; g.J = NARROW; g.K = H; g.Cf = ws.f(p.o_suno); g.bias = pk + p.b_s4;
    RC(bsp::launch_kc_narrow(g, st));
  }
  if (!p.sc && !p.nd_fin && !p.relight) {  // last layer of rgb / beta / beta_s / semantic heads: block-diagonal [32][KF]
    bsp::KcArgs g;
    ws.a(g, p.h1, p.KF); weights(g, p, pk, p.wj_fin);
    g.I = P; g.J = NARROW; g.K = p.KF; g.Cf = ws.f(p.o_fino); g.bias = pk + p.b_fin;
    RC(bsp::launch_kc_narrow(g, st));
  }
  // 4. composite (reads the three 32-wide fp32 buffers)
  CompArgs c;
  c.N = p.N; c.S = p.S; c.H = H; c.C = p.C; c.sc = p.sc; c.sem_sigmoid = p.sem_sigmoid; c.has_sbeta = p.blk_sbeta >= 0;
  c.z = z; c.sigo = ws.f(p.o_sigo); c.fino = ws.f(p.o_fino); c.suno = ws.f(p.o_suno);
  narrow_parts(c, p, pk, ws);
  c.sun_d = in->sun_d; c.sun_stride = in->sun_stride; c.sky = pk + p.sky;
  c.o_rgb = out->rgb; c.o_depth = out->depth; c.o_weights = out->weights; c.o_transparency = out->transparency;
  c.o_albedo = out->albedo; c.o_sun = out->sun; c.o_sky = out->sky; c.o_beta = out->beta; c.o_sigmas = out->sigmas;
  c.o_beta_s = out->beta_semantic; c.o_logits = out->semantic_logits; c.o_label = (long long*)out->semantic_label;
  if (p.train) { c.save_T = ws.f(p.o_T); c.save_rgbraw = ws.f(p.o_rgbraw); }
  RC(launch_composite_fwd(c, st));
  return SNERF_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
namespace {
// Deferred reductions: every dW launch writes its split slabs, every dX launch its column-sum partials, into a region of
// its OWN inside the reduction arena (p.o_rq); the reductions into the packed gradient buffer are queued and run as two
// launches at the end of the pass (aux_kernels.hip: launch_reductions) instead of ~60 small ones in between the GEMMs.
struct RQ {
  float* base; size_t cap, used = 0; bool over = false;   // base == null: a counting arena (bsp_rq_floats)
  RedTable elem, col;
  float* take(size_t floats) {
    const size_t n = round_up_sz(floats, 64);
    if (used + n > cap) { over = true; return base; }
    float* r = base ? base + used : nullptr; used += n; return r;
  }
};
struct DwMat { DwSplit sp; size_t stride; int ldw; float* slab; };
inline int cs_ld(int width) { return (width + 3) & ~3; }

// Every region a backward pass takes from the arena, by the launch that fills it: the split-K slabs of each weight matrix (w_*),
// the column-sum partials of each dX launch (cs_*: one row per 128-row tile) and the 256-row partial sums of the three 32-wide
// gradients (nar_*).  take_regions is the ONE walk over them: Plan::rq_floats is what it takes from a counting arena, and
// backward_bsp runs it on the real one before its first launch.
struct BwdRegions {
  float *nar_fin = nullptr, *nar_sun = nullptr, *nar_sig = nullptr;
  DwMat w_fin, w_s4, w_s3, w_s2, w_h1, w_fs;
  float *cs_fin = nullptr, *cs_s3 = nullptr, *cs_s2 = nullptr, *cs_sun = nullptr, *cs_fa = nullptr, *cs_hl = nullptr;
  int ld_cs1 = 0;   // composed: cs_fin and cs_sun are column ranges of ONE [tiles][h1w] region (row 0 of it becomes g_c, the bias gradient of the composed layer)
  struct Layer { DwMat w, w_gamma; float* cs; } tr[SNERF_MAX_LAYERS];   // w_gamma: skip layers; cs: the dX launch into layer i - 1
};
// `embed_only` (SNERF_FLAG_EMBED_GRAD): the two regions of the launches that lie between the cotangents and d t -- the 256-row partials
// of d fin and the column-sum partials of the dX launch into dz1[:, :KF] -- and nothing else.
void take_regions(const Plan& p, RQ& rq, BwdRegions& r, bool embed_only = false) {
  // `split_rows`: the rows the split count is chosen for when they differ from the slab's (the [W + 32][W] matrix of feats + sigma:
  // its wide launch covers W rows -- counting the 32 sigma rows as a third row tile gave it 43 splits, 172 workgroups for 256 CUs)
  auto dw = [&](int rows, int ldw, int cols, bool narrow_rows, int split_rows = 0) {
    DwMat m;
    m.sp = dw_choose_bsp(p.P, split_rows > 0 ? split_rows : rows, cols, narrow_rows);
    m.stride = round_up_sz((size_t)rows * ldw, 64);
    m.ldw = ldw;
    m.slab = rq.take(m.stride * m.sp.ns);
    return m;
  };
  auto cs = [&](int width) { return rq.take((size_t)((p.P + 127) / 128) * cs_ld(width)); };
  auto nar = [&]() { return rq.take((size_t)((p.P + 255) / 256) * NARROW); };
  const int W = p.W, H = p.H;
  if (embed_only) {
    if (p.sc) return;
    r.nar_fin = nar();
    if (p.compose_feats) { r.ld_cs1 = cs_ld(p.h1w); r.cs_fin = cs(p.h1w); }
    else r.cs_fin = cs(p.KF);
    return;
  }
  if (!p.sc) { r.nar_fin = nar(); r.w_fin = dw(NARROW, p.KF, p.KF, true); if (!p.compose_feats) r.cs_fin = cs(p.KF); }
  r.nar_sun = nar(); r.w_s4 = dw(NARROW, H, H, true); r.w_s3 = dw(H, H, H, false); r.w_s2 = dw(H, H, H, false);   // one slab region per matrix
  r.cs_s3 = cs(H); r.cs_s2 = cs(H);
  if (p.compose_feats) {
    // no d feats tensor, so no cs_fa; of the [W + 32][W] matrix only the 32 sigma rows are a dW launch (same splits as before)
    r.ld_cs1 = cs_ld(p.h1w); r.cs_fin = cs(p.h1w); r.cs_sun = r.cs_fin ? r.cs_fin + (p.sc ? 0 : p.sun_col) : nullptr;   // (null: the counting arena)
    r.w_h1 = dw(p.h1w, p.FA, p.FA, false);
    r.nar_sig = nar(); r.w_fs = dw(NARROW, W, W, false, W); r.cs_hl = cs(W);
  } else {
    r.cs_sun = cs(H);
    r.w_h1 = dw(p.h1w, p.FA, p.FA, false); r.cs_fa = cs(p.FA);
    r.nar_sig = nar(); r.w_fs = dw(W + NARROW, W, W, false, W); r.cs_hl = cs(W);
  }
  for (int i = p.L - 1; i >= 0; --i) {
    // skip layer W_i = [W_gamma (Ep columns) | W_h (W columns)]: the two column blocks are two contractions of very different
    // width over the same dz, so each gets a slab region and a split count of its own (the 64-column block: two tiles x 128 splits;
    // sharing the wide block's 64 splits left half the chip idle for it: 275 us against 180) and a 2-D reduction into its columns
    if (i > 0 && ((p.skip_mask >> i) & 1u)) { r.tr[i].w_gamma = dw(W, p.Ep, p.Ep, false); r.tr[i].w = dw(W, W, W, false); }
    else r.tr[i].w = dw(W, p.k_tr[i], i == 0 ? p.Ep : W, false);
    r.tr[i].cs = i > 0 ? cs(W) : nullptr;
  }
}
}  // namespace

size_t bsp_rq_floats(const Plan& p) {
  RQ rq{nullptr, ~(size_t)0};
  BwdRegions r;
  take_regions(p, rq, r);
  return rq.used;
}

int backward_bsp(const Plan& p, const float* pk, const SnerfInputs* in, const SnerfOutGrads* go, float* gp, float* d_t, float* d_t_s,
                 void* workspace, hipStream_t st) {
  const Ws ws{(char*)workspace};
  const int P = p.P, W = p.W, H = p.H;
  // SNERF_FLAG_EMBED_GRAD: d_t / d_t_s alone.  t enters at the extras columns of the first head layer and the density does not depend
  // on it, so the pass ends where transient_grads() has run: composite backward, planes of d fin, the dX launch into dz1[:, :KF], the
  // narrow launch into d extras, the per-ray sums -- the launches of the full pass with the operands of the full pass, hence its bits.
  // gp may be NULL and is never touched: no reduction is queued, none is run.
  const bool embed = p.embed_grad;
  int kcq = 0;     // (the counters are cleared by the composite backward kernel, the first launch of this pass)
  auto launch_kc = [&](bsp::KcArgs& g) { g.rev = kcq & 1; g.tile_ctr = kcq < KCQ_SLOTS ? ws.i(p.o_kcq) + 16 * kcq++ : nullptr; return bsp::launch_kc(g, st); };
  RQ rq{ws.f(p.o_rq), p.rq_floats};
  BwdRegions r;
  take_regions(p, rq, r, embed);
  if (rq.over) { set_error("reduction arena too small (plan / pass mismatch)"); return SNERF_ERR_WORKSPACE; }
  // activation derivative in a dX epilogue, rebuilt from the stored activation h (column col0 of it): siren
  // w0 * sign(cos) * sqrt(1 - h^2) with h's sign words; relu: h > 0
  auto dact = [&](bsp::KcArgs& g, const PlaneT& h, int col0 = 0, float w0 = 1.f) {
    ws.h(g, h, col0);
    if (p.siren) { g.aux_mode = AUX_SINREC; g.w0 = w0; }
    else g.aux_mode = AUX_RELU_MASK;
  };
  // a dX launch leaves the column sums of what it stores, one row per 128-row tile: the bias gradient of the layer below
  auto colsum = [&](bsp::KcArgs& g, float* cs, int width) { g.colsum = cs; g.ldcs = cs_ld(width); };
  auto bias_from_colsum = [&](const float* cs, int width, float* gout) { return red_add_col(rq.col, cs, (P + 127) / 128, (size_t)cs_ld(width), width, gout); };
  // slab[split][i][slab_off + j] = sum_p dZ[p][i] X[p][x_col0 + j]
  auto dw_gemm = [&](const DwMat& m, const PlaneT& dz, int I, bool narrow_i, const PlaneT& X, int x_col0, int J, size_t slab_off = 0) {
    bsp::DwArgs g;
    ws.dz(g, dz); ws.x(g, X, x_col0);
    g.I = I; g.J = J; g.P = P;
    g.C = m.slab + slab_off; g.ldc = m.ldw;
    g.k_split = m.sp.k_split; g.n_split = m.sp.ns; g.slab_stride = m.stride; g.pl = p.pl;
    return bsp::launch_dw(g, narrow_i, st);
  };
  auto dw_reduce = [&](const DwMat& m, size_t count, float* gout) { return red_add_elem(rq.elem, m.slab, m.sp.ns, m.stride, count, gout); };
  // bias gradient of a 32-wide pre-activation gradient; the same pass writes its planes + exponents (the dX / dW operands)
  auto narrow_grad = [&](const float* dnar, float* part, const PlaneT& t, float* gout) {
    RC(bsp::launch_colsum32_bsp(dnar, P, part, ws.c(t.o), ws.i(t.e), p.pl, st));
    return red_add_col(rq.col, part, (P + 255) / 256, NARROW, NARROW, gout);
  };
  float* dsig = ws.f(p.o_dsig); float* dfin = ws.f(p.o_dfin); float* dsun = ws.f(p.o_dsun);
  if (embed && p.sc) {   // the sun-visibility block reads [feats | sun_d] only: zeros, as transient_grads() below writes them, and no launch besides
    if (d_t) RC(launch_zero_bytes(d_t, (size_t)p.N * p.tau * sizeof(float), st));
    if (d_t_s && p.x_ts >= 0) RC(launch_zero_bytes(d_t_s, (size_t)p.N * p.tau * sizeof(float), st));
    return SNERF_OK;
  }
  // 0. composite backward -> gradients of the 32-wide pre-activations (+ sky MLP grads)
  CompBwdArgs b;
  CompArgs& c = b.f;
  c.N = p.N; c.S = p.S; c.H = H; c.C = p.C; c.sc = p.sc; c.sem_sigmoid = p.sem_sigmoid; c.has_sbeta = p.blk_sbeta >= 0;
  c.z = ws.f(p.o_z); c.sigo = ws.f(p.o_sigo); c.fino = ws.f(p.o_fino); c.suno = ws.f(p.o_suno);
  narrow_parts(c, p, pk, ws);
  c.sun_d = in->sun_d; c.sun_stride = in->sun_stride; c.sky = pk + p.sky;
  b.T = ws.f(p.o_T); b.rgbraw = ws.f(p.o_rgbraw);
  b.g_rgb = go->rgb; b.g_depth = go->depth; b.g_weights = go->weights; b.g_transparency = go->transparency;
  b.g_albedo = go->albedo; b.g_sun = go->sun; b.g_sky = go->sky; b.g_beta = go->beta; b.g_sigmas = go->sigmas;
  b.g_beta_s = go->beta_semantic; b.g_logits = go->semantic_logits;
  b.d_sigo = dsig; b.d_fino = dfin; b.d_suno = dsun; b.sky_slab = (p.sc || embed) ? nullptr : ws.f(p.o_skyslab);
  b.zero = ws.u(p.o_kcq); b.zero_n = KCQ_SLOTS * 16;
  RC(launch_composite_bwd(b, st));
  if (!p.sc && !embed)
    RC(red_add_col(rq.col, ws.f(p.o_skyslab), p.comp_blocks * 4, (size_t)p.sky_floats, p.sky_floats, gp + p.sky));


  const PlaneT dz1 = p.dza.view(p.h1w);   // d(pre-activation) of the fused first head layer, [P][h1w]
  const int sun_col = p.sc ? 0 : p.sun_col;
  if (!p.sc) {
    // 1. final head layers: bias gradient + planes of dfin, dW, then dz1[:, :KF] = (dfin . W_fin) * act'
    if (embed) RC(bsp::launch_colsum32_bsp(dfin, P, r.nar_fin, ws.c(p.pdfin.o), ws.i(p.pdfin.e), p.pl, st));   // narrow_grad's plane conversion, its bias sums left in the arena
    else {
      RC(narrow_grad(dfin, r.nar_fin, p.pdfin, gp + p.b_fin));
      RC(dw_gemm(r.w_fin, p.pdfin, NARROW, true, p.h1, 0, p.KF));
      RC(dw_reduce(r.w_fin, (size_t)NARROW * p.KF, gp + p.w_fin));
    }
    bsp::KcArgs g;
    ws.a(g, p.pdfin, NARROW); weights(g, p, pk, p.wj_tfin);
    g.I = P; g.J = p.KF; g.K = NARROW; ws.out(g, dz1);
    dact(g, p.h1);
    colsum(g, r.cs_fin, p.KF);
    if (p.compose_feats) g.ldcs = r.ld_cs1;
    RC(launch_kc(g));
    if (!p.compose_feats && !embed) RC(bias_from_colsum(r.cs_fin, p.KF, gp + p.b_h1));
  }
  if (!embed) {  // 2. sun visibility chain: output layer, layer 3, layer 2
    RC(narrow_grad(dsun, r.nar_sun, p.pdsun, gp + p.b_s4));
    RC(dw_gemm(r.w_s4, p.pdsun, NARROW, true, p.s3, 0, H));
    RC(dw_reduce(r.w_s4, (size_t)NARROW * H, gp + p.w_s4));
    bsp::KcArgs g;
    ws.a(g, p.pdsun, NARROW); weights(g, p, pk, p.wj_ts4);
    g.I = P; g.J = H; g.K = NARROW; ws.out(g, p.dsa);
    dact(g, p.s3);
    colsum(g, r.cs_s3, H);
    RC(launch_kc(g));  // dz_s3
    RC(bias_from_colsum(r.cs_s3, H, gp + p.b_s3));
    RC(dw_gemm(r.w_s3, p.dsa, H, false, p.s2, 0, H));
    RC(dw_reduce(r.w_s3, (size_t)H * H, gp + p.w_s3));
    ws.a(g, p.dsa, H); g.K = H; weights(g, p, pk, p.wj_ts3);
    ws.out(g, p.dsb);
    dact(g, p.s2);
    colsum(g, r.cs_s2, H);
    RC(launch_kc(g));  // dz_s2
    RC(bias_from_colsum(r.cs_s2, H, gp + p.b_s2));
    RC(dw_gemm(r.w_s2, p.dsb, H, false, p.h1, sun_col, H));
    RC(dw_reduce(r.w_s2, (size_t)H * H, gp + p.w_s2));
    ws.a(g, p.dsb, H); weights(g, p, pk, p.wj_ts2);
    ws.out(g, dz1, sun_col);
    dact(g, p.h1, sun_col);
    colsum(g, r.cs_sun, H);
    if (p.compose_feats) g.ldcs = r.ld_cs1;
    RC(launch_kc(g));  // dz1[:, sun block]
    if (!p.compose_feats) RC(bias_from_colsum(r.cs_sun, H, gp + p.b_h1 + (size_t)p.sun_col));
  }
  // d extras[p][c] = sum_j dz1[p][j] W_h1[j][Wf + c] over the blocks whose first layer reads t or t_s (api.hip: head1), summed per ray
  auto transient_grads = [&]() {
    const bool want_t = d_t != nullptr, want_ts = d_t_s != nullptr && p.x_ts >= 0;
    if (p.sc) {   // the sun-visibility block reads [feats | sun_d] only: no gradient reaches t / t_s through this pass
      if (want_t) RC(launch_zero_bytes(d_t, (size_t)p.N * p.tau * sizeof(float), st));
      if (want_ts) RC(launch_zero_bytes(d_t_s, (size_t)p.N * p.tau * sizeof(float), st));
    } else if (want_t || want_ts) {
      int b_lo = p.blk_beta, b_hi = p.blk_beta;
      auto use = [&](int blk, bool on) { if (on && blk >= 0) { if (blk < b_lo) b_lo = blk; if (blk > b_hi) b_hi = blk; } };
      use(p.blk_rgb, p.rgb_t); use(p.blk_sem, p.sem_t || p.sem_ts); use(p.blk_sbeta, true);
      const int k_lo = b_lo * H, k_n = (b_hi + 1 - b_lo) * H;
      float* dext = ws.f(p.o_dfin);      // [P][32] fp32: the final-layer gradients that lived here were consumed in step 1
      bsp::KcArgs x;
      ws.a(x, dz1, k_n, k_lo); weights(x, p, pk, p.wj_th1, p.Wf, k_lo);
      x.I = P; x.J = p.Xp; x.K = k_n; x.Cf = dext;
      RC(bsp::launch_kc_narrow(x, st));
      if (want_t) RC(launch_ray_sum32(dext, p.x_t, p.N, p.S, p.tau, d_t, st));
      if (want_ts) RC(launch_ray_sum32(dext, p.x_ts, p.N, p.S, p.tau, d_t_s, st));
    }
    return (int)SNERF_OK;
  };
  if (embed) return transient_grads();   // (it reads dz1 in [k_lo, k_lo + k_n), inside [0, KF): the sun block's columns are unwritten in this pass)
  PlaneT dz_cur = p.dza.view(W);   // dz of the trunk layers, [P][W], in dza and dzb in turn (dz1 is dead by then)
  PlaneT dz_nxt = p.dzb.view(W);
  // The density branch carries a gradient only if one reaches weights / transparency (/ sigmas, depth, rgb, logits in the main
  // pass).  In the solar-correction pass of a training step none does: the loss detaches T' and w' (baseline/components/loss.py:8-10)
  // and the composite backward then writes d sigma = 0 exactly -- its bias sums, its dW launch and the 32 extra contraction columns
  // of the dX launch are skipped (SURVEY 8(d) counts the sc backward "through sun_v / feats / trunk only").
  const bool sig_live = !p.sc || go->weights != nullptr || go->transparency != nullptr || go->sigmas != nullptr;
  const PlaneT& hl = p.h[p.L - 1];
  bool uncompose = false;
  if (p.compose_feats) {
    // 3 + 4, composed: the layer is pre1 = W_c [h_last | extras] + b_c with W_c = [A W_f | W_h1[:, W:]], A = W_h1[:, :W].
    const int r0 = p.sc ? p.sun_col : 0;
    const int nt = (P + 127) / 128, X = p.FA - W;
    // G_c = dz1^T [h_last | extras]: the dW launch as before.  Its extras columns are W_h1's own gradient; its first W columns are
    // summed over the splits INTO the first slab, where the un-compose launch at the end of the pass reads them.
    RC(dw_gemm(r.w_h1, dz1, p.h1w, false, p.fa, 0, p.FA));
    RC(red_add_elem2d(rq.elem, r.w_h1.slab + W, r.w_h1.sp.ns, r.w_h1.stride, p.h1w, X, p.FA, gp + p.w_h1 + (size_t)r0 * p.FA + W, p.FA));
    RC(red_add_elem2d(rq.elem, r.w_h1.slab, r.w_h1.sp.ns, r.w_h1.stride, p.h1w, W, p.FA, r.w_h1.slab, p.FA));
    RC(red_store_last(rq.elem));
    // g_c, the column sums of dz1 (steps 1 and 2 left their partials side by side), into row 0 of the partials
    RC(red_add_col(rq.col, r.cs_fin, nt, (size_t)r.ld_cs1, p.h1w, r.cs_fin));
    RC(red_store_last(rq.col));
    uncompose = true;
    RC(transient_grads());
    // sigma: bias gradient, planes of d sigma, its 32 rows of the [W + 32][W] gradient
    if (sig_live) {
      RC(narrow_grad(dsig, r.nar_sig, p.pdsig, gp + p.b_fs + W));
      RC(dw_gemm(r.w_fs, p.pdsig, NARROW, true, hl, 0, W));
      RC(dw_reduce(r.w_fs, (size_t)NARROW * W, gp + p.w_fs + (size_t)W * W));
    }
    // ONE dX launch for d feats and dz of the last trunk layer:  dz_last = [dz1 | d sigma] [W_c[:, :W]; w_sigma] * act'(h_last).
    // It reads dz1 in dza, so it writes dzb, and the trunk walk below starts there.
    { const PlaneT sw = dz_cur; dz_cur = dz_nxt; dz_nxt = sw; }
    bsp::KcArgs g;
    ws.a(g, dz1, p.h1w);
    if (sig_live) ws.a2(g, p.pdsig);
    weights(g, p, pk, p.wj_th1, 0, r0); g.I = P; g.J = W; g.K = sig_live ? p.h1w + NARROW : p.h1w;
    ws.out(g, dz_cur);
    dact(g, hl, 0, (p.L == 1) ? 30.f : 1.f);
    colsum(g, r.cs_hl, W);
    RC(launch_kc(g));
    RC(bias_from_colsum(r.cs_hl, W, gp + p.b_tr[p.L - 1]));
  }
  const PlaneT dfa = p.dzb.view(p.FA);   // [P][FA]
  if (!p.compose_feats) {  // 3. fused first head layer: dW, then d[feats | extras]
    const int r0 = p.sc ? p.sun_col : 0;
    RC(dw_gemm(r.w_h1, dz1, p.h1w, false, p.fa, 0, p.FA));
    RC(dw_reduce(r.w_h1, (size_t)p.h1w * p.FA, gp + p.w_h1 + (size_t)r0 * p.FA));
    bsp::KcArgs g;
    ws.a(g, dz1, p.h1w); weights(g, p, pk, p.wj_th1, 0, r0);
    // d feats only (J = W): the 16 extras columns would be a third column tile of 256 for 16 useful columns (a third of this
    // launch: 954 -> ~640 us at 4096 x 64), and nothing needs d sun_d.  The gradient of the transient codes comes from a 32-wide
    // launch over the head blocks that read them instead (default: the beta block alone, K = H).
    g.I = P; g.J = W; g.K = p.h1w; ws.out(g, dfa);
    colsum(g, r.cs_fa, p.FA);   // columns [0, W) = bias gradient of feats_from_xyz
    RC(launch_kc(g));
    RC(red_add_col(rq.col, r.cs_fa, (P + 127) / 128, (size_t)cs_ld(p.FA), W, gp + p.b_fs));
    RC(transient_grads());
  }
  if (!p.compose_feats) {  // 4. feats + sigma: dW for the [W + 32][W] matrix, then dz of the last trunk layer (dfa is dead once these launches have read it)
    if (sig_live) RC(narrow_grad(dsig, r.nar_sig, p.pdsig, gp + p.b_fs + W));
    RC(dw_gemm(r.w_fs, dfa, W, false, hl, 0, W));
    if (sig_live) RC(dw_gemm(r.w_fs, p.pdsig, NARROW, true, hl, 0, W, (size_t)W * W));
    RC(dw_reduce(r.w_fs, (size_t)(sig_live ? W + NARROW : W) * W, gp + p.w_fs));
    bsp::KcArgs g;
    ws.a(g, dfa, W);
    if (sig_live) ws.a2(g, p.pdsig);
    weights(g, p, pk, p.wj_tfs); g.I = P; g.J = W; g.K = sig_live ? W + NARROW : W;
    ws.out(g, dz_cur);
    dact(g, hl, 0, (p.L == 1) ? 30.f : 1.f);
    colsum(g, r.cs_hl, W);
    RC(launch_kc(g));
    RC(bias_from_colsum(r.cs_hl, W, gp + p.b_tr[p.L - 1]));
  }
  // 5. trunk, last layer to first
  for (int i = p.L - 1; i >= 0; --i) {
    const BwdRegions::Layer& t = r.tr[i];
    if (i > 0 && ((p.skip_mask >> i) & 1u)) {   // [W_gamma | W_h]: two slab regions (take_regions), each reduced into its columns
      RC(dw_gemm(t.w_gamma, dz_cur, W, false, p.pe, 0, p.Ep));
      RC(dw_gemm(t.w, dz_cur, W, false, p.h[i - 1], 0, W));
      RC(red_add_elem2d(rq.elem, t.w_gamma.slab, t.w_gamma.sp.ns, t.w_gamma.stride, W, p.Ep, p.Ep, gp + p.w_tr[i], p.k_tr[i]));
      RC(red_add_elem2d(rq.elem, t.w.slab, t.w.sp.ns, t.w.stride, W, W, W, gp + p.w_tr[i] + p.Ep, p.k_tr[i]));
    } else {
      if (i == 0) RC(dw_gemm(t.w, dz_cur, W, false, p.pe, 0, p.Ep));
      else RC(dw_gemm(t.w, dz_cur, W, false, p.h[i - 1], 0, W));
      RC(dw_reduce(t.w, (size_t)W * p.k_tr[i], gp + p.w_tr[i]));
    }
    if (i == 0) break;
    bsp::KcArgs g;
    ws.a(g, dz_cur, W); weights(g, p, pk, p.wj_tt[i]);
    g.I = P; g.J = W; g.K = W; ws.out(g, dz_nxt);
    dact(g, p.h[i - 1], 0, (i - 1 == 0) ? 30.f : 1.f);
    colsum(g, t.cs, W);
    RC(launch_kc(g));
    RC(bias_from_colsum(t.cs, W, gp + p.b_tr[i - 1]));
    const PlaneT sw = dz_cur; dz_cur = dz_nxt; dz_nxt = sw;
  }
  RC(launch_reductions(rq.elem, rq.col, st));
  if (!uncompose) return SNERF_OK;
  // Un-compose (after the reductions: G_c and g_c are final), ADDING into the packed gradients as every reduction does:
  //   dW_h1[:, :W] += G_c[:, :W] W_f^T + g_c (x) b_f     db_h1 += g_c     dW_f += A^T G_c[:, :W]     db_f += A^T g_c
  // with this pass's G_c and g_c alone (the sc pass: the sun block's rows of W_h1 / b_h1).
  {
    const size_t r0 = p.sc ? (size_t)p.sun_col : 0;
    bsp::SgTable tb;
    bsp::uncompose_jobs(tb, r.w_h1.slab, r.cs_fin, pk + p.w_h1 + r0 * p.FA, pk + p.w_fs, pk + p.b_fs,
                        gp + p.w_h1 + r0 * p.FA, gp + p.b_h1 + r0, gp + p.w_fs, gp + p.b_fs, W, p.FA, p.h1w);
    return bsp::launch_sgemm(tb, 32, st);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// snerf_density_grad (include/snerf_normals.h): coef * d sigma / d xyz per sample and summed per ray.  The backward of a training pass
// between a cotangent on sigma and the sample positions, as SNERF_FLAG_EMBED_GRAD is the one between the cotangents and t: the composite
// backward with g_sigmas = coef alone, the planes of d sigma, the dX launches down the trunk with the operands backward_bsp gives
// them -- no dW launch, no column sums, no reduction, nothing taken from the reduction arena -- and, at every layer that reads the
// encoding while its dz is live, the encoding-gradient launch of normals.hip.  It writes only what backward_bsp rewrites before it
// reads (the 32-wide gradients and their planes, dza / dzb, the tile counters), so a snerf_backward on the same workspace afterwards
// gives its own bits.
int density_grad_bsp(const Plan& p, const float* pk, const SnerfInputs* in, const float* coef, double* grad_ray, float* grad_sample,
                     void* workspace, void* scratch, hipStream_t st) {
  const Ws ws{(char*)workspace};
  const NormalsScratch ns = normals_scratch(p);
  double* G = reinterpret_cast<double*>((char*)scratch + ns.o_G);
  double* wd = reinterpret_cast<double*>((char*)scratch + ns.o_wd);
  float* part = reinterpret_cast<float*>((char*)scratch + ns.o_part);
  const int P = p.P, W = p.W;
  int kcq = 0;     // (the counters are cleared by the composite backward kernel, the first launch of this pass)
  auto launch_kc = [&](bsp::KcArgs& g) { g.rev = kcq & 1; g.tile_ctr = kcq < KCQ_SLOTS ? ws.i(p.o_kcq) + 16 * kcq++ : nullptr; return bsp::launch_kc(g, st); };
  auto dact = [&](bsp::KcArgs& g, const PlaneT& h, float w0) {
    ws.h(g, h, 0);
    if (p.siren) { g.aux_mode = AUX_SINREC; g.w0 = w0; }
    else g.aux_mode = AUX_RELU_MASK;
  };
  // 0. composite backward: d sigma's pre-activation = coef * softplus'(pre); no other cotangent, no sky slab
  CompBwdArgs b;
  CompArgs& c = b.f;
  c.N = p.N; c.S = p.S; c.H = p.H; c.C = p.C; c.sc = 0; c.sem_sigmoid = p.sem_sigmoid; c.has_sbeta = p.blk_sbeta >= 0;
  c.z = ws.f(p.o_z); c.sigo = ws.f(p.o_sigo); c.fino = ws.f(p.o_fino); c.suno = ws.f(p.o_suno);
  narrow_parts(c, p, pk, ws);
  c.sun_d = in->sun_d; c.sun_stride = in->sun_stride; c.sky = pk + p.sky;
  b.T = ws.f(p.o_T); b.rgbraw = ws.f(p.o_rgbraw);
  b.g_sigmas = coef;
  b.d_sigo = ws.f(p.o_dsig); b.d_fino = ws.f(p.o_dfin); b.d_suno = ws.f(p.o_dsun); b.sky_slab = nullptr;
  b.zero = ws.u(p.o_kcq); b.zero_n = KCQ_SLOTS * 16;
  RC(launch_composite_bwd(b, st));
  // 1. planes of d sigma (the bias sums of the same launch go to scratch and are never read)
  RC(bsp::launch_colsum32_bsp(ws.f(p.o_dsig), P, part, ws.c(p.pdsig.o), ws.i(p.pdsig.e), p.pl, st));
  // 2. dz of the last trunk layer from d sigma alone: K = 32 against the sigma rows of the transposed pack, which lie behind the N1
  //    rows of W_c in a composed plan (api.hip: plan_weights) and behind the W rows of W_f otherwise
  PlaneT dz_cur = p.dza.view(W), dz_nxt = p.dzb.view(W);
  {
    bsp::KcArgs g;
    ws.a(g, p.pdsig, NARROW);
    if (p.compose_feats) weights(g, p, pk, p.wj_th1, 0, p.N1);
    else weights(g, p, pk, p.wj_tfs, 0, W);
    g.I = P; g.J = W; g.K = NARROW; ws.out(g, dz_cur);
    dact(g, p.h[p.L - 1], (p.L == 1) ? 30.f : 1.f);
    RC(launch_kc(g));
  }
  // 3. trunk, last layer to first (backward_bsp step 5 without its dW launches); a skip layer's dz is overwritten two launches later,
  //    so its encoding columns are contracted here, before the launch into the layer below
  const NormalsDump dump = normals_dump();
  if (dump.enc) RC(bsp::launch_from_planes(ws.c(p.pe.o), ws.i(p.pe.e), p.pe.ld, 0, P, p.Ep, dump.enc, p.Ep, p.pl, st));
  int n_enc = 0;
  for (int i = p.L - 1; i >= 0; --i) {
    if (i == 0 || ((p.skip_mask >> i) & 1u)) {
      RC(launch_encgrad_weights(pk + p.w_tr[i], p.k_tr[i], W, p.E, wd, ns.ldw, st));
      EncGradArgs a;
      a.dz = ws.c(dz_cur.o); a.Edz = ws.i(dz_cur.e); a.ld_dz = dz_cur.ld;
      a.pe = ws.c(p.pe.o); a.Epe = ws.i(p.pe.e); a.Ep = p.Ep;
      a.wd = wd; a.ldw = ns.ldw; a.G = G; a.P = P; a.W = W; a.F = p.F; a.first = n_enc == 0;
      RC(launch_encgrad(a, st));
      if (dump.dz) RC(bsp::launch_from_planes(a.dz, a.Edz, a.ld_dz, 0, P, W, dump.dz + (size_t)n_enc * P * W, W, p.pl, st));
      ++n_enc;
    }
    if (i == 0) break;
    bsp::KcArgs g;
    ws.a(g, dz_cur, W); weights(g, p, pk, p.wj_tt[i]);
    g.I = P; g.J = W; g.K = W; ws.out(g, dz_nxt);
    dact(g, p.h[i - 1], (i - 1 == 0) ? 30.f : 1.f);
    RC(launch_kc(g));
    const PlaneT sw = dz_cur; dz_cur = dz_nxt; dz_nxt = sw;
  }
  // 4. per ray
  return launch_ray_fold3(G, p.N, p.S, grad_ray, grad_sample, st);
}

}  // namespace snerf
