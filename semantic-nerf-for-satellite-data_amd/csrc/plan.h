// Host-side layout plan: packed parameter offsets and workspace regions derived from a SnerfDesc.
// Everything the kernels index is computed here once per call, so host code can check every
// operand shape before a launch (a faulting kernel can reset the node).
#pragma once
#include "bsp.h"
#include "common.h"
#include "../../include/snerf_hip.h"

namespace snerf {

constexpr int NARROW = 32;   // padded width of the 1..(5+C)-wide head outputs
constexpr int MAX_CLASSES = 16;
constexpr int ND_FIN = 5;       // projections per column tile of a folded final-layer launch (bsp_kc.hip: NDOT = 5)
constexpr int MAX_SKY_UNITS = 8;  // feat_last <= 512 (units per lane in the composite kernels)

// One block-scaled plane tensor of the workspace (csrc/bsp.h), byte offsets: its planes [Pp][ld], its exponent table and, for the
// activations a SIREN training pass keeps, the sign words of cos (0: none).  ld is the leading dimension it was allocated with and
// the only one it is ever used with.
struct PlaneT { size_t o = 0, e = 0, s = 0; int ld = 0; };
// Backward scratch sized for the widest gradient tensor (maxw columns).  It is VIEWED at the leading dimension of the tensor that
// lives in it at the time (h1w, W, FA) -- the exponent table is indexed by that ld -- so it has none of its own: view(ld) at the use site.
struct PlaneScratch {
  size_t o = 0, e = 0; int maxw = 0;
  PlaneT view(int ld) const { PlaneT t; t.o = o; t.e = e; t.ld = ld; return t; }
};

struct Plan {
  // dims
  int N = 0, S = 0, P = 0, Pp = 0;
  int W = 0, H = 0, L = 0, E = 0, Ep = 0, F = 0, tau = 0, C = 0;
  bool siren = false, train = false, sc = false, sem_sigmoid = false;
  bool relight = false;   // SNERF_FLAG_RELIGHT: the sun-dependent launches alone, on the workspace of a finished inference main pass (same layout)
  bool embed_grad = false;   // SNERF_FLAG_EMBED_GRAD: snerf_backward writes d_t / d_t_s alone (bsp_pass.hip); forward and every size as without it
  bool geometry = false;   // SNERF_FLAG_GEOMETRY: depths, encoding, trunk, sigma and the composite alone (inference); the workspace holds no head tensor
  bool depth_median = false;   // SNERF_FLAG_DEPTH_MEDIAN: one launch behind an inference pass's composite rewrites out->depth (raymedian.hip); sizes and workspace as without it
  unsigned skip_mask = 0;
  // extras columns appended to the feats buffer: [sun(3) | t(tau) | t_s(tau)] padded to 4
  int x_sun = 0, x_t = 3, x_ts = -1, Xp = 0, FA = 0;
  // first head layers fused into one GEMM: blocks of H rows; sun block last
  int nblk = 0, blk_rgb = 0, blk_sem = -1, blk_beta = -1, blk_sbeta = -1, blk_sun = -1;
  int N1 = 0;   // rows of the fused first-head-layer matrix = KF + H
  int KF = 0;   // contraction length of the block-diagonal final-layer matrix: all blocks but sun, (nblk - 1) H, rounded up to
                // 128 so that the sun block starts on an exponent block
  int sun_col = 0;  // first row of the sun block in the fused first-layer matrix / its column in the h1 buffer (= KF)
  int Wf = 0;   // column of the extras block [sun | t | t_s] behind the feats columns: W rounded up to 128
  bool rgb_t = false, sem_t = false, sem_ts = false, sbeta_ts = false;
  // final-layer output columns inside the NARROW-wide buffer
  static constexpr int col_rgb = 0, col_beta = 3, col_sbeta = 4, col_sem = 5;

  // packed parameter layout (float offsets). weights: row-major [rows][ld]
  size_t w_tr[SNERF_MAX_LAYERS] = {0}, b_tr[SNERF_MAX_LAYERS] = {0};
  int k_tr[SNERF_MAX_LAYERS] = {0};
  size_t w_fs = 0, b_fs = 0;        // [W + NARROW][W]: feats rows then sigma row
  size_t w_h1 = 0, b_h1 = 0;        // [N1][FA]
  size_t w_s2 = 0, b_s2 = 0, w_s3 = 0, b_s3 = 0;  // [H][H]
  size_t w_s4 = 0, b_s4 = 0;        // [NARROW][H], row 0 used
  size_t w_fin = 0, b_fin = 0;      // [NARROW][KF]
  size_t sky = 0;                   // [H][4] w0 | [H] b0 | [4][H] w2 | [4] b2
  int sky_floats = 0;
  size_t n_fp32 = 0;         // floats of the fp32 region (the parameters; gradients use the same layout); the weight packs follow it
  size_t packed_floats = 0;  // whole packed buffer in floats: fp32 region + WF16 packs + exponents
  int pl = 2;        // fp16 planes of every activation tensor and weight pack (csrc/bsp.h): 2 = the default arithmetic (SNERF_FLAG_F16X2),
                     // 1 = SNERF_FLAG_F16X1 (reduced precision)

  // workspace layout (byte offsets)
  size_t o_z = 0, o_T = 0, o_rgbraw = 0;
  // block-scaled plane tensors: gamma(x) [Ep], [feats | sun | t | t_s] [FA], the fused first head layer [h1w], the sun-visibility
  // layers 2, 3 [H], the trunk layers [W] (inference: two buffers in turn)
  PlaneT pe, fa, h1, s2, s3, h[SNERF_MAX_LAYERS];
  size_t o_sigo = 0, o_fino = 0, o_suno = 0;
  // sigma / sun-visibility pre-activations as partial dot products of the producing SIREN launches' epilogues (bsp_kc.hip: NDOT):
  // [4 * (W / 256)][Pp] and [4 * (H / 256)][Pp] floats; folded when the producing layer is a SIREN layer of whole 256-column tiles
  size_t o_sigpart = 0, o_sunpart = 0, o_finpart = 0;
  bool nd_sig = false, nd_sun = false;
  // the whole SIREN trunk as ONE persistent launch with the activation tile resident in LDS (bsp_trunk.hip): one plane, W = 512, gamma
  // of 64 columns; training passes leave every layer's planes / sign words for the backward pass (round 5)
  bool fuse_trunk = false;
  bool nd_fin = false;   // the final layers of the rgb / semantic / beta heads ride in the fused first head layer's epilogue (H = 256: one column tile per head)
  // backward scratch: two regions of the widest gradient tensor, two of the sun-visibility chain [H], the 32-wide pre-activation
  // gradients as fp32 (o_d*) and as planes (pd*: the dX / dW operands)
  PlaneScratch dza, dzb;
  PlaneT dsa, dsb, pdsig, pdfin, pdsun;
  size_t o_dsig = 0, o_dfin = 0, o_dsun = 0;
  size_t o_skyslab = 0;
  size_t o_kcq = 0;                 // tile counters of the K-contiguous launches: KCQ_SLOTS slots of 64 bytes, zeroed at the start of a pass
  size_t o_rq = 0, rq_floats = 0;   // reduction arena of the block-scaled plane backward (bsp_pass.hip: per-launch slabs / column-sum partials)
  // weight operands: every K-contiguous GEMM's B (a matrix or its transpose) as a WF16 pack behind the fp32 region of the packed buffer.
  // ONE table: what the pack kernels need (where the fp32 master lies) and what a launch needs (pack offset, rows, K, exponent slot)
  bsp::WPackTable wj = {};
  int wj_tr[SNERF_MAX_LAYERS] = {0}, wj_tt[SNERF_MAX_LAYERS] = {0};
  int wj_fs = 0, wj_sig = 0, wj_tfs = 0, wj_h1 = 0, wj_th1 = 0, wj_s2 = 0, wj_ts2 = 0, wj_s3 = 0, wj_ts3 = 0, wj_s4 = 0, wj_ts4 = 0,
      wj_fin = 0, wj_tfin = 0;
  size_t wp_bytes = 0;                       // plane region size; then WPACK_MAX exponents (int) and WPACK_MAX |max| words
  int h1w = 0;       // width of the h1 buffer in this pass (N1, or H for the sc pass)
  // feats_from_xyz (a Linear with no activation) composed into the fused first head layer: W_c = [W_h1[:, :W] W_f | W_h1[:, W:]],
  // b_c = b_h1 + W_h1[:, :W] b_f, built by the pack (api.hip: snerf_pack_params); the pass then runs no feats launch forward, no feats
  // dW launch and one dX launch less backward, and un-composes the gradient of W_c into those of W_h1 and W_f (bsp_pass.hip).
  // Two planes, feat_last % 32 == 0, N1 + 32 <= 2048, unless SNERF_COMPOSE_FEATS=0 (read when the plan is made).
  bool compose_feats = false;
  int wj_first = 0;          // composed: the leading jobs of wj (h1, th1) are packed from the scratch W_c BEFORE the others, whose packs lie over it
  size_t o_wc = 0;           // float offset (from the packed buffer's start) of the pack-time scratch [N1 + NARROW][FA]: W_c, then the sigma rows
  size_t o_bc = 0;           // float offset of b_c [N1] behind the exponents
  int comp_blocks = 0;
  size_t ws_bytes = 0;
};

// A frame that asks for no beta (full-frame inference: rgb / depth / labels -- eval/extract_pointcloud.py:66-79) does not compute the
// beta block of the fused first head layer: a quarter of that launch.  Only with the finals folded (each block's final rows read
// its own tile only; the 32-wide final launch would contract the unwritten columns) and when beta is the pass's only use of the block.
// (bsp_pass.hip: KcArgs::tj_skip; api.hip notes it per workspace: a relight cannot hand out a beta its base pass never computed.)
inline bool skips_beta_block(const Plan& p, bool want_beta) {
  return p.nd_fin && !p.train && p.H == 256 && p.blk_beta >= 0 && !want_beta && !p.rgb_t && p.blk_sbeta < 0;
}

constexpr int KCQ_SLOTS = 64;
struct DwSplit { int ns = 1; int k_split = 32; };
DwSplit dw_choose_bsp(int P, int rows, int cols, bool narrow_rows);

#define RC(expr) do { int _rc = (expr); if (_rc) return _rc; } while (0)   // hand a callee's error code on

// returns SNERF_OK or an error (message via set_error)
int make_plan(const SnerfDesc* d, Plan* pl);

size_t bsp_rq_floats(const Plan& p);   // bsp_pass.hip

}  // namespace snerf
