// Test hooks of the C-ABI (include/snerf_hip.h: snerf_test_*): scaffolding around single kernels, never on the product path.
#include "aux_kernels.h"
#include "bsp.h"
#include "plan.h"

using namespace snerf;

namespace {
struct DevBuf {
  void* p = nullptr;
  ~DevBuf() { if (p) (void)hipFree(p); }
  int alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 16) == hipSuccess ? 0 : 1; }
  template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};
#define TALLOC(buf, bytes) do { if ((buf).alloc(bytes)) { set_error("test hook: hipMalloc failed"); return SNERF_ERR_HIP; } } while (0)
}  // namespace

extern "C" {

// ---- test hooks of the block-scaled plane kernels (tests/test_gpu_bsp.py): fp32 in / fp32 out around ONE launch of the
// kernel under test; the conversions run through the library's own to_planes / from_planes / weight pack.  Synchronous,
// allocating -- never on the product path.

int snerf_test_bsp_roundtrip(const float* src, int rows, int cols, int ld, int col0, float* dst, int* exps_out, int planes, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  DevBuf pl, E;
  const size_t rp = round_up_sz(rows, 128);
  TALLOC(pl, bsp::plane_bytes(rp, ld, planes)); TALLOC(E, bsp::etab_ints(rp, ld) * 4);
  SNERF_HIP_CHECK(hipMemsetAsync(E.p, 0, bsp::etab_ints(rp, ld) * 4, st));
  RC(bsp::launch_to_planes(src, cols, rows, cols, pl.as<char>(), E.as<int>(), ld, col0, planes, st));
  RC(bsp::launch_from_planes(pl.as<char>(), E.as<int>(), ld, col0, rows, cols, dst, cols, planes, st));
  if (exps_out) SNERF_HIP_CHECK(hipMemcpyAsync(exps_out, E.p, bsp::etab_ints(rp, ld) * 4, hipMemcpyDeviceToDevice, st));
  SNERF_HIP_CHECK(hipStreamSynchronize(st));
  return SNERF_OK;
}

// persistent grid of the K-contiguous launches: n workgroups instead of two per CU (0: default) -- small test problems then walk
// several tiles per workgroup and draw them from the tile counters
int snerf_test_set_kc_grid(int n) { bsp::kc_set_grid_override(n); bsp::trunk_set_grid_override(n); return SNERF_OK; }
// 0: every pass takes the launch-per-layer path (the fused trunk of bsp_trunk.hip is compared with it bit for bit); 1: default
int snerf_test_set_trunk_fusion(int on) { bsp::trunk_set_fusion(on); return SNERF_OK; }

// C[I][J] = epilogue(A[I][Ka] | A2[I][K-Ka]) . W[J][K]^T).  The A tensors are placed at column a_col0 of wider plane
// tensors and the output at column c_col0 (exercises the column-offset / exponent-block arithmetic).
int snerf_test_bsp_kc(const float* A, const float* A2, int Ka, const float* W, const float* bias, int I, int J, int K, int a_col0,
                      int c_col0, int act, float w0, int aux_mode, const float* Hact, const unsigned* Hsign, float* C,
                      unsigned* Csign, float* colsum, const float* nd_w, float* nd_out, const int* nd_rows, int narrow, int planes, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (K % 16 || Ka % 16 || Ka <= 0 || Ka > K) { set_error("test_bsp_kc: K, Ka % 16"); return SNERF_ERR_BAD_DESC; }
  if (planes != 1 && planes != 2) { set_error("test_bsp_kc: planes"); return SNERF_ERR_BAD_DESC; }
  const int pl = planes;
  const size_t rp = round_up_sz(I, 128);
  const int lda = a_col0 + Ka, lda2 = K > Ka ? K - Ka : 16, ldc = c_col0 + round_up(J, 16);
  DevBuf pa, ea, pa2, ea2, wp, we, wm, pc, ec, ph, eh;
  // (+ 64 pad columns: a one-plane launch whose K is an odd multiple of 16 reads -- against zero weights -- up to 16 columns
  //  beyond K; in the passes those are the next row's columns, here they must not be uninitialised memory)
  TALLOC(pa, bsp::plane_bytes(rp + 1, lda, pl)); TALLOC(ea, bsp::etab_ints(rp, lda) * 4);
  TALLOC(pa2, bsp::plane_bytes(rp + 1, lda2, pl)); TALLOC(ea2, bsp::etab_ints(rp, lda2) * 4);
  SNERF_HIP_CHECK(hipMemsetAsync(pa.p, 0, bsp::plane_bytes(rp + 1, lda, pl), st));
  SNERF_HIP_CHECK(hipMemsetAsync(pa2.p, 0, bsp::plane_bytes(rp + 1, lda2, pl), st));
  RC(bsp::launch_to_planes(A, Ka, I, Ka, pa.as<char>(), ea.as<int>(), lda, a_col0 & ~127, pl, st));
  if (a_col0 & 127) { set_error("test_bsp_kc: a_col0 % 128"); return SNERF_ERR_BAD_DESC; }
  if (K > Ka) RC(bsp::launch_to_planes(A2, K - Ka, I, K - Ka, pa2.as<char>(), ea2.as<int>(), lda2, 0, pl, st));
  bsp::WPackTable tb; tb.n = 1;
  tb.j[0] = bsp::WPackJob{0ull, K, J, K, 0, 0ull, 0, J, K};
  TALLOC(wp, bsp::wp16_bytes(J, K, pl)); TALLOC(we, bsp::WPACK_MAX * 4); TALLOC(wm, bsp::WPACK_MAX * 4);
  RC(bsp::launch_wpack(tb, W, wp.as<char>(), we.as<int>(), wm.as<unsigned>(), pl, st));
  bsp::KcArgs g;
  g.pl = pl;
  g.A = pa.as<char>(); g.EA = ea.as<int>(); g.lda = lda; g.a_col0 = a_col0; g.Ka = Ka;
  if (K > Ka) { g.A2 = pa2.as<char>(); g.EA2 = ea2.as<int>(); g.lda2 = lda2; g.a2_col0 = 0; }
  g.W = wp.as<char>(); g.EW = we.as<int>(); g.w_rb32 = (J + 31) / 32; g.w_bytes = (unsigned)bsp::wp16_bytes(J, K, pl);
  g.I = I; g.J = J; g.K = K; g.bias = bias; g.act = act; g.w0 = w0;
  if (narrow) {
    g.Cf = C;
    RC(bsp::launch_kc_narrow(g, st));
    SNERF_HIP_CHECK(hipStreamSynchronize(st));
    return SNERF_OK;
  }
  TALLOC(pc, bsp::plane_bytes(rp, ldc, pl)); TALLOC(ec, bsp::etab_ints(rp, ldc) * 4);
  g.C = pc.as<char>(); g.EC = ec.as<int>(); g.ldc = ldc; g.c_col0 = c_col0; g.Csign = Csign;
  if (aux_mode != AUX_NONE) {
    TALLOC(ph, bsp::plane_bytes(rp, ldc, pl)); TALLOC(eh, bsp::etab_ints(rp, ldc) * 4);
    RC(bsp::launch_to_planes(Hact, J, I, J, ph.as<char>(), eh.as<int>(), ldc, c_col0, pl, st));
    g.aux_mode = aux_mode; g.H = ph.as<char>(); g.EH = eh.as<int>(); g.ldh = ldc; g.h_col0 = c_col0; g.Hsign = Hsign;
  }
  g.colsum = colsum; g.ldcs = J;
  g.nd_w = nd_w; g.nd_out = nd_out; g.nd_stride = (unsigned long long)I;
  if (nd_w && nd_rows) {   // several projections per column tile: nd_w [sum rows][J], tile tj's rows follow tile tj - 1's
    g.nd_omax = ND_FIN; g.nd_ldw = J;
    for (int tj = 0, r = 0; tj < (J + 255) / 256 && tj < 8; ++tj) { g.nd_rows[tj] = nd_rows[tj]; g.nd_row0[tj] = r; r += nd_rows[tj]; }
  }
  DevBuf ctr; TALLOC(ctr, 64);
  SNERF_HIP_CHECK(hipMemsetAsync(ctr.p, 0, 64, st));
  g.tile_ctr = ctr.as<int>();
  RC(bsp::launch_kc(g, st));
  RC(bsp::launch_from_planes(pc.as<char>(), ec.as<int>(), ldc, c_col0, I, J, C, J, pl, st));
  SNERF_HIP_CHECK(hipStreamSynchronize(st));
  return SNERF_OK;
}

// C[I][J] = sum_p A[p][a_col0 + i] B[p][b_col0 + j] through split-K slabs + the library's deterministic slab reduction
int snerf_test_bsp_dw(const float* A, int lda_src, const float* B, int ldb_src, int P, int I, int J, int a_col0, int b_col0,
                      int k_split, int narrow_i, float* C, int planes, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (planes == 0) {
    // No planes: the fp32 GEMMs on the WEIGHTS of the composed first head layer, ONE launch with the job table the product builds
    // (bsp.h: compose_jobs / uncompose_jobs), on caller buffers.  I = rows of the layer (block), J = FA, P = W; narrow_i picks the table:
    //   0 compose:     A = [W_h1 [I][FA] | b_h1 [I]],  B = [W_f [P + 32][P] (sigma rows last) | b_f [P]],  C = [W_c [I + 32][FA] | b_c [I]] (written)
    //   1 un-compose:  A = [G_c [I][FA] | g_c [I]],  B = [W_h1 rows [I][FA] | W_f [P][P] | b_f [P]],
    //                  C = [dW_h1 rows [I][FA] | db_h1 [I] | dW_f [P][P] | db_f [P]] (added to)
    const int M = I, FA = J, W = P;
    if (M <= 0 || W <= 0 || FA <= W || !A || !B || !C) { set_error("test_bsp_dw: fp32 weight GEMMs: bad argument"); return SNERF_ERR_BAD_DESC; }
    bsp::SgTable tb;
    if (!narrow_i) bsp::compose_jobs(tb, A, B, B + (size_t)(W + 32) * W, A + (size_t)M * FA, C, C + (size_t)(M + 32) * FA, W, FA, M);
    else bsp::uncompose_jobs(tb, A, A + (size_t)M * FA, B, B + (size_t)M * FA, B + (size_t)M * FA + (size_t)W * W,
                             C, C + (size_t)M * FA, C + (size_t)M * FA + M, C + (size_t)M * FA + M + (size_t)W * W, W, FA, M);
    RC(bsp::launch_sgemm(tb, narrow_i ? 32 : 64, st));
    SNERF_HIP_CHECK(hipStreamSynchronize(st));
    return SNERF_OK;
  }
  if (planes != 1 && planes != 2) { set_error("test_bsp_dw: planes"); return SNERF_ERR_BAD_DESC; }
  const int pl = planes;
  const size_t rp = round_up_sz(P, 128);
  const int lda = round_up(lda_src, 16), ldb = round_up(ldb_src, 16);
  DevBuf pa, ea, pb, eb, slab, tmp;
  TALLOC(pa, bsp::plane_bytes(rp, lda, pl)); TALLOC(ea, bsp::etab_ints(rp, lda) * 4);
  TALLOC(pb, bsp::plane_bytes(rp, ldb, pl)); TALLOC(eb, bsp::etab_ints(rp, ldb) * 4);
  RC(bsp::launch_to_planes(A, lda_src, P, lda_src, pa.as<char>(), ea.as<int>(), lda, 0, pl, st));
  RC(bsp::launch_to_planes(B, ldb_src, P, ldb_src, pb.as<char>(), eb.as<int>(), ldb, 0, pl, st));
  const int ns = (P + k_split - 1) / k_split;
  const size_t stride = round_up_sz((size_t)I * J, 64);
  TALLOC(slab, stride * ns * 4); TALLOC(tmp, 64 * stride * 4);
  bsp::DwArgs g;
  g.A = pa.as<char>(); g.EA = ea.as<int>(); g.lda = lda; g.a_col0 = a_col0;
  g.B = pb.as<char>(); g.EB = eb.as<int>(); g.ldb = ldb; g.b_col0 = b_col0;
  g.I = I; g.J = J; g.P = P; g.C = slab.as<float>(); g.ldc = J; g.k_split = k_split; g.n_split = ns; g.slab_stride = stride; g.pl = pl;
  RC(bsp::launch_dw(g, narrow_i != 0, st));
  SNERF_HIP_CHECK(hipMemsetAsync(C, 0, (size_t)I * J * 4, st));
  RC(reduce_partials(slab.as<float>(), ns, stride, I * J, tmp.as<float>(), C, st));
  SNERF_HIP_CHECK(hipStreamSynchronize(st));
  return SNERF_OK;
}

}  // extern "C"
