"""The distortion loss on the ray weights on the device (snerf_ray_distortion, ops.ray_distortion, loss_ops.distortion_loss, the
training step behind `lambda_dist`).  Run with -m gpu on an MI355X.

The bar everywhere is BIT EQUALITY.  The kernel against tests/raydist_numpy.py: the spec is fp64 with every operation rounded on
its own and integer sums, so it has one result.  The training step against a manual chain -- the same step without the term, the
restatement's scaled gradient added to the rendered weights' cotangent: the same kernels on operands that must be bit-identical."""
import types

import numpy as np
import pytest
import torch

from oracle import snerf_oracle as O
from tests import raydist_numpy as RN
from tests.test_raydist_cpu import FAR, NEAR, composited, make_depths, make_rays

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SHAPES = [(1, 1), (5, 2), (77, 7), (130, 64), (33, 65), (9, 130), (2, 1024), (4, 700), (3, 1024), (4096, 64)]
KINDS = 13


def _case(N, S, shift):
    """rows cycle through thirteen kinds: 0 dense, 1 sparse composited weights, 2 a three-sample peak with exact zeros elsewhere, 3 all
    zero, 4 two separated peaks, 5 a NaN weight, 6 an Inf weight, 7 weights of -1 and 2.0 (a good ray: the clamp), 8 a decreasing
    depth (S = 1: a NaN depth), 9 far <= near, 10 a depth far outside the bounds, 11 exact zeros of both signs among dense
    weights, 12 repeated depths"""
    rng = np.random.default_rng(100000 * shift + 1000 * S + N)
    z = make_depths(rng, N, S)
    rays = rng.uniform(-1.0, 1.0, (N, 11)).astype(np.float32)                   # a stride above 8: the ray rows of a scene bank
    rays[:, 6], rays[:, 7] = NEAR, FAR
    dense, sparse = composited(rng, z, 3.0), composited(rng, z, 60.0)
    w = dense.copy()
    for n in range(N):
        kind = (n + shift) % KINDS
        at = int(rng.integers(0, S))
        if kind == 1:
            w[n] = sparse[n]
        elif kind in (2, 3, 4):
            w[n] = 0.0
            if kind == 2:
                k0 = int(rng.integers(0, max(S - 2, 1)))
                w[n, k0:k0 + 3] = rng.uniform(0.05, 0.3, min(3, S - k0)).astype(np.float32)
            elif kind == 4:
                w[n, int(rng.integers(0, max(S // 3, 1)))] = np.float32(rng.uniform(0.1, 0.4))
                w[n, int(rng.integers(S - max(S // 3, 1), S))] = np.float32(rng.uniform(0.1, 0.4))
        elif kind == 5:
            w[n, at] = np.nan
        elif kind == 6:
            w[n, at] = np.inf if n % 2 else -np.inf
        elif kind == 7:
            w[n, at] = -1.0
            w[n, (at + 1) % S] = 2.0
        elif kind == 8:
            if S > 1:
                k = int(rng.integers(0, S - 1))
                z[n, k + 1] = np.nextafter(z[n, k], np.float32(-np.inf))
            else:
                z[n, 0] = np.nan
        elif kind == 9:
            rays[n, 7] = rays[n, 6] if n % 2 else np.float32(NEAR - 1.0)
        elif kind == 10:
            z[n, S - 1] = 1.0e6
        elif kind == 11:
            w[n, ::3] = 0.0
            w[n, 1::3] = -0.0
        elif kind == 12:
            z[n, 1::2] = z[n, 0:S - 1:2]
    return w, z, rays


def _u32(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def _u64(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint64)


def _assert_bits(got, want, what):
    bad = got != want
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist())


@pytest.fixture(scope="module")
def big():
    """the 4096 x 64 case and its restatement, computed once: the kernel test, the sharding test and the loss test share it"""
    w, z, rays = _case(4096, 64, 0)
    return {"w": w, "z": z, "rays": rays, "want": RN.ray_distortion(w, z, rays),
            "dev": tuple(torch.from_numpy(a).to(DEV) for a in (w, z, rays))}


@pytest.mark.parametrize("N,S", SHAPES, ids=[f"{n}x{s}" for n, s in SHAPES])
def test_kernel_equals_the_restatement_bit_for_bit(N, S, big):
    """d_weights, per_ray and the accumulator words, every launch twice (the bits must repeat), with and without per_ray.  A shape
    with fewer rows than kinds is launched once per remaining offset, so every shape sees every kind of row."""
    from snerf_amd import ops
    for shift in range(0, KINDS, min(N, KINDS)):
        if (N, S) == (4096, 64):
            (w, z, rays), (wd, zd, rd), want = (big["w"], big["z"], big["rays"]), big["dev"], big["want"]
        else:
            w, z, rays = _case(N, S, shift)
            wd, zd, rd = (torch.from_numpy(a).to(DEV) for a in (w, z, rays))
            want = RN.ray_distortion(w, z, rays)
        want_g, want_L, want_acc = want
        n_bad = int(want_acc[2])
        assert n_bad == int(np.isnan(want_L).sum()) and (N < KINDS or 0 < n_bad < N)
        for again in range(2):
            g, acc, L = ops.ray_distortion(wd, zd, rd, per_ray=True)
            assert g.shape == (N, S) and g.dtype == torch.float32 and L.shape == (N,) and L.dtype == torch.float64
            assert acc.shape == (4,) and acc.dtype == torch.int64
            what = (shift, again)
            _assert_bits(_u32(g), want_g.view(np.uint32), what + ("d_weights",))
            _assert_bits(_u64(L), want_L.view(np.uint64), what + ("per_ray",))
            assert _u64(acc).tolist() == want_acc.tolist(), what
        g, acc = ops.ray_distortion(wd, zd, rd)                                   # per_ray = NULL
        _assert_bits(_u32(g), want_g.view(np.uint32), (shift, "no per_ray"))
        assert _u64(acc).tolist() == want_acc.tolist()


def test_shards_add_up_to_the_whole_call(big):
    """N = 4096 cut into eight unequal shards, one of them a single ray: accumulated into ONE acc, and into eight that the host folds
    (mod 2^64), the words equal the whole call's; the gradient rows equal the whole call's rows"""
    from snerf_amd import ops
    wd, zd, rd = big["dev"]
    want_g, _, want_acc = big["want"]
    cuts = [0, 1, 300, 1111, 1112, 2000, 2999, 3500, 4096]
    assert len(cuts) == 9 and 1 in np.diff(cuts)
    one = torch.zeros(4, dtype=torch.int64, device=DEV)
    folded = [0, 0, 0, 0]
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        sl = slice(lo, hi)
        g, acc = ops.ray_distortion(wd[sl], zd[sl], rd[sl], acc=one)
        assert acc is one
        _assert_bits(_u32(g), want_g[sl].view(np.uint32), ("one acc", lo, hi))
        g2, own = ops.ray_distortion(wd[sl], zd[sl], rd[sl])
        _assert_bits(_u32(g2), want_g[sl].view(np.uint32), ("own acc", lo, hi))
        folded = [(a + int(b)) % (1 << 64) for a, b in zip(folded, _u64(own))]
    assert _u64(one).tolist() == want_acc.tolist() == folded
    assert int(want_acc[1]) == 4096 and int(want_acc[2]) > 0 and int(want_acc[0]) > 0


def test_no_output_depends_on_bytes_the_library_did_not_write(monkeypatch):
    """the harness of tests/test_gpu_fill.py on the entry's two pure outputs, d_weights and per_ray (weights, z_vals and rays are read
    only; acc is the caller's accumulator, zeroed as the header states): both carry the fill before the launch, under 0x00, 0xFF
    and 0x7B; the results are bit-identical, those of the restatement, and finite wherever the restatement is.  A shape with a
    ragged last workgroup, several samples per lane and bad rays (whose rows and values are written too)."""
    from snerf_amd import ops
    from tests.test_gpu_fill import _finite_where, _poison, run_filled
    N, S = 9, 130
    w, z, rays = _case(N, S, 3)
    wd, zd, rd = (torch.from_numpy(a).to(DEV) for a in (w, z, rays))
    want_g, want_L, want_acc = RN.ray_distortion(w, z, rays)
    assert 0 < int(want_acc[2]) < N

    def run(fill):
        _poison(monkeypatch, fill)
        g, acc, L = ops.ray_distortion(wd, zd, rd, per_ray=True)
        return {"d_weights": g, "per_ray": L, "acc": acc}

    for fill, got in run_filled(run).items():
        _assert_bits(_u32(got["d_weights"]), want_g.view(np.uint32), hex(fill))
        _assert_bits(_u64(got["per_ray"]), want_L.view(np.uint64), hex(fill))
        assert _u64(got["acc"]).tolist() == want_acc.tolist()
        _finite_where(got["d_weights"], torch.from_numpy(want_g), hex(fill))
        _finite_where(got["per_ray"], torch.from_numpy(want_L), hex(fill))


def test_distortion_loss_value_and_gradient(big):
    """the term and, after a backward from a non-unit cotangent, the weight gradient: the restatement through the same fp32 chain
    (term = (float)((lam * (acc0 * 2^-40)) / acc1); gradient = ((float)g * (float)(lam / acc1)) * g_total, each product an fp32 one);
    the depths and the rays get no gradient, and a second backward raises"""
    from snerf_amd import loss_ops
    lam, g_total = 0.01, np.float32(1.75)
    wd, zd, rd = big["dev"]
    want_g, _, want_acc = big["want"]
    term_w, scale = RN.loss_chain(want_acc, lam)
    w = wd.clone().requires_grad_(True)
    z = zd.clone().requires_grad_(True)
    total, term = loss_ops.distortion_loss(w, z, rd, lam)
    assert total.requires_grad and not term.requires_grad and total.dtype == torch.float32 and total.dim() == 0
    assert _u32(total).tolist() == _u32(term).tolist() == np.asarray(term_w).view(np.uint32).tolist() and float(term_w) > 0
    total.backward(torch.tensor(float(g_total), device=DEV), retain_graph=True)
    want = (want_g * scale) * g_total
    assert want.dtype == np.float32
    _assert_bits(_u32(w.grad), want.view(np.uint32), "d weights")
    assert z.grad is None and float(np.abs(want).max()) > 0
    with pytest.raises(RuntimeError, match="second backward through one distortion loss"):
        total.backward()


# ---- the pipeline's training step ------------------------------------------------------------------------------------------------
N_RAYS, S_COARSE, LAM = 77, 7, 0.01


def _step(pipe, pcfg, batch, forward=None):
    """one training step under the pipeline config `pcfg`, jitter and uniforms from a fixed seed -> (loss, the logged terms, the
    activation flag or None, every gradient, the step's results)"""
    keep = pipe.cfgs
    pipe.cfgs = types.SimpleNamespace(run=keep.run, pipeline=pcfg)
    try:
        for p in pipe.parameters():
            p.grad = None
        pipe.logged = {}
        pipe.current_epoch = 0
        torch.manual_seed(3)
        if forward is None:
            out = pipe.training_step(batch, 0)
            out["loss"].backward()
            res = None
        else:
            res = forward()
        torch.cuda.synchronize()
        terms = {k[len("train/"):]: v.detach().clone() for k, v in pipe.logged.items() if k.startswith("train/coarse_")}
        grads = {n: p.grad.clone() for n, p in pipe.named_parameters() if p.grad is not None}
        return (None if forward is not None else out["loss"].detach().clone(), terms, pipe.logged.get("train/distortion_loss_activated"),
                grads, res)
    finally:
        pipe.cfgs = keep
        for p in pipe.parameters():
            p.grad = None


def _same(a, b, what):
    assert set(a) == set(b), (what, sorted(set(a) ^ set(b)))
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, (what, k)
        same = a[k].contiguous().reshape(-1).view(torch.uint8) == b[k].contiguous().reshape(-1).view(torch.uint8)
        assert bool(same.all()), (what, k, f"{int((~same).sum())} of {same.numel()} bytes differ")


@pytest.mark.parametrize("n_importance", [0, 5])
def test_training_step_with_the_distortion_loss(n_importance):
    """fc_units = 64, feat_last = 32, N = 77, S = 7 (+ 5 resampled depths).  lambda_dist = 0: loss, loss dict and every gradient are
    bit-identical to a config without the key.  lambda_dist = 0.01: the loss is the base loss plus the term, the term is the
    restatement's through the fp32 chain, and every parameter gradient and the embedding's equal the manual chain -- the step
    without the term, with the restatement's scaled gradient added to the cotangent of the rendered weights -- bit for bit (fp32
    addition commutes: the order in which autograd sums the two cotangents does not matter)."""
    from tests.test_gpu_pipeline import _batch_to_dev, _pipeline_for
    cfg = O.OracleCfg(fc_units=64, n_samples=S_COARSE, first_beta_epoch=0)
    pipe, _ = _pipeline_for(cfg, 64, 3, n_importance=n_importance, render_chunk_size=4096)
    assert pipe.model_coarse.spec.feat_last == 32 and pipe.model_coarse.spec.mfma == "f16x2"
    full = pipe.cfgs.pipeline
    assert full.lambda_dist == 0.0 and full.dist_start_epoch == 0
    bare = types.SimpleNamespace(**{k: v for k, v in full.model_dump().items() if k not in ("lambda_dist", "dist_start_epoch")})
    batch = _batch_to_dev(O.batch_to_torch(O.synthetic_batch(N_RAYS, S_COARSE, seed=21)))
    S = S_COARSE + n_importance

    loss0, terms0, flag0, grads0, _ = _step(pipe, bare, batch)
    assert flag0 is None and "coarse_distortion" not in terms0 and len(grads0) >= len(pipe.model_coarse.spec.param_names()) + 1
    loss_z, terms_z, flag_z, grads_z, _ = _step(pipe, full.model_copy(update={"lambda_dist": 0.0}), batch)
    assert flag_z == 0.0
    _same({"loss": loss_z}, {"loss": loss0}, "lambda_dist = 0: loss")
    _same(terms_z, terms0, "lambda_dist = 0: loss dict")
    _same(grads_z, grads0, "lambda_dist = 0: gradients")
    loss_l, terms_l, flag_l, grads_l, _ = _step(pipe, full.model_copy(update={"lambda_dist": 0.0, "dist_start_epoch": 0}), batch)
    _same(grads_l, grads0, "lambda_dist = 0 again")

    loss1, terms1, flag1, grads1, _ = _step(pipe, full.model_copy(update={"lambda_dist": LAM}), batch)
    assert flag1 == 1.0 and set(terms1) == set(terms0) | {"coarse_distortion"}
    # before its start epoch the term is off
    _, terms_e, flag_e, grads_e, _ = _step(pipe, full.model_copy(update={"lambda_dist": LAM, "dist_start_epoch": 1}), batch)
    assert flag_e == 0.0 and "coarse_distortion" not in terms_e
    _same(grads_e, grads0, "before dist_start_epoch")

    # the manual chain: the step without the term on a forward that also returns the depths
    module_forward = type(pipe).forward

    def manual():
        pipe.forward = lambda data, render_options=None: module_forward(pipe, data, {"return_z_vals": True})
        try:
            results, base, base_terms = pipe._training_step.training_step(pipe, batch, 0)
        finally:
            del pipe.forward
        w, z = results["weights_coarse"], results["z_vals_coarse"]
        assert w.shape == (N_RAYS, S) and z.shape == (N_RAYS, S) and w.requires_grad and not z.requires_grad
        g, _, acc = RN.ray_distortion(w.detach().cpu().numpy(), z.cpu().numpy(), batch["rgb"]["rays"].cpu().numpy())
        assert acc.tolist()[1:] == [N_RAYS, 0, 0]
        term, scale = RN.loss_chain(acc, LAM)
        gs = g * scale
        assert gs.dtype == np.float32 and float(np.abs(gs).max()) > 0
        torch.autograd.backward([base, w], [torch.ones_like(base), torch.from_numpy(gs).to(DEV)])
        return {"base": base.detach().clone(), "terms": {k: v.detach().clone() for k, v in base_terms.items()}, "term": term}

    _, _, _, grads_m, m = _step(pipe, bare, batch, forward=manual)
    _same({"base": m["base"]}, {"base": loss0}, "the manual chain's base loss")
    _same(m["terms"], terms0, "the manual chain's base terms")
    assert _u32(terms1["coarse_distortion"]).tolist() == np.asarray(m["term"]).view(np.uint32).tolist() and float(m["term"]) > 0
    _same({k: v for k, v in terms1.items() if k != "coarse_distortion"}, terms0, "lambda_dist = 0.01: the other terms")
    want_loss = loss0 + torch.from_numpy(np.asarray(m["term"])).to(DEV)
    _same({"loss": loss1}, {"loss": want_loss}, "lambda_dist = 0.01: loss = base + term")
    assert "model_t.weight" in grads1 and float(grads1["model_t.weight"].abs().max()) > 0
    _same(grads1, grads_m, "lambda_dist = 0.01: gradients vs the manual chain")
    assert any(not torch.equal(grads1[k], grads0[k]) for k in grads0)               # the term does reach the network
