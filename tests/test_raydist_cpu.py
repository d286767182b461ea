"""CPU-side checks of the distortion loss on the ray weights (include/snerf_hip.h snerf_ray_distortion, csrc/raydist.hip,
ops.ray_distortion, loss_ops.distortion_loss, the training step's gate): the numpy restatement
(tests/raydist_numpy.py, the oracle of tests/test_gpu_raydist.py) against the O(S^2) definition and its autograd gradient in fp64,
closed forms, every bad-ray and clamp rule, every refusal through the binding, the names of the prototype's parameters, and
the gate on a stub pipeline.  No GPU.  (`make -C snerf_amd/csrc raydist-refusals` runs the refusals of the entry point in a
stand-alone host program under ASAN + UBSAN: a make target for CPU machines, not a test.)"""
import types

import numpy as np
import pytest
import torch

from tests import raydist_numpy as RN

SIZES = (1, 2, 7, 64, 65, 130, 1024)
FAMILIES = ("dense", "sparse", "peak", "zero", "two_peaks")
NEAR, FAR = 0.25, 4.0


def composited(rng, z, scale):
    """weights composited from random densities along z, as a pass does: alpha = 1 - exp(-sigma * dz), w = alpha * transmittance"""
    N, S = z.shape
    sigma = rng.uniform(0.0, scale, (N, S)) * (rng.random((N, S)) < (1.0 if scale < 10 else 0.1))
    dz = np.diff(z.astype(np.float64), axis=1, append=z[:, -1:].astype(np.float64) + 1.0)
    alpha = 1.0 - np.exp(-sigma * dz)
    trans = np.cumprod(np.concatenate([np.ones((N, 1)), 1.0 - alpha[:, :-1]], 1), 1)
    return (alpha * trans).astype(np.float32)


def family_weights(rng, z, family):
    """(N, S) fp32 weights of one family; every row sums to at most 1"""
    N, S = z.shape
    if family == "dense":
        return composited(rng, z, 3.0)
    if family == "sparse":
        return composited(rng, z, 60.0)
    w = np.zeros((N, S), np.float32)
    if family == "peak":                                       # three samples, exact zeros elsewhere
        for n in range(N):
            k0 = int(rng.integers(0, max(S - 2, 1)))
            w[n, k0:k0 + 3] = rng.uniform(0.05, 0.3, min(3, S - k0)).astype(np.float32)
    elif family == "two_peaks":                                # a floater in front of a roof
        for n in range(N):
            k0, k1 = int(rng.integers(0, max(S // 3, 1))), int(rng.integers(S - max(S // 3, 1), S))
            w[n, k0] += np.float32(rng.uniform(0.1, 0.4))
            w[n, k1] += np.float32(rng.uniform(0.1, 0.4))
    return w


def make_rays(N, near=NEAR, far=FAR):
    rays = np.zeros((N, 8), np.float32)
    rays[:, 6], rays[:, 7] = near, far
    return rays


def make_depths(rng, N, S):
    return np.sort(rng.uniform(NEAR + 0.05, FAR - 0.05, (N, S)).astype(np.float32), 1)


def direct(weights, z, rays):
    """the O(S^2) definition in torch fp64 and its autograd gradient: L = sum_ij w_i w_j |m_i - m_j| + 1/3 sum_i w_i^2 delta_i"""
    _, delta, m = RN.midpoints(z, rays[:, 6], rays[:, 7])
    w = torch.tensor(np.asarray(weights, np.float32).astype(np.float64), requires_grad=True)
    m, delta = torch.from_numpy(m), torch.from_numpy(delta)
    wc = w.clamp(0.0, 1.0)
    L = (wc[:, :, None] * wc[:, None, :] * (m[:, :, None] - m[:, None, :]).abs()).sum((1, 2)) + (wc * wc * delta).sum(1) / 3.0
    L.sum().backward()
    return L.detach().numpy(), w.grad.numpy()


@pytest.mark.parametrize("S", SIZES)
def test_restatement_against_the_quadratic_definition(S):
    """The bar is derived, not measured: every quantised item (a, b, q) errs by at most 2^-51 and at most a few S of them are summed
    into any result (rows sum to <= 1 and t lies in [0, 1]), so the O(S) form differs from the definition by at most 4 S 2^-50, for
    L_r and for every g_k (the fp64 g_k before it is written as a float).  At S = 1024: 3.6e-12; a run of this test showed 1.8e-14
    for L_r and 4.0e-14 for g."""
    bar = 4 * S * 2.0 ** -50
    rng = np.random.default_rng(S)
    N = 6 if S < 1024 else 3
    worst = [0.0, 0.0]
    for family in FAMILIES:
        z = make_depths(rng, N, S)
        w = family_weights(rng, z, family)
        assert float(w.sum(1).max()) <= 1.0 + 1e-6 and (family != "zero" or not w.any())
        rays = make_rays(N)
        g32, per_ray, acc, g64 = RN.ray_distortion(w, z, rays, return_g64=True)
        L, grad = direct(w, z, rays)
        eL, eg = float(np.abs(per_ray - L).max()), float(np.abs(g64 - grad).max())
        worst = [max(worst[0], eL), max(worst[1], eg)]
        assert eL <= bar and eg <= bar, (family, eL, eg, bar)
        assert np.array_equal(g32, g64.astype(np.float32)) and g32.dtype == np.float32
        assert acc.tolist() == [sum(int(np.rint(v * 2.0 ** 40)) for v in per_ray), N, 0, 0]
        if family == "zero":
            assert not per_ray.any() and not g64.any()
        elif S > 1 and family != "sparse":                     # (a sparse row of a short ray can be empty)
            assert float(per_ray.min()) > 0
    print(f"S = {S}: |L_r - L| <= {worst[0]:.2e}, |g - dL/dw| <= {worst[1]:.2e}, bar {bar:.2e}")


def test_closed_forms():
    """a one-hot at i < S - 1: L = w^2 delta_i / 3; at the last sample: L = 0; two point masses w1 at i < j - 0 and w2 at j:
    L = 2 w1 w2 (m_j - m_i) + (w1^2 delta_i + w2^2 delta_j) / 3 -- all to the 2^-50 quantum of the sums (three quantised items)"""
    S = 9
    z = np.linspace(0.5, 3.5, S, dtype=np.float32)[None, :]
    rays = make_rays(1)
    _, delta, m = RN.midpoints(z, rays[:, 6], rays[:, 7])
    tol = 3 * 2.0 ** -50
    for i, wi in ((0, 1.0), (3, 0.625), (S - 2, 0.3)):
        w = np.zeros((1, S), np.float32)
        w[0, i] = wi
        g, per_ray, _ = RN.ray_distortion(w, z, rays)
        want = float(np.float32(wi)) ** 2 * delta[0, i] / 3.0
        assert abs(per_ray[0] - want) <= tol and want > 0
        # d / d w_i = 2 w delta_i / 3; every other sample feels the mass: 2 w |m_k - m_i|
        k = np.arange(S) != i
        assert abs(float(g[0, i]) - 2.0 * float(np.float32(wi)) * delta[0, i] / 3.0) <= 1e-7
        assert np.allclose(g[0, k], 2.0 * float(np.float32(wi)) * np.abs(m[0, k] - m[0, i]), rtol=0, atol=1e-7)
    w = np.zeros((1, S), np.float32)
    w[0, S - 1] = 0.8
    g, per_ray, acc = RN.ray_distortion(w, z, rays)
    assert per_ray[0] == 0.0 and acc.tolist() == [0, 1, 0, 0] and g[0, S - 1] == 0.0
    w1, w2, i, j = 0.25, 0.5, 2, 6
    w = np.zeros((1, S), np.float32)
    w[0, i], w[0, j] = w1, w2
    _, per_ray, _ = RN.ray_distortion(w, z, rays)
    want = 2 * w1 * w2 * (m[0, j] - m[0, i]) + (w1 * w1 * delta[0, i] + w2 * w2 * delta[0, j]) / 3.0
    assert abs(per_ray[0] - want) <= 2 * tol


def _one(w, z, near=NEAR, far=FAR):
    w, z = np.asarray([w], np.float32), np.asarray([z], np.float32)
    return RN.ray_distortion(w, z, make_rays(1, near, far))


def test_every_bad_ray_rule():
    """a weight or a depth that is not finite, a decreasing depth, near / far not finite, far <= near, a t outside [-1, 2]: a row of
    +0, a per-ray NaN, nothing in word 0, one in words 1 and 2; the rays next to a bad one are untouched by it"""
    z, w = [0.5, 1.0, 1.0, 2.0, 3.0], [0.1, 0.2, 0.0, 0.3, 0.1]
    g_ok, L_ok, acc_ok = _one(w, z)
    assert np.isfinite(L_ok[0]) and L_ok[0] > 0 and acc_ok.tolist()[1:] == [1, 0, 0]         # repeated depths are fine
    inf, nan = np.inf, np.nan
    cases = {"w nan": (w[:2] + [nan] + w[3:], z, NEAR, FAR), "w +inf": ([inf] + w[1:], z, NEAR, FAR), "w -inf": (w[:4] + [-inf], z, NEAR, FAR),
             "z nan": (w, z[:3] + [nan] + z[4:], NEAR, FAR), "z inf": (w, z[:4] + [inf], NEAR, FAR),
             "z decreasing": (w, [0.5, 1.0, 0.99999994, 2.0, 3.0], NEAR, FAR),
             "near nan": (w, z, nan, FAR), "far inf": (w, z, NEAR, inf), "near -inf": (w, z, -inf, FAR),
             "far == near": (w, z, 1.0, 1.0), "far < near": (w, z, FAR, NEAR),
             "t > 2": (w, z[:4] + [NEAR + 2.0 * (FAR - NEAR) + 0.01], NEAR, FAR), "t < -1": (w, [NEAR - (FAR - NEAR) - 0.01] + z[1:], NEAR, FAR)}
    for name, (ww, zz, near, far) in cases.items():
        g, L, acc = _one(ww, zz, near, far)
        assert np.array_equal(g.view(np.uint32), np.zeros((1, 5), np.uint32)), name
        assert L.view(np.uint64)[0] == RN.NAN_BITS and acc.tolist() == [0, 1, 1, 0], name
    # t exactly -1 and exactly 2 are inside
    _, L, acc = _one(w, [-1.0, 0.0, 0.5, 1.0, 2.0], 0.0, 1.0)
    assert np.isfinite(L[0]) and acc.tolist()[1:] == [1, 0, 0]
    # in a batch: the good rows equal their single-ray results, the words add up
    W = np.asarray([w, w[:2] + [nan] + w[3:], w], np.float32)
    Z = np.asarray([z, z, z], np.float32)
    g, L, acc = RN.ray_distortion(W, Z, make_rays(3))
    assert np.array_equal(g[0], g_ok[0]) and np.array_equal(g[2], g_ok[0]) and not g[1].any()
    assert L[0] == L[2] == L_ok[0] and np.isnan(L[1]) and acc.tolist() == [2 * int(acc_ok[0]), 3, 1, 0]


def test_every_clamp_rule():
    """w < 0 counts as 0 and w > 1 as 1, both with a gradient of +0 (the clamp's derivative); an exact 0 of either sign and an exact
    1 keep the formula; the other samples' gradients see the clamped masses"""
    z = [0.5, 1.0, 1.5, 2.0, 3.0]
    g_a, L_a, _ = _one([0.1, -1.0, 0.2, 2.0, 0.1], z)
    g_b, L_b, _ = _one([0.1, 0.0, 0.2, 1.0, 0.1], z)
    assert L_a[0] == L_b[0]
    assert np.array_equal(g_a[0, [0, 2, 4]], g_b[0, [0, 2, 4]])
    assert g_a[0, 1].view(np.uint32) == 0 and g_a[0, 3].view(np.uint32) == 0
    assert g_b[0, 1] != 0 and g_b[0, 3] != 0                                                  # exact 0 and exact 1: the formula
    g_c, L_c, _ = _one([0.1, -0.0, 0.2, 1.0, 0.1], z)                                         # -0 is +0
    assert L_c[0] == L_b[0] and np.array_equal(g_c.view(np.uint32), g_b.view(np.uint32))
    assert RN.clamp(np.asarray([-0.0, 0.0, -3.0, 0.5, 1.0, 7.0], np.float32)).view(np.uint64).tolist() == \
        np.asarray([0.0, 0.0, 0.0, 0.5, 1.0, 1.0]).view(np.uint64).tolist()
    # all-zero weights: value 0, gradient +0 everywhere (every term has a zero factor)
    g, L, acc = _one([0.0] * 5, z)
    assert L[0] == 0.0 and not g.any() and acc.tolist() == [0, 1, 0, 0]


def test_loss_chain_is_the_spec():
    acc = np.array([(-5 * 2 ** 40) % 2 ** 64, 4, 1, 0], np.uint64)                           # word 0 is an int64
    term, scale = RN.loss_chain(acc, 0.01)
    assert term.dtype == scale.dtype == np.float32
    assert term == np.float32((0.01 * -5.0) / 4.0) and scale == np.float32(0.01 / 4.0)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
DUMMY = 4096        # a non-null address no refusal path dereferences


def _call(w=DUMMY, z=DUMMY, rays=DUMMY, stride=8, n=2, s=6, dw=DUMMY, per_ray=DUMMY, acc=DUMMY):
    from snerf_amd import _lib
    return _lib.lib().snerf_ray_distortion(w, z, rays, stride, n, s, dw, per_ray, acc, None)


REFUSALS = [
    ("null-weights", lambda: _call(w=None), 3, "weights is NULL"),
    ("null-z_vals", lambda: _call(z=None), 3, "z_vals is NULL"),
    ("null-rays", lambda: _call(rays=None), 3, "rays is NULL"),
    ("null-d_weights", lambda: _call(dw=None), 3, "d_weights is NULL"),
    ("null-acc", lambda: _call(acc=None), 3, "acc is NULL"),
    ("null-acc-and-per_ray", lambda: _call(acc=None, per_ray=None), 3, "acc is NULL"),
    ("N0", lambda: _call(n=0), 1, "n_rays = 0"),
    ("N-neg", lambda: _call(n=-7), 1, "n_rays = -7"),
    ("N-2^22+1", lambda: _call(n=2 ** 22 + 1), 1, "n_rays = 4194305"),
    ("S0", lambda: _call(s=0), 1, "n_samples = 0"),
    ("S-neg", lambda: _call(s=-1), 1, "n_samples = -1"),
    ("S1025", lambda: _call(s=1025), 1, "n_samples = 1025"),
    ("stride7", lambda: _call(stride=7), 1, "ray_stride = 7"),
    ("stride-neg", lambda: _call(stride=-8), 1, "ray_stride = -8"),
]


@pytest.mark.parametrize("call,code,needle", [r[1:] for r in REFUSALS], ids=[r[0] for r in REFUSALS])
def test_every_refusal_returns_its_code_and_a_message(call, code, needle):
    """all before the device is touched (the addresses are dummies), each with a message that names the argument"""
    from snerf_amd import _lib
    assert call() == code
    msg = _lib.lib().snerf_last_error().decode()
    assert needle in msg and msg.startswith("snerf_ray_distortion: "), msg


def test_the_limits_are_the_headers():
    from snerf_amd import _lib
    assert _lib.VIS_MAX_SAMPLES == RN.MAX_SAMPLES == 1024 and RN.MAX_RAYS == 2 ** 22


def test_entry_is_in_the_one_header_and_table():
    """snerf_ray_distortion is declared in include/snerf_hip.h and bound by a row of _lib.SIGNATURES like every other entry, so
    tests/test_abi_cpu.py compares the two type by type.  What that test does not pin: the parameter names (the keys of the pointer
    roles in tests/test_gpu_fill.py and the words of the refusal messages), and that the entry came at ABI version 6."""
    from snerf_amd import _lib
    from tests.test_abi_cpu import _header_prototypes
    _, params = _header_prototypes()["snerf_ray_distortion"]
    assert [n for _, n in params] == ["weights", "z_vals", "rays", "ray_stride", "n_rays", "n_samples", "d_weights", "per_ray", "acc",
                                      "stream"]
    assert "snerf_ray_distortion" in _lib.SIGNATURES and "snerf_ray_distortion" in _lib._PLANS
    assert _lib.lib().snerf_version() == _lib.ABI_VERSION == 6


def test_ops_and_loss_refusals():
    from snerf_amd import loss_ops, ops
    w, z, rays = torch.zeros(5, 6), torch.zeros(5, 6), torch.zeros(5, 8)
    with pytest.raises(RuntimeError, match=r"'weights' must live on the GPU \(the HIP path has no CPU fallback\)"):
        ops.ray_distortion(w, z, rays)
    with pytest.raises(RuntimeError, match=r"must live on the GPU"):
        ops.ray_distortion(w, z, rays, per_ray=True)
    with pytest.raises(RuntimeError, match=r"must live on the GPU"):
        loss_ops.distortion_loss(w.requires_grad_(True), z, rays, 0.01)


def test_config_fields():
    from pydantic import ValidationError
    from snerf_amd.baseline.pipelines.satnerf import NeRFConfig, SatNeRFConfig
    from snerf_amd.semantic.pipelines.rs_semantic import RSSemanticConfig
    for cls in (NeRFConfig, SatNeRFConfig, RSSemanticConfig):
        c = cls()
        assert c.lambda_dist == 0.0 and c.dist_start_epoch == 0 and "lambda_dist" not in c.model_fields_set      # the default: off
        c = cls(lambda_dist=0.01, dist_start_epoch=3)
        assert c.lambda_dist == 0.01 and c.dist_start_epoch == 3 and "lambda_dist" in c.model_fields_set
        with pytest.raises(ValidationError, match="lambda_dist must be >= 0"):
            cls(lambda_dist=-0.5)
        with pytest.raises(ValidationError, match="dist_start_epoch must be >= 0"):
            cls(dist_start_epoch=-1)


# ---- the training step's gate ---------------------------------------------------------------------------------------------------------
class _StubPipeline:
    """what color_and_depth_losses and main_pass touch of a pipeline: the config, the epoch, a colour loss, the log, the forward"""

    def __init__(self, epoch, **keys):
        self.cfgs = types.SimpleNamespace(pipeline=types.SimpleNamespace(first_beta_epoch=0, depth_enabled=False, **keys))
        self.epoch, self.logged, self.forwards = epoch, {}, []
        self.loss = self.loss_without_beta = lambda results, rgbs: (torch.tensor(2.0), {"coarse_color": torch.tensor(2.0)})
        self.results = {"rgb_coarse": torch.zeros(3, 3), "weights_coarse": torch.rand(3, 4), "z_vals_coarse": torch.rand(3, 4)}

    def get_current_epoch(self):
        return self.epoch

    def log(self, name, value, **kw):
        self.logged[name] = value

    def __call__(self, data, render_options=None):
        self.forwards.append((data, render_options))
        return dict(self.results) if render_options else {k: v for k, v in self.results.items() if k != "z_vals_coarse"}


def _gate(monkeypatch, epoch, **keys):
    from snerf_amd import loss_ops
    from snerf_amd.baseline.components.training_step import SatNeRFTrainingStep
    calls = []

    def fake(weights, z_vals, rays, lam, sync=True):
        calls.append((weights, z_vals, rays, lam, sync))
        return torch.tensor(0.5), torch.tensor(0.5)
    monkeypatch.setattr(loss_ops, "distortion_loss", fake)
    pipe = _StubPipeline(epoch, **keys)
    batch = {"rgb": {"rays": torch.rand(3, 8), "extras": torch.rand(3, 4), "rgbs": torch.rand(3, 3)}}
    results, loss, terms = SatNeRFTrainingStep().training_step(pipe, batch, 0)
    return pipe, batch, calls, results, loss, terms


def test_training_step_gate(monkeypatch):
    """no key, or lambda_dist = 0: distortion_loss is never called, the forward is called as before (one argument) and nothing new is
    logged unless the key is configured; before dist_start_epoch: not called, 0.0 logged; from dist_start_epoch on: called once, with
    the main pass's weights and depths and the batch's rays, its total added and its term in the loss dict"""
    pipe, _, calls, results, loss, terms = _gate(monkeypatch, 5)
    assert not calls and pipe.forwards[0][1] is None and len(pipe.forwards) == 1 and "z_vals_coarse" not in results
    assert float(loss) == 2.0 and set(terms) == {"coarse_color"} and set(pipe.logged) == {"train/beta_loss_activated"}
    pipe, _, calls, results, loss, terms = _gate(monkeypatch, 5, lambda_dist=0.0)
    assert not calls and pipe.forwards[0][1] is None and float(loss) == 2.0 and set(terms) == {"coarse_color"}
    assert pipe.logged["train/distortion_loss_activated"] == 0.0
    pipe, _, calls, results, loss, terms = _gate(monkeypatch, 2, lambda_dist=0.01, dist_start_epoch=3)
    assert not calls and pipe.forwards[0][1] is None and float(loss) == 2.0 and set(terms) == {"coarse_color"}
    assert pipe.logged["train/distortion_loss_activated"] == 0.0
    for epoch, keys in ((3, dict(lambda_dist=0.01, dist_start_epoch=3)), (0, dict(lambda_dist=0.01))):
        pipe, batch, calls, results, loss, terms = _gate(monkeypatch, epoch, **keys)
        assert len(calls) == 1 and len(pipe.forwards) == 1 and pipe.forwards[0][1] == {"return_z_vals": True}
        w, z, rays, lam, sync = calls[0]
        assert w is pipe.results["weights_coarse"] and z is pipe.results["z_vals_coarse"] and rays is batch["rgb"]["rays"]
        assert lam == 0.01 and sync is True
        assert float(loss) == 2.5 and set(terms) == {"coarse_color", "coarse_distortion"} and float(terms["coarse_distortion"]) == 0.5
        assert pipe.logged["train/distortion_loss_activated"] == 1.0
    # a pydantic config that leaves the key at its default logs nothing new: today's step
    from snerf_amd.baseline.pipelines.satnerf import SatNeRFConfig
    from snerf_amd.baseline.components.training_step import _key_is_configured
    assert not _key_is_configured(SatNeRFConfig(), "lambda_dist") and _key_is_configured(SatNeRFConfig(lambda_dist=0.0), "lambda_dist")
