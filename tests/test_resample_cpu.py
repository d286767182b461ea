"""CPU-side checks of the depth resampling (include/snerf_hip.h snerf_resample_z, csrc/resample.hip, ops.resample_z; DESIGN.md
section 5p): the numpy restatement (tests/resample_numpy.py, the oracle of tests/test_gpu_resample.py) against the reference's
own sample_pdf (tests/golden/resample_*.npz, recorded by tools/gen_golden_resample.py), the properties of the restatement, and
every refusal -- of the entry point through the binding, of ops.resample_z, of the config and of fit_image_embedding.  No GPU.
(`make -C snerf_amd/csrc resample-refusals` runs the same refusals of the entry point in a stand-alone host program under
ASAN + UBSAN: a make target for CPU machines, like geo-refusals and shadow-refusals, not a test.)"""
import glob
import os
import types

import numpy as np
import pytest
import torch

from tests import resample_numpy as RN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = [f"{kind}_{n}x{s}x{ni}" for n, s, ni in ((64, 64, 64), (16, 7, 5), (8, 130, 200)) for kind in ("det", "rand")]
EPS = 1e-5
SUB_EPS_CAP = 0.05


def _load(case):
    c = dict(np.load(os.path.join(GOLDEN, f"resample_{case}.npz")))
    c.setdefault("u", None)
    return c


def test_every_fixture_is_there():
    have = sorted(os.path.basename(p)[len("resample_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "resample_*.npz")))
    assert have == sorted(CASES)
    assert sum(os.path.getsize(os.path.join(GOLDEN, f"resample_{c}.npz")) for c in CASES) < 400_000


def _reference_bin_pdf(w, Ni, u):
    """the reference's own pdf (sample_pdf: (w + eps) / sum, fp64) of the bin its searchsorted puts each sample in"""
    wd = w[:, 1:-1].astype(np.float64) + EPS
    pdf = wd / wd.sum(1, keepdims=True)
    cdf = np.concatenate([np.zeros((w.shape[0], 1)), np.cumsum(pdf, 1)], 1)
    ud = np.broadcast_to(np.linspace(0.0, 1.0, Ni), (w.shape[0], Ni)) if u is None else u.astype(np.float64)
    k = np.stack([np.clip(np.searchsorted(cdf[n], ud[n], side="right") - 1, 0, pdf.shape[1] - 1) for n in range(w.shape[0])])
    return np.take_along_axis(pdf, k, 1), k


@pytest.mark.parametrize("case", CASES)
def test_restatement_against_the_reference_sample_pdf(case):
    """The spec against the reference's fp64 result.  Where the reference's pdf of a sample's bin is >= 2 eps, the two agree to
    1 fp32 ulp after rounding: the only difference in what is computed is the quantisation of the masses to multiples of 2^-50,
    an error of at most S * 2^-51 of the cdf, i.e. at most S * 2^-51 / (2 eps) < 2e-8 of one bin's width for S <= 1024 -- far
    below the fp32 rounding that follows (derived, not measured).  Below 2 eps the reference's `denom < eps` rule may pin the
    sample to the bin's left edge while the restatement interpolates: there both must lie in the same bin.  The share judged by
    the second rule is capped at 5 % per case, asserted before anything is compared.  The reference's everyday fp32 result is
    recorded next to its fp64 one; its distance is printed, not asserted."""
    c = _load(case)
    z, w, u, ref64 = c["z"], c["weights"], c["u"], c["ref64"]
    N, S = z.shape
    Ni = ref64.shape[1]
    assert set(np.unique(c["family"])) == {0, 1, 2}                               # random, peaked, all zero
    assert bool((w[c["family"] == 2] == 0).all()) and bool(((w[c["family"] == 1] != 0).sum(1) == 3).all())
    assert (u is None) == case.startswith("det")
    pdf, _ = _reference_bin_pdf(w, Ni, u)
    sub = pdf < 2 * EPS
    print(f"{case}: {100 * sub.mean():.2f} % of the samples in bins below 2 eps")
    assert sub.mean() <= SUB_EPS_CAP
    fine, k = RN.fine_samples(z, w, Ni, u, return_bins=True)
    assert fine.dtype == np.float32 and fine.shape == (N, Ni)
    ref_r = ref64.astype(np.float32)
    ulp = np.spacing(np.abs(ref_r)).astype(np.float64)
    err = np.abs(fine.astype(np.float64) - ref_r.astype(np.float64)) / ulp
    far32 = np.abs(c["ref32"].astype(np.float64) - ref64) / ulp
    print(f"{case}: restatement vs the reference's fp64 result, rounded: max {err[~sub].max():.0f} ulp outside the sub-eps bins; "
          f"the reference's own fp32 result lies up to {far32.max():.1f} ulp from its fp64 one (recorded, not asserted)")
    assert bool((err[~sub] <= 1.0).all())
    b = RN.bins(z)
    rows = np.arange(N)[:, None]
    lo, hi = b[rows, k].astype(np.float32), b[rows, k + 1].astype(np.float32)      # rounding is monotone
    assert bool(((fine >= lo) & (fine <= hi))[sub].all())
    assert bool(((ref_r >= lo) & (ref_r <= hi))[sub].all())


def _peak_rays(rng, N, S):
    z = np.sort(rng.uniform(0.5, 3.0, (N, S)).astype(np.float32), 1)
    w = np.zeros((N, S), np.float32)
    k0 = rng.integers(1, S - 3, N)
    for n in range(N):
        w[n, k0[n]:k0[n] + 3] = rng.uniform(0.05, 0.3, 3).astype(np.float32)
    return z, w, k0


@pytest.mark.parametrize("S,Ni", [(7, 5), (64, 64), (33, 100)])
def test_restatement_properties(S, Ni):
    """z_out is non-decreasing and contains every coarse depth bit for bit (as a multiset: the fine samples are the rest), and the
    samples go where the weight is: the peak's three bins are one interval of the cdf of length L = (m[k0] + m[k0+1] + m[k0+2]) / T,
    and a half-open interval of length L holds at least floor(L * Ni) > L * Ni - 1 of the stratum midpoints u_i = (i + 0.5) / Ni:
    the share in the peak's bins is at least L - 1 / Ni.  Uniforms jittered inside their strata can miss both partly covered
    strata: at least L - 2 / Ni.  The regular grid of u = None has the spacing 1 / (Ni - 1): more than L * (Ni - 1) - 1 samples,
    a share of at least L - (1 + L) / Ni."""
    rng = np.random.default_rng(S * 1000 + Ni)
    N = 12
    z, w, k0 = _peak_rays(rng, N, S)
    m = RN.masses(w)
    L = np.array([m[n, k0[n] - 1:k0[n] + 2].sum() / m[n].sum() for n in range(N)])      # weight j is mass j - 1
    assert bool((L > 0.98).all())
    mid = np.broadcast_to(((np.arange(Ni) + 0.5) / Ni).astype(np.float32), (N, Ni))
    jit = ((np.arange(Ni)[None, :] + 0.1 + 0.8 * rng.random((N, Ni))) / Ni).astype(np.float32)      # well inside its stratum
    for u, slack in ((mid, 1.0 / Ni), (jit, 2.0 / Ni), (None, (1.0 + L) / Ni)):
        z_out, fine = RN.resample_z(z, w, Ni, u)
        _, k = RN.fine_samples(z, w, Ni, u, return_bins=True)
        assert z_out.shape == (N, S + Ni) and z_out.dtype == np.float32
        assert bool((np.diff(z_out, axis=1) >= 0).all())
        assert np.array_equal(np.sort(z_out.view(np.uint32), 1), np.sort(np.concatenate([z, fine], 1).view(np.uint32), 1))
        for n in range(N):                                           # every coarse depth, bit for bit, in its order
            rest = list(z_out[n].view(np.uint32))
            for v in z[n].view(np.uint32):
                rest.remove(v)
            assert sorted(rest) == sorted(fine[n].view(np.uint32))
        inside = ((k >= k0[:, None] - 1) & (k <= k0[:, None] + 1)).mean(1)
        assert bool((inside >= L - slack).all()), (inside, L - slack)
        b = RN.bins(z)
        rows = np.arange(N)[:, None]
        assert bool(((fine >= b[rows, k].astype(np.float32)) & (fine <= b[rows, k + 1].astype(np.float32))).all())


def test_restatement_edge_rules():
    """the clamp rule of the weights (NaN, negative and +Inf count as 0, 2.0 as 1), the rule of the uniforms (NaN and everything
    <= 0 is +0, above 1 is 1; u == 1 lands at the right edge of the last bin), ties (coarse before fine) and the signed zeros"""
    w = np.array([[9, np.nan, -1, np.inf, 2.0, 0.25, 9]], np.float32)
    m = RN.masses(w)[0].tolist()
    e = int(np.rint(1e-5 * 2.0 ** 50))
    assert m == [e, e, e, int(np.rint((1.0 + 1e-5) * 2.0 ** 50)), int(np.rint((0.25 + 1e-5) * 2.0 ** 50))]
    z = np.array([[-0.0, 0.0, 1.0, 1.0, 2.0, 3.0, 4.0]], np.float32)
    u = np.array([[np.nan, -3.0, -0.0, 0.0, 1.0, 7.0, np.nextafter(np.float32(1), np.float32(0))]], np.float32)
    z_out, fine = RN.resample_z(z, w, 7, u)
    b = RN.bins(z)[0]
    assert np.array_equal(fine[0, :4].view(np.uint32), np.zeros(4, np.uint32))       # b[0] = 0.5 * (-0 + 0) = +0, f = +0
    assert fine[0, 4] == fine[0, 5] == np.float32(b[-1]) and fine[0, 6] < fine[0, 4]
    assert np.array_equal(z_out[0, :6].view(np.uint32), np.array([0x80000000, 0, 0, 0, 0, 0], np.uint32))   # -0 (coarse) first
    # a fine sample equal to a coarse depth goes behind it: one bin [1, 3], u = 0.5 -> exactly 2
    zz = np.array([[0.0, 2.0, 2.0, 4.0]], np.float32)
    out, f = RN.resample_z(zz, np.ones((1, 4), np.float32), 1, np.array([[0.5]], np.float32))
    assert f[0, 0] == 2.0 and out[0].tolist() == [0.0, 2.0, 2.0, 2.0, 4.0]
    # u = None is the regular grid, 0 for a single sample
    assert np.array_equal(RN.uniforms(None, 2, 5)[1], np.arange(5) / 4.0) and RN.uniforms(None, 1, 1)[0, 0] == 0.0


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
DUMMY = 4096        # a non-null address no refusal path dereferences


def _call(z=DUMMY, w=DUMMY, u=DUMMY, out=DUMMY, fine=DUMMY, n=2, s=6, ni=4):
    from snerf_amd import _lib
    return _lib.lib().snerf_resample_z(z, w, u, out, fine, n, s, ni, None)


REFUSALS = [
    ("null-z", lambda: _call(z=None), 3, "z is NULL"),
    ("null-weights", lambda: _call(w=None), 3, "weights is NULL"),
    ("null-z_out", lambda: _call(out=None), 3, "z_out is NULL"),
    ("null-z_out-and-optionals", lambda: _call(out=None, u=None, fine=None), 3, "z_out is NULL"),
    ("N0", lambda: _call(n=0), 1, "n_rays = 0"),
    ("N-neg", lambda: _call(n=-7), 1, "n_rays = -7"),
    ("S2", lambda: _call(s=2), 1, "n_samples = 2"),
    ("S-neg", lambda: _call(s=-1), 1, "n_samples = -1"),
    ("Ni0", lambda: _call(ni=0), 1, "n_importance = 0"),
    ("Ni-neg", lambda: _call(ni=-3), 1, "n_importance = -3"),
    ("1025", lambda: _call(s=512, ni=513), 1, "n_samples + n_importance = 1025"),
    ("2^32-2", lambda: _call(s=2 ** 31 - 1, ni=2 ** 31 - 1), 1, "n_samples + n_importance = 4294967294"),
]


@pytest.mark.parametrize("call,code,needle", [r[1:] for r in REFUSALS], ids=[r[0] for r in REFUSALS])
def test_every_refusal_returns_its_code_and_a_message(call, code, needle):
    """a NULL z, weights or z_out; n_rays < 1, n_samples < 3, n_importance < 1, n_samples + n_importance > 1024 -- all before the
    device is touched (the addresses are dummies), each with a message that names the argument"""
    from snerf_amd import _lib
    assert call() == code
    msg = _lib.lib().snerf_last_error().decode()
    assert needle in msg and msg.startswith("snerf_resample_z: "), msg


def test_the_limit_is_the_visualisers_limit_on_a_ray():
    from snerf_amd import _lib
    assert _lib.VIS_MAX_SAMPLES == RN.MAX_SAMPLES == 1024


def test_entry_is_in_the_one_header_and_table():
    """snerf_resample_z is declared in include/snerf_hip.h and bound by a row of _lib.SIGNATURES like every other entry, so
    tests/test_abi_cpu.py compares the two type by type.  What that test does not pin: the parameter names (the keys of the pointer
    roles in tests/test_gpu_fill.py and the words of the refusal messages), and that the entry came at ABI version 6."""
    from snerf_amd import _lib
    from tests.test_abi_cpu import _header_prototypes
    _, params = _header_prototypes()["snerf_resample_z"]
    assert [n for _, n in params] == ["z", "weights", "u", "z_out", "z_fine", "n_rays", "n_samples", "n_importance", "stream"]
    assert "snerf_resample_z" in _lib.SIGNATURES and "snerf_resample_z" in _lib._PLANS
    assert _lib.lib().snerf_version() == _lib.ABI_VERSION == 6


def test_ops_resample_z_refusals():
    from snerf_amd import ops
    z, w = torch.zeros(5, 6), torch.zeros(5, 6)
    with pytest.raises(RuntimeError, match=r"'z' must live on the GPU \(the HIP path has no CPU fallback\)"):
        ops.resample_z(z, w, 4)
    with pytest.raises(RuntimeError, match=r"must live on the GPU"):
        ops.resample_z(z, w, 4, u=torch.zeros(5, 4), return_fine=True)


def test_config_refusals():
    from pydantic import ValidationError
    from snerf_amd.baseline.pipelines.satnerf import NeRFConfig, SatNeRFConfig
    from snerf_amd.semantic.pipelines.rs_semantic import RSSemanticConfig
    from snerf_amd.framework.components.rendering import n_render_samples
    for cls in (NeRFConfig, SatNeRFConfig, RSSemanticConfig):
        with pytest.raises(ValidationError, match="n_importance must be >= 0"):
            cls(n_importance=-1)
        with pytest.raises(ValidationError, match="n_samples >= 3"):
            cls(n_samples=2, n_importance=4)
        with pytest.raises(ValidationError, match="<= 1024"):
            cls(n_samples=512, n_importance=513)
        assert n_render_samples(cls(n_samples=512, n_importance=512)) == 1024
        assert n_render_samples(cls(n_samples=3, n_importance=1)) == 4
        assert cls().n_importance == 0 and n_render_samples(cls()) == cls().n_samples      # the default: today's behaviour
        assert n_render_samples(cls(n_samples=1)) == 1 and n_render_samples(cls(n_samples=2000)) == 2000   # untouched without it
    assert n_render_samples(types.SimpleNamespace(n_samples=7)) == 7


def test_renderer_names_its_sample_counts():
    from snerf_amd.framework.components.rendering import BaseRenderer

    class R(BaseRenderer):
        def _model_rendering(self, *a, **k):
            return {}
    r = R(types.SimpleNamespace(pipeline=types.SimpleNamespace(n_samples=7, n_importance=5)))
    assert (r.N_samples, r.N_importance, r.n_render_samples) == (7, 5, 12)
    r = R(types.SimpleNamespace(pipeline=types.SimpleNamespace(n_samples=7)))
    assert (r.N_samples, r.N_importance, r.n_render_samples) == (7, 0, 7)


def test_fit_image_embedding_refuses_n_importance():
    from snerf_amd.eval.utils.embedding import fit_image_embedding
    renderer = types.SimpleNamespace(N_samples=7, N_importance=5)
    with pytest.raises(NotImplementedError, match="n_importance"):
        fit_image_embedding(None, renderer, {}, torch.zeros(4, 8), torch.zeros(4, 4), torch.zeros(4, 3), steps=1, lr=0.1,
                            rays_per_fit=4)
