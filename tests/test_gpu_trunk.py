"""The SIREN trunk as one persistent launch (csrc/bsp_trunk.hip; one-plane passes of the W = 512 model) against the
launch-per-layer path it replaces (reference: semantic/models/rs_semantic.py:325-334 inside the chunk loop :63-78).

Both paths issue the same MFMA sequence on the same operands per accumulator, the same FMA / v_sin_f32 / fp16 conversion per element and
the same partial sums of sigma's projection, so the comparison is BIT FOR BIT on every rendered tensor -- and the launch-per-layer path is
the one the oracle-based tests hold to the reference: tests/test_gpu_kernels.py / test_gpu_configs.py at the default depth, and
tests/test_gpu_geometry.py at every depth, skip set and encoding width the plan accepts (one-plane bars: the reference-made yardsticks of
tests/golden/sem_siren_full.npz, see test_gpu_configs.py).

Every geometry the plan sends to the fused kernel is run here (depth 3 ... 8, skips anywhere in 1 ... L - 2, 6 / 10 frequencies; raw xyz
is refused in one-plane mode: tests/test_abi_cpu.py), on forced grids of one and three workgroups that walk many tiles each: the tile-to-tile handover (the next tile's
encoding requested in a late layer's epilogue) is the code under test.  The profiler's launch count of the fused kernel (variant 1)
guards against comparing the launch-per-layer path with itself, and pins where the plan must NOT fuse."""
import ctypes as C

import pytest
import torch

from oracle import snerf_oracle as O
from tests.test_gpu_kernels import _dev, _gpu_params, _spec

pytestmark = pytest.mark.gpu


@pytest.fixture
def lib():
    from snerf_amd import _lib
    L = _lib.lib()
    yield L
    L.snerf_test_set_trunk_fusion(1)
    L.snerf_test_set_kc_grid(0)


def _render(cfg, gp, b, dev, sc):
    from snerf_amd import ops
    spec = _spec(cfg)
    rays, extras, u = b["rays"].to(dev), b["extras"].to(dev), b["u"].to(dev)
    t = torch.zeros(rays.shape[0], cfg.t_embedding_tau, device=dev) + 0.25
    zs = torch.linspace(0, 1, cfg.n_samples).to(dev)
    with torch.no_grad():
        return ops.render_pass(spec, gp, ops.PassInputs(sun_d=extras[:, :3], rays=rays, z_steps=zs, u=u), t, None, sc_pass=sc)


@pytest.mark.parametrize("n_rays,n_samples,grid", [(37, 64, 0), (37, 64, 3), (300, 24, 2), (2048, 64, 0)])
def test_fused_trunk_equals_layer_per_launch_bit_for_bit(n_rays, n_samples, grid, lib, monkeypatch):
    """ragged tiles (37 x 64 = 18.5 tiles of 128 points, 300 x 24 = 56.25), forced persistent grids of 3 / 2 workgroups (every workgroup
    walks many tiles and draws them from the counter), and 1,024 tiles on the default grid; main and solar-correction pass"""
    from snerf_amd import ops, _lib
    dev = _dev()
    monkeypatch.setattr(ops, "BASE_FLAGS", _lib.FLAG_F16X1)
    cfg = O.OracleCfg(n_samples=n_samples)              # W = 512, 8 layers, skip at 4, SIREN
    gp = _gpu_params(O.init_params_numpy(cfg, 21), dev)
    b = O.batch_to_torch(O.synthetic_batch(n_rays, n_samples, seed=n_rays))
    for sc in (False, True):
        lib.snerf_test_set_kc_grid(grid)
        lib.snerf_test_set_trunk_fusion(0)
        ref = _render(cfg, gp, b, dev, sc)
        lib.snerf_test_set_trunk_fusion(1)
        got = _render(cfg, gp, b, dev, sc)
        again = _render(cfg, gp, b, dev, sc)
        assert set(got) == set(ref)
        for k in ref:
            assert torch.equal(got[k], ref[k]), (sc, k, float((got[k].float() - ref[k].float()).abs().max()))
            assert torch.equal(again[k], got[k]), (sc, k)                   # and run to run
        assert torch.isfinite(got["rgb" if not sc else "sun"]).all()


@pytest.mark.parametrize("n_rays,n_samples,grid", [(37, 64, 0), (150, 24, 3), (1024, 64, 0)])
def test_fused_trunk_training_pass_equals_layer_per_launch_bit_for_bit(n_rays, n_samples, grid, lib, monkeypatch):
    """training passes: every layer's planes, exponents and sign words of cos leave the fused launch for the backward pass -- the
    rendered tensors AND every parameter gradient (the backward consumes what the fused forward stored) equal the launch-per-layer
    path's bit for bit, main pass and solar-correction pass"""
    from snerf_amd import ops, _lib
    dev = _dev()
    monkeypatch.setattr(ops, "BASE_FLAGS", _lib.FLAG_F16X1)
    cfg = O.OracleCfg(n_samples=n_samples)
    spec = _spec(cfg)
    pn = O.init_params_numpy(cfg, 22)
    b = O.batch_to_torch(O.synthetic_batch(n_rays, n_samples, seed=n_rays + 1))
    rays, extras, u = b["rays"].to(dev), b["extras"].to(dev), b["u"].to(dev)
    zs = torch.linspace(0, 1, n_samples).to(dev)
    lib.snerf_test_set_kc_grid(grid)

    def run(on, sc):
        lib.snerf_test_set_trunk_fusion(on)
        gp = _gpu_params(pn, dev, requires_grad=True)
        t = (torch.zeros(n_rays, cfg.t_embedding_tau, device=dev) + 0.25).requires_grad_(True)
        res = ops.render_pass(spec, gp, ops.PassInputs(sun_d=extras[:, :3], rays=rays, z_steps=zs, u=u), t, None, sc_pass=sc)
        g = torch.Generator().manual_seed(5)
        loss = 0.0
        for k in sorted(res):
            if k not in ("z_vals", "semantic_label") and res[k].requires_grad:
                loss = loss + (res[k] * torch.rand(res[k].shape, generator=g).to(dev)).sum()
        loss.backward()
        return {k: v.detach() for k, v in res.items()}, {k: v.grad for k, v in gp.items()}, t.grad

    for sc in (False, True):
        r0, g0, t0 = run(0, sc)
        r1, g1, t1 = run(1, sc)
        for k in r0:
            assert torch.equal(r1[k], r0[k]), (sc, k)
        n = 0
        for k in g0:
            if g0[k] is None:
                assert g1[k] is None, k
                continue
            assert torch.equal(g1[k], g0[k]), (sc, k, float((g1[k] - g0[k]).abs().max()))
            n += 1
        assert n >= 20
        assert (t0 is None and t1 is None) or torch.equal(t0, t1)


def test_fused_trunk_is_taken_only_where_it_applies(lib, monkeypatch):
    """two planes, other widths, depths 2 and 9, a skip at the last layer, 12 frequencies (a 128-column encoding), ReLU: the plan keeps
    the launch-per-layer path -- no fused launch is made and the results do not depend on the switch"""
    from snerf_amd import ops, _lib
    dev = _dev()
    b = O.batch_to_torch(O.synthetic_batch(40, 16, seed=2))
    one = _lib.FLAG_F16X1
    for flags, cfg in ((0, O.OracleCfg(n_samples=16)), (one, O.OracleCfg(n_samples=16, fc_units=256)),
                       (one, O.OracleCfg(n_samples=16, fc_layers=2, fc_skips=())),
                       (one, O.OracleCfg(n_samples=16, fc_layers=9, fc_skips=(4,))),
                       (one, O.OracleCfg(n_samples=16, fc_layers=5, fc_skips=(4,))),
                       (one, O.OracleCfg(n_samples=16, mapping_pos_n_freq=12)),
                       (one, O.OracleCfg(n_samples=16, activation_function="relu"))):
        assert not _plan_fuses(cfg, flags == one, False)
        monkeypatch.setattr(ops, "BASE_FLAGS", flags)
        gp = _gpu_params(O.init_params_numpy(cfg, 4), dev)
        lib.snerf_test_set_trunk_fusion(0)
        ref = _render(cfg, gp, b, dev, False)
        lib.snerf_test_set_trunk_fusion(1)
        got, n_on = _trunk_launches(lib, lambda: _render(cfg, gp, b, dev, False))
        assert n_on == 0, (flags, cfg.fc_layers, cfg.fc_skips, cfg.mapping_pos_n_freq, cfg.activation_function, cfg.fc_units)
        for k in ref:
            assert torch.equal(got[k], ref[k]), k
    # and the default geometry DOES fuse (the guard above is not vacuous)
    cfg = O.OracleCfg(n_samples=16)
    monkeypatch.setattr(ops, "BASE_FLAGS", one)
    gp = _gpu_params(O.init_params_numpy(cfg, 4), dev)
    _, n_on = _trunk_launches(lib, lambda: _render(cfg, gp, b, dev, False))
    assert _plan_fuses(cfg, True, False) and n_on > 0


def _plan_fuses(cfg, one_plane, train):
    """where csrc/api.hip (make_plan) sends the trunk to the fused kernel, restated: one plane, SIREN, W = 512, an encoding of at most
    64 columns (and at least one frequency: raw xyz is refused in one-plane mode), 3 <= L <= 8, skips in 1 ... L - 2 -- and not a
    pass whose final layer would request the next tile's encoding (the last layer reading it, at least 2, clamped to L - 1: only
    L = 3, and only without the feats layer behind the trunk, i.e. in training passes)"""
    L, skips = cfg.fc_layers, tuple(cfg.fc_skips)
    F = cfg.mapping_pos_n_freq if cfg.model == "semantic" else 0
    E = 6 * F
    gamma_free = min(max([2] + [s for s in skips if s >= 2]), L - 1)
    feats_fused = not train
    return (one_plane and cfg.siren and cfg.fc_units == 512 and 0 < E <= 64 and 3 <= L <= 8 and all(1 <= s <= L - 2 for s in skips)
            and not (not feats_fused and gamma_free == L - 1))


def _trunk_launches(lib, fn):
    """fn()'s result and how many fused trunk launches (SnerfProfile variant 1) it made"""
    from snerf_amd import _lib
    _lib.check(lib.snerf_profile_begin(), "snerf_profile_begin")
    try:
        out = fn()
    finally:
        prof = _lib.SnerfProfile()
        _lib.check(lib.snerf_profile_end(C.byref(prof)), "snerf_profile_end")
    return out, int(prof.launches[1])


def _geom_cfg(geom, n_samples):
    L, skips, F = geom
    return O.OracleCfg(n_samples=n_samples, fc_layers=L, fc_skips=skips, mapping_pos_n_freq=F)


GEOMS = [(3, (), 10), (3, (1,), 10), (4, (), 10), (4, (2,), 10), (5, (1, 3), 10), (6, (4,), 10), (8, (2, 4, 6), 10), (8, (4,), 6)]
GEOM_IDS = [f"L{g[0]}-skips{'_'.join(map(str, g[1])) or 'none'}-F{g[2]}" for g in GEOMS]
# 67 x 64 = 4,288 points = 33.5 tiles: one workgroup walks all 34, each of three about 11 (>= 8); the last tile is ragged
GEOM_RAYS, GEOM_SAMPLES = 67, 64


@pytest.mark.parametrize("grid", [1, 3])
@pytest.mark.parametrize("geom", GEOMS, ids=GEOM_IDS)
def test_fused_trunk_geometries_inference_bit_for_bit(geom, grid, lib, monkeypatch):
    """inference passes (the feats layer rides behind the last SIREN layer) at every depth / skip set / encoding the plan fuses: fused
    equals launch-per-layer bit for bit, main and solar-correction pass, twice"""
    from snerf_amd import ops, _lib
    dev = _dev()
    monkeypatch.setattr(ops, "BASE_FLAGS", _lib.FLAG_F16X1)
    cfg = _geom_cfg(geom, GEOM_SAMPLES)
    assert _plan_fuses(cfg, True, False)
    gp = _gpu_params(O.init_params_numpy(cfg, 41), dev)
    b = O.batch_to_torch(O.synthetic_batch(GEOM_RAYS, GEOM_SAMPLES, seed=42))
    lib.snerf_test_set_kc_grid(grid)
    lib.snerf_test_set_trunk_fusion(1)
    for sc in (False, True):
        lib.snerf_test_set_trunk_fusion(0)
        ref, n_off = _trunk_launches(lib, lambda: _render(cfg, gp, b, dev, sc))
        lib.snerf_test_set_trunk_fusion(1)
        got, n_on = _trunk_launches(lib, lambda: _render(cfg, gp, b, dev, sc))
        again = _render(cfg, gp, b, dev, sc)
        assert set(got) == set(ref)
        for k in ref:
            assert torch.equal(got[k], ref[k]), (sc, k, float((got[k].float() - ref[k].float()).abs().max()))
            assert torch.equal(again[k], got[k]), (sc, k)
        assert torch.isfinite(got["rgb" if not sc else "sun"]).all()
        assert n_off == 0 and n_on > 0, (sc, n_off, n_on)


@pytest.mark.parametrize("grid", [1, 3])
@pytest.mark.parametrize("geom", GEOMS, ids=GEOM_IDS)
def test_fused_trunk_geometries_training_bit_for_bit(geom, grid, lib, monkeypatch):
    """training passes at the same geometries: rendered tensors and every parameter gradient of the fused pass equal the
    launch-per-layer pass's bit for bit, twice.  L = 3 training is NOT fused (its final layer would request the next tile's encoding
    behind a barrier that does not wait for it): the guard pins that."""
    from snerf_amd import ops, _lib
    dev = _dev()
    monkeypatch.setattr(ops, "BASE_FLAGS", _lib.FLAG_F16X1)
    cfg = _geom_cfg(geom, GEOM_SAMPLES)
    spec = _spec(cfg)
    pn = O.init_params_numpy(cfg, 43)
    b = O.batch_to_torch(O.synthetic_batch(GEOM_RAYS, GEOM_SAMPLES, seed=44))
    rays, extras, u = b["rays"].to(dev), b["extras"].to(dev), b["u"].to(dev)
    zs = torch.linspace(0, 1, GEOM_SAMPLES).to(dev)
    lib.snerf_test_set_kc_grid(grid)

    def run(on, sc):
        lib.snerf_test_set_trunk_fusion(on)
        gp = _gpu_params(pn, dev, requires_grad=True)
        t = (torch.zeros(GEOM_RAYS, cfg.t_embedding_tau, device=dev) + 0.25).requires_grad_(True)
        res = ops.render_pass(spec, gp, ops.PassInputs(sun_d=extras[:, :3], rays=rays, z_steps=zs, u=u), t, None, sc_pass=sc)
        g = torch.Generator().manual_seed(5)
        loss = 0.0
        for k in sorted(res):
            if k not in ("z_vals", "semantic_label") and res[k].requires_grad:
                loss = loss + (res[k] * torch.rand(res[k].shape, generator=g).to(dev)).sum()
        loss.backward()
        return {k: v.detach() for k, v in res.items()}, {k: v.grad for k, v in gp.items()}, t.grad

    fuses = _plan_fuses(cfg, True, True)
    for sc in (False, True):
        (r0, g0, t0), n_off = _trunk_launches(lib, lambda: run(0, sc))
        (r1, g1, t1), n_on = _trunk_launches(lib, lambda: run(1, sc))
        r2, g2, t2 = run(1, sc)
        for k in r0:
            assert torch.equal(r1[k], r0[k]), (sc, k, float((r1[k].float() - r0[k].float()).abs().max()))
            assert torch.equal(r2[k], r1[k]), (sc, k)
        n = 0
        for k in g0:
            if g0[k] is None:
                assert g1[k] is None and g2[k] is None, k
                continue
            assert torch.equal(g1[k], g0[k]), (sc, k, float((g1[k] - g0[k]).abs().max()))
            assert torch.equal(g2[k], g1[k]), (sc, k)
            n += 1
        assert n >= 20
        assert (t0 is None and t1 is None) or torch.equal(t0, t1)
        assert n_off == 0 and (n_on > 0) == fuses, (sc, fuses, n_off, n_on)
