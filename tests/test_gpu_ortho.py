"""The ortho products on the device (csrc/ortho.hip, eval/utils/ortho.py, eval/ortho.py) against the numpy restatement
(tests/ortho_numpy.py), bit for bit: the spec is integer arithmetic, so no comparison here carries a tolerance.  Run with -m gpu
on an MI355X."""
import os

import numpy as np
import pytest
import torch

from tests import ortho_numpy as R
from tests.test_gpu_fill import FILLS, _filled, _is_fill, run_filled

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _u64(t):
    return t.detach().cpu().numpy().reshape(-1).view(np.uint64)


def _struct(g):
    from snerf_amd import _lib
    return _lib.SnerfDsmGrid(**g)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def hip_top(xyz, g, radius, index0=0, top=None, stats=None):
    from snerf_amd.eval.utils import ortho as OR
    return OR.top_surface(_t(np.asarray(xyz, np.float64).reshape(-1, 3)), _struct(g), radius, index0, top, stats)


def hip_votes(xyz, labels, g, n_classes, radius, votes=None, stats=None):
    from snerf_amd.eval.utils import ortho as OR
    return OR.label_votes(_t(np.asarray(xyz, np.float64).reshape(-1, 3)), _t(np.asarray(labels, np.int64)), _struct(g), n_classes,
                          radius, votes, stats)


# ---- hand-made clouds on a 5 x 4 lattice -----------------------------------------------------------------------------------
X0, Y1, RES = 10.0, 22.0, 0.5          # west edge, north edge: cell (i, j) covers x in [10 + i/2, 10.5 + i/2), y in (22 - (j+1)/2, 22 - j/2]
HAND = np.array([
    [10.6, 21.4, 7.0], [10.7, 21.3, 7.0],                    # 0, 1: the same altitude in cell (1, 1): 0 wins
    [11.1, 21.4, 3.0], [11.2, 21.4, 3.0 + 0.3 * R.Q],        # 2, 3: less than q/2 apart, equal once quantised, in (2, 1): 2 wins
    [11.6, 21.4, 3.0], [11.7, 21.4, 3.0 + R.Q],              # 4, 5: q apart in (3, 1): 5 wins
    [11.0, 21.0, 1.0],                                       # 6: x and y exactly on a cell edge: cell (2, 2)
    [10.1, 20.1, -5.25], [10.2, 20.2, -5.5],                 # 7, 8: negative altitudes in (0, 3): 7 wins
    [9.9, 21.9, 2.0],                                        # 9: own cell (-1, 0) is outside; radius 1 reaches (0, 0) and (0, 1)
    [12.6, 20.6, 50.0],                                      # 10: own cell (5, 2) is outside; radius 1 reaches column 4
    [10.6, 21.9, np.nan], [10.6, 21.9, np.inf], [10.6, 21.9, -np.inf], [10.6, 21.9, 4.0e4], [10.6, 21.9, -4.0e4],   # 11..15: stats[0]
    [np.nan, 21.9, 1.0], [10.6, np.inf, 1.0],                # 16, 17: no cell
    [100.0, 21.9, 9.0],                                      # 18: far outside
    [10.6, 21.9, 32767.9], [10.6, 21.9, -32768.0],           # 19, 20: the ends of the key's range, both in (1, 0): 19 wins
])
WINDOWS = {"whole": (0, 0, 5, 4), "window": (1, 1, 3, 2), "beyond": (-1, 2, 4, 5)}


@pytest.mark.parametrize("radius", (0, 1, 2))
@pytest.mark.parametrize("window", WINDOWS)
def test_hand_made_clouds(window, radius):
    g = R.grid(X0, Y1, RES, 5, 4, *WINDOWS[window])
    want, wstats = R.top_loop(HAND, g, radius, index0=3)
    top, stats = hip_top(HAND, g, radius, index0=3)
    got, gstats = _u64(top), _u64(stats)
    print(window, radius, "stats", gstats.tolist(), "winners", [R.decode(k) for k in got])
    assert np.array_equal(gstats, wstats) and int(gstats[0]) == 5
    assert np.array_equal(got, want)
    assert np.array_equal(got, R.top_at(HAND, g, radius, index0=3)[0])
    if window == "whole" and radius == 0:
        win = {c: R.decode(k) for c, k in enumerate(got)}
        assert win[1 * 5 + 1] == (round(7.0 / R.Q), 3 + 0)
        assert win[1 * 5 + 2] == (round(3.0 / R.Q), 3 + 2)
        assert win[1 * 5 + 3] == (round(3.0 / R.Q) + 1, 3 + 5)
        assert win[2 * 5 + 2] == (round(1.0 / R.Q), 3 + 6)
        assert win[3 * 5 + 0] == (round(-5.25 / R.Q), 3 + 7)
        assert win[0 * 5 + 1] == (round(32767.9 / R.Q), 3 + 19)
        assert win[0] is None and int(gstats[1]) == 11
    if window == "whole" and radius == 1:
        assert R.decode(got[0])[1] == 3 + 19 and R.decode(got[2 * 5 + 4])[1] == 3 + 10      # reached from outside the lattice
    if window == "window":
        assert got.size == 6
    # the gather of the same words: altitude and index of every cell
    from snerf_amd.eval.utils import ortho as OR
    out = OR.gather(top, 3, len(HAND))
    ref = R.gather(want, 3, len(HAND))
    assert _same_bits(out["alt"].cpu().numpy().reshape(-1), ref["alt"]) and _same_bits(out["index"].cpu().numpy().reshape(-1), ref["index"])


# ---- contention ----------------------------------------------------------------------------------------------------------------
def _cloud(n, w, h, seed, n_labels=5):
    rng = np.random.default_rng(seed)
    xyz = np.stack([X0 + rng.uniform(-1.0, w * RES + 1.0, n), Y1 - rng.uniform(-1.0, h * RES + 1.0, n),
                    np.round(rng.normal(20.0, 4.0, n), 1)], 1)           # altitudes on a 0.1 m raster: equal keys' altitudes abound
    return xyz, rng.integers(-1, n_labels + 1, n)


@pytest.mark.parametrize("radius", (0, 1, 2))
@pytest.mark.parametrize("case", ("spread", "one-cell"))
def test_contention(case, radius):
    if case == "spread":
        w, h = 37, 29
        xyz, lab = _cloud(5000, w, h, 11)
    else:
        w, h = 7, 7                                                        # every point in cell (3, 3)
        rng = np.random.default_rng(12)
        xyz = np.stack([X0 + 1.5 + rng.uniform(0.0, 0.49, 3000), Y1 - 1.5 - rng.uniform(0.01, 0.49, 3000),
                        np.round(rng.normal(20.0, 0.3, 3000), 1)], 1)
        lab = rng.integers(0, 5, 3000)
    g = R.grid(X0, Y1, RES, w, h)
    top, stats = hip_top(xyz, g, radius, index0=17)
    want, wstats = R.top_at(xyz, g, radius, index0=17)
    assert np.array_equal(_u64(top), want) and np.array_equal(_u64(stats), wstats)
    votes, vstats = hip_votes(xyz, lab, g, 5, radius)
    wv, wvs = R.votes_at(xyz, lab, g, 5, radius)
    assert np.array_equal(votes.cpu().numpy().view(np.uint32).reshape(5, -1), wv) and np.array_equal(_u64(vstats), wvs)
    if case == "one-cell":
        assert (want != 0).sum() == (2 * radius + 1) ** 2 and int(wv.max()) > 500


# ---- commutativity -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", (0, 1))
def test_chunking_and_call_order_do_not_change_a_word(radius):
    w, h = 37, 29
    xyz, lab = _cloud(5000, w, h, 21)
    g = R.grid(X0, Y1, RES, w, h)
    dx, dl, gs = _t(xyz), _t(lab.astype(np.int64)), _struct(g)
    from snerf_amd.eval.utils import ortho as OR
    top0, ts0 = OR.top_surface(dx, gs, radius, 5)
    votes0, vs0 = OR.label_votes(dx, dl, gs, 5, radius)
    assert np.array_equal(_u64(top0), R.top_at(xyz, g, radius, index0=5)[0])
    for chunk in (1, 7, 1000):
        for order in (1, -1):
            top = ts = votes = vs = None
            for lo in list(range(0, 5000, chunk))[::order]:
                top, ts = OR.top_surface(dx[lo:lo + chunk], gs, radius, 5 + lo, top, ts)
                votes, vs = OR.label_votes(dx[lo:lo + chunk], dl[lo:lo + chunk], gs, 5, radius, votes, vs)
            assert torch.equal(top, top0) and torch.equal(ts, ts0), (chunk, order)
            assert torch.equal(votes, votes0) and torch.equal(vs, vs0), (chunk, order)


# ---- gather --------------------------------------------------------------------------------------------------------------------
def _three_images(seed=31):
    rng = np.random.default_rng(seed)
    w, h = 9, 7
    g = R.grid(X0, Y1, RES, w, h)
    images, index0 = [], 0
    for n in (40, 55, 23):
        xyz, _ = _cloud(n, w, h, seed + n)
        xyz[:, 2] = np.round(rng.normal(20.0, 1.0, n), 0)                  # few distinct altitudes: the index decides often
        lab = rng.choice(np.array([0, 1, 4, 254, 255, 300, -1], np.int64), n)
        images.append(dict(xyz=xyz, index0=index0, n=n, rgb=rng.random((n, 3), np.float32), labels=lab,
                           scalar=rng.normal(0.0, 1.0, n).astype(np.float32)))
        index0 += n
    return g, images


def test_gather_takes_every_cell_from_the_image_that_won_it():
    from snerf_amd.eval.utils import ortho as OR
    g, images = _three_images()
    top = ts = want = ws = None
    for im in images[::-1]:
        top, ts = hip_top(im["xyz"], g, 0, im["index0"], top, ts)
        want, ws = R.top_at(im["xyz"], g, 0, im["index0"], top=want, stats=ws)
    assert np.array_equal(_u64(top), want)
    owner = np.array([-1 if R.decode(k) is None else sum(R.decode(k)[1] >= im["index0"] for im in images) - 1 for k in want])
    assert set(owner.tolist()) == {-1, 0, 1, 2}                            # empty cells, and every image owns some
    out = ref = None
    for k, im in enumerate(images):
        out = OR.gather(top, im["index0"], im["n"], rgb=_t(im["rgb"]), labels=_t(im["labels"]), scalar=_t(im["scalar"]), out=out)
        ref = R.gather(want, im["index0"], im["n"], rgb=im["rgb"], labels=im["labels"], scalar=im["scalar"], out=ref)
        got = {key: v.cpu().numpy().reshape(ref[key].shape) for key, v in out.items()}
        for key in ("alt", "index", "rgb", "label", "scalar"):
            assert _same_bits(got[key], ref[key]), (k, key)
        later = owner > k                                                   # cells of images not gathered yet: still the pre-fill
        assert np.isnan(got["scalar"][later]).all() and (got["label"][later] == 255).all() and np.isnan(got["rgb"][:, later]).all()
    assert np.isnan(got["alt"][owner < 0]).all() and (got["index"][owner < 0] == -1).all() and np.isnan(got["scalar"][owner < 0]).all()
    seen = set(got["label"][owner >= 0].tolist())
    assert {0, 254, 255} <= seen and seen <= {0, 1, 4, 254, 255}            # 255, 300 and -1 are written as 255
    # NULL payload pairs: each pair alone, and none, give the same planes
    im = images[1]
    for keys in ((), ("rgb",), ("labels",), ("scalar",), ("rgb", "scalar")):
        o = OR.gather(top, im["index0"], im["n"], **{key: _t(im[key]) for key in keys})
        r = R.gather(want, im["index0"], im["n"], **{key: im[key] for key in keys})
        assert set(o) == set(r) == {"alt", "index"} | {"label" if key == "labels" else key for key in keys}
        for key in r:
            assert _same_bits(o[key].cpu().numpy().reshape(r[key].shape), r[key]), (keys, key)


# ---- votes ---------------------------------------------------------------------------------------------------------------------
def _centre(i, j):
    return [X0 + (i + 0.5) * RES, Y1 - (j + 0.5) * RES, 0.0]


@pytest.mark.parametrize("n_classes", (1, 5, 255))
def test_votes_and_their_finish(n_classes):
    from snerf_amd.eval.utils import ortho as OR
    w, h = 5, 4
    g = R.grid(X0, Y1, RES, w, h)
    xyz, lab = _cloud(400, w, h, 41, n_labels=n_classes)                    # labels -1 .. n_classes: both ends are out of range
    hi = n_classes - 1
    ties = [(_centre(0, 0), l) for l in (hi, 0)] + [(_centre(1, 0), l) for l in (hi, hi // 2, 0, hi, hi // 2, 0)]
    if n_classes >= 5:
        ties += [(_centre(2, 0), l) for l in (4, 2, 3, 3, 2, 4, 1)]         # three-way tie of 2, 3, 4 over a single vote for 1
    keep = ~((xyz[:, 1] > Y1 - RES) & (xyz[:, 0] < X0 + 3 * RES))           # the random points stay out of the tie cells ...
    keep &= ~((xyz[:, 0] >= X0 + 4 * RES) & (xyz[:, 0] < X0 + 5 * RES))     # ... and out of column 4: empty cells
    xyz = np.concatenate([xyz[keep], np.array([p for p, _ in ties])])
    lab = np.concatenate([lab[keep], np.array([l for _, l in ties], np.int64)])
    xyz[3, 0] = np.nan                                                      # counted in stats[0], like the labels out of range
    votes, vstats = hip_votes(xyz, lab, g, n_classes, 0)
    wv, wvs = R.votes_at(xyz, lab, g, n_classes, 0)
    assert np.array_equal(votes.cpu().numpy().view(np.uint32).reshape(n_classes, -1), wv)
    assert np.array_equal(wv, R.votes_loop(xyz, lab, g, n_classes, 0)[0])
    bad = (lab < 0) | (lab >= n_classes) | ~np.isfinite(xyz[:, 0]) | ~np.isfinite(xyz[:, 1])
    assert int(wvs[0]) == bad.sum() >= 1 + (n_classes < 255) and np.array_equal(_u64(vstats), wvs)
    label, share, stats = OR.finish_votes(votes, h, w, vstats)
    wl, wsh, wst = R.votes_finish(wv, wvs)
    label, share = label.cpu().numpy().reshape(-1), share.cpu().numpy().reshape(-1)
    print(n_classes, "labels", label.tolist(), "share", share.tolist(), "stats", _u64(stats).tolist())
    assert _same_bits(label, wl) and _same_bits(share, wsh) and np.array_equal(_u64(stats), wst)
    tot = wv.astype(np.int64).sum(0)
    assert (tot[4::5] == 0).all() and (label[4::5] == 255).all() and np.isnan(share[4::5]).all()      # empty cells
    assert label[0] == 0 and label[1] == 0                                  # the lowest class of a tie
    assert share[0] == np.float32(1.0 if n_classes == 1 else 0.5)          # a two-way tie of the highest class and class 0
    assert share[1] == np.float32(np.float64(6.0 if n_classes == 1 else 2.0) / np.float64(6.0))      # a three-way tie
    if n_classes >= 5:
        assert label[2] == 2 and share[2] == np.float32(np.float64(2.0) / np.float64(7.0))
    fin = ~np.isnan(wsh)
    assert np.array_equal(share[fin], (wv.max(0)[fin].astype(np.float64) / tot[fin].astype(np.float64)).astype(np.float32))
    assert int(_u64(stats)[1]) == tot.max()


# ---- fill independence ---------------------------------------------------------------------------------------------------------
def test_outputs_do_not_depend_on_the_bytes_under_them():
    """the method of tests/test_gpu_fill.py on the two entries with pure outputs.  snerf_ortho_gather: alt_out, idx_out "out";
    rgb_out, label_out, scalar_out "out" in the cells a point of the call won, untouched elsewhere; top and the payloads "in".
    snerf_ortho_votes_finish: label_out, share_out "out", votes "in", stats "acc" (the caller's).  snerf_ortho_top / _votes have
    accumulators only ("acc": zeroed by the caller, never filled)."""
    from snerf_amd import _lib
    from snerf_amd.eval.utils import ortho as OR
    g, images = _three_images(51)
    top = ts = None
    for im in images:
        top, ts = hip_top(im["xyz"], g, 0, im["index0"], top, ts)
    want = _u64(top)
    cells = want.size
    im = images[1]
    owned_np = np.array([R.decode(k) is not None and im["index0"] <= R.decode(k)[1] < im["index0"] + im["n"] for k in want])
    assert owned_np.any() and not owned_np.all()
    owned = _t(owned_np)
    rgb, labels, scalar = _t(im["rgb"]), _t(im["labels"]), _t(im["scalar"])
    xyz, lab = _cloud(300, 9, 7, 52)
    votes, vstats = hip_votes(xyz, lab, g, 5, 1)

    def run(fill):
        o = {"alt": _filled((cells,), torch.float32, fill), "index": _filled((cells,), torch.int64, fill),
             "rgb": _filled((3, cells), torch.float32, fill), "label": _filled((cells,), torch.uint8, fill),
             "scalar": _filled((cells,), torch.float32, fill), "vlabel": _filled((cells,), torch.uint8, fill),
             "share": _filled((cells,), torch.float32, fill), "vstats": vstats.clone()}
        _lib.call("snerf_ortho_gather", top, cells, im["index0"], im["n"], OR.Z0, OR.Q, rgb, labels, scalar, o["alt"], o["index"],
                  o["rgb"], o["label"], o["scalar"])
        _lib.call("snerf_ortho_votes_finish", votes, 5, cells, o["vlabel"], o["share"], o["vstats"])
        for key in ("rgb", "label", "scalar"):           # cells no winner of the call owns keep the fill ...
            t = o[key]
            assert _is_fill(t[..., ~owned], fill), key
            o[key] = t[..., owned].contiguous()          # ... and the owned ones must not depend on it
        return o

    r = run_filled(run)[0xFF]
    ref = R.gather(want, im["index0"], im["n"], rgb=im["rgb"], labels=im["labels"], scalar=im["scalar"])
    assert _same_bits(r["alt"].cpu().numpy(), ref["alt"]) and _same_bits(r["index"].cpu().numpy(), ref["index"])
    assert _same_bits(r["rgb"].cpu().numpy(), ref["rgb"][:, owned_np]) and _same_bits(r["label"].cpu().numpy(), ref["label"][owned_np])
    assert _same_bits(r["scalar"].cpu().numpy(), ref["scalar"][owned_np])
    wl, wsh, wst = R.votes_finish(R.votes_at(xyz, lab, g, 5, 1)[0], _u64(vstats))
    assert _same_bits(r["vlabel"].cpu().numpy(), wl) and _same_bits(r["share"].cpu().numpy(), wsh) and np.array_equal(_u64(r["vstats"]), wst)
    assert FILLS == (0x00, 0xFF, 0x7B)


def test_zero_points_change_nothing():
    from snerf_amd import _lib
    from snerf_amd.eval.utils import ortho as OR
    g = R.grid(X0, Y1, RES, 5, 4)
    gs = _struct(g)
    top, ts = hip_top(HAND, g, 1)
    votes, vs = hip_votes(HAND, np.arange(len(HAND)) % 3, g, 3, 1)
    before = [t.clone() for t in (top, ts, votes, vs)]
    empty = torch.empty((0, 3), dtype=torch.float64, device=DEV)
    OR.top_surface(empty, gs, 1, 7, top, ts)
    OR.label_votes(empty, torch.empty(0, dtype=torch.int64, device=DEV), gs, 3, 1, votes, vs)
    _lib.call("snerf_ortho_top", None, 0, 0, gs, 0, OR.Z0, OR.Q, top, ts)
    _lib.call("snerf_ortho_votes", None, None, 0, gs, 0, 3, votes, vs)
    alt, idx = _filled((20,), torch.float32, 0x7B), _filled((20,), torch.int64, 0x7B)
    _lib.call("snerf_ortho_gather", top, 20, 4, 0, OR.Z0, OR.Q, None, None, None, alt, idx, None, None, None)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, (top, ts, votes, vs)))
    assert _is_fill(alt, 0x7B) and _is_fill(idx, 0x7B)
    t2, s2 = OR.top_surface(empty, gs, 0)                      # fresh accumulators stay zero
    assert not bool(t2.any()) and not bool(s2.any())


SEED = 1234


# ---- end to end on the fixture scene ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    from snerf_amd.framework.pipelines import load_pipeline
    from tests.test_gpu_scene import _pipeline_cfgs
    torch.manual_seed(0)                                       # a seeded, untrained semantic model
    c = _pipeline_cfgs(False, tmp_path_factory.mktemp("cache"))
    pipe = load_pipeline(c).to(torch.device(DEV))
    bank = pipe.datasets["rgb_test"]
    return c, pipe, bank.scene_images(), bank.dataset.geo


def _restated_products(c, pipe, images, geo, radius, dsm_radius):
    """the spec on the host, fed with the same lean_inference outputs and geo.cloud clouds"""
    from snerf_amd.eval.utils import dsm as D
    from snerf_amd.eval.utils.util import lean_inference
    from tests import dsm_numpy as N
    frames, index0 = [], 0
    torch.manual_seed(SEED)                                    # the renderer jitters the depths: the same draws as the walk under test
    for im in images:
        res = lean_inference(c, pipe.renderer, pipe.models, im["rays"], im["extras"],
                             keys=("rgb_coarse", "depth_coarse", "semantic_label_coarse"))
        cloud, _ = geo.cloud(im["rays"], res["depth_coarse"])
        frames.append(dict(cloud=cloud, xyz=cloud.cpu().numpy(), rgb=res["rgb_coarse"].cpu().numpy(),
                           labels=res["semantic_label_coarse"].cpu().numpy(), index0=index0, n=cloud.shape[0]))
        index0 += cloud.shape[0]
    cat = np.concatenate([f["xyz"] for f in frames])
    grid = D.DsmGrid(*N.bounds_grid(cat, D.RESOLUTION))
    g = R.grid(grid.xoff, grid.yoff, grid.resolution, grid.xsize, grid.ysize)
    top = votes = None
    for f in frames:
        top, _ = R.top_at(f["xyz"], g, radius, f["index0"], top=top)
        votes, vstats = R.votes_at(f["xyz"], f["labels"], g, 5, radius, votes=votes)
    out = None
    for f in frames:
        out = R.gather(top, f["index0"], f["n"], rgb=f["rgb"], labels=f["labels"], out=out)
    out["label_vote"], out["vote_share"], _ = R.votes_finish(votes)
    out["dsm"] = D.create_dsm(torch.cat([f["cloud"] for f in frames]), radius=dsm_radius)
    return grid, out, index0


def _assert_products(prod, grid, ref, n_points):
    h, w = grid.ysize, grid.xsize
    assert tuple(prod["grid"]) == tuple(grid) and prod["n_points"] == n_points and prod["bad_points"] == 0 and prod["bad_labels"] == 0
    for key, rkey in (("top_alt", "alt"), ("top_index", "index"), ("rgb", "rgb"), ("label_top", "label"), ("label_vote", "label_vote"),
                      ("vote_share", "vote_share")):
        want = ref[rkey].reshape((3, h, w) if key == "rgb" else (h, w))
        assert _same_bits(prod[key].cpu().numpy(), want), key
    assert torch.equal(prod["dsm"].view(torch.int32), ref["dsm"].view(torch.int32))
    assert (prod["top_index"] >= 0).any() and (prod["top_index"] < 0).any()


@pytest.mark.parametrize("radius,dsm_radius", [(0, 1), (1, 1)])
def test_products_of_the_fixture_scene_equal_the_restatement(scene, radius, dsm_radius):
    from snerf_amd.eval.utils.ortho import ortho_products
    c, pipe, images, geo = scene
    todo = images[1:]
    grid, ref, n_points = _restated_products(c, pipe, todo, geo, radius, dsm_radius)
    torch.manual_seed(SEED)
    prod = ortho_products(c, pipe.renderer, pipe.models, todo, geo=geo, radius=radius, dsm_radius=dsm_radius)
    print("grid", tuple(grid), "points", n_points, "max votes", prod["max_votes"], "filled cells", int((prod["top_index"] >= 0).sum()))
    _assert_products(prod, grid, ref, n_points)
    # the grid given instead of found: the same map, with one walk over the images
    torch.manual_seed(SEED)
    again = ortho_products(c, pipe.renderer, pipe.models, todo, geo=geo, radius=radius, dsm_radius=dsm_radius, grid=grid)
    _assert_products(again, grid, ref, n_points)


def test_export_writes_every_product_and_sharded_gives_the_same_bits(scene, tmp_path):
    from PIL import Image
    from snerf_amd.eval.ortho import export_ortho
    from snerf_amd.framework.util import img_utils as I
    c, pipe, images, geo = scene
    grid, ref, n_points = _restated_products(c, pipe, images[1:], geo, 0, 1)
    torch.manual_seed(SEED)
    prod = export_ortho(c, pipe.renderer, pipe.models, images, str(tmp_path), geo=geo)       # split "test": image 0 is skipped
    _assert_products(prod, grid, ref, n_points)
    names = {k + e for k in ("rgb", "label_top", "label_vote", "top_alt", "dsm", "vote_share") for e in (".png", ".tif")}
    assert set(prod["files"]) == names == set(os.listdir(tmp_path / "ortho" / "test"))
    gt = (grid.xoff, grid.yoff, grid.resolution, grid.resolution)
    for key in ("dsm", "top_alt", "vote_share"):
        a, tf = I.load_dsm_geotiff(prod["files"][key + ".tif"])
        assert a.dtype == np.float32 and tf == gt and _same_bits(a, prod[key].cpu().numpy()), key
    for key in ("label_top", "label_vote"):
        a, tf = I.load_dsm_geotiff(prod["files"][key + ".tif"])
        assert a.dtype == np.uint8 and tf == gt and np.array_equal(a, prod[key].cpu().numpy()), key
    with Image.open(prod["files"]["rgb.tif"]) as im:
        rgb8 = np.array(im)
        assert im.mode == "RGB" and tuple(im.tag_v2[I.TAG_GEO_KEY_DIRECTORY])[-1] == 32617           # the scene's zone, 17R
    want8 = torch.nan_to_num(prod["rgb"], nan=0.0).mul(255).add(0.5).clamp(0, 255).to(torch.uint8).permute(1, 2, 0).cpu().numpy()
    assert np.array_equal(rgb8, want8)
    for name in names:
        if name.endswith(".png"):
            with Image.open(prod["files"][name]) as im:
                assert im.size == (grid.xsize, grid.ysize) and im.mode == "RGB", name
    with Image.open(prod["files"]["label_top.png"]) as im:
        px = np.array(im)
    assert (px[prod["label_top"].cpu().numpy() == 255] == 0).all()                                # no data is black
    torch.manual_seed(SEED)
    sharded = export_ortho(c, pipe.renderer, pipe.models, images, str(tmp_path / "sharded"), geo=geo, sharded=True)
    _assert_products(sharded, grid, ref, n_points)
