"""CPU-side checks of the ortho products (the ortho section of include/snerf_hip.h, csrc/ortho.hip, eval/utils/ortho.py,
img_utils.save_geotiff): the constants of the header against their mirrors (tests/test_abi_cpu.py holds the binding rows to the
prototypes), every refusal without a GPU, the key's layout, the two forms of the numpy restatement against each other, and the
GeoTIFF writer's round trip."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import ortho_numpy as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "snerf_hip.h")


def test_ortho_constants_match_the_header_and_the_library():
    from snerf_amd import _lib
    L = _lib.lib()
    assert L.snerf_version() == _lib.ABI_VERSION == 6
    assert not hasattr(L, "snerf_ortho_version")                # the ortho entries have no version of their own any more
    text = open(HEADER).read()
    assert int(re.search(r"#define SNERF_ABI_VERSION (\d+)", text).group(1)) == _lib.ABI_VERSION
    assert int(re.search(r"#define SNERF_ORTHO_MAX_RADIUS (\d+)", text).group(1)) == _lib.ORTHO_MAX_RADIUS == 7
    assert int(re.search(r"#define SNERF_ORTHO_MAX_CLASSES (\d+)", text).group(1)) == _lib.ORTHO_MAX_CLASSES == 255
    assert int(re.search(r"#define SNERF_ORTHO_NO_LABEL (\d+)", text).group(1)) == _lib.ORTHO_NO_LABEL == R.NO_LABEL
    from snerf_amd.eval.utils import ortho as OR
    assert OR.Z0 == R.Z0 == 0.0 and OR.Q == R.Q == 2.0 ** -16


def _grid(**kw):
    from snerf_amd import _lib
    f = dict(xoff=0.0, yoff=2.0, res=0.5, xsize=5, ysize=4, ioff=0, joff=0, out_w=5, out_h=4)
    f.update(kw)
    return _lib.SnerfDsmGrid(*[f[n] for n, _ in _lib.SnerfDsmGrid._fields_])


P = C.c_void_p(256)        # a non-null address no refused call may touch
INF, NAN = float("inf"), float("nan")


def _refusals():
    g = _grid()
    top = lambda **k: ("snerf_ortho_top", [k.get("xyz", P), k.get("n", 3), k.get("index0", 0), k.get("grid", g), k.get("radius", 0),      # noqa: E731
                                           k.get("z0", 0.0), k.get("q", R.Q), k.get("top", P), k.get("stats", P), None])
    gat = lambda **k: ("snerf_ortho_gather", [k.get("top", P), k.get("cells", 20), k.get("index0", 0), k.get("n", 3), k.get("z0", 0.0),    # noqa: E731
                                              k.get("q", R.Q), k.get("rgb"), k.get("labels"), k.get("scalar"), k.get("alt_out", P),
                                              k.get("idx_out", P), k.get("rgb_out"), k.get("label_out"), k.get("scalar_out"), None])
    vot = lambda **k: ("snerf_ortho_votes", [k.get("xyz", P), k.get("labels", P), k.get("n", 3), k.get("grid", g), k.get("radius", 0),     # noqa: E731
                                             k.get("n_classes", 5), k.get("votes", P), k.get("stats", P), None])
    fin = lambda **k: ("snerf_ortho_votes_finish", [k.get("votes", P), k.get("n_classes", 5), k.get("cells", 20), k.get("label_out", P),   # noqa: E731
                                                    k.get("share_out", P), k.get("stats", P), None])
    cases = []
    for who in ("xyz", "grid", "top", "stats"):
        cases.append((top(**{who: None}), b"null pointer"))
    for who in ("top", "alt_out", "idx_out"):
        cases.append((gat(**{who: None}), b"null pointer"))
    for a, b in (("rgb", "rgb_out"), ("labels", "label_out"), ("scalar", "scalar_out")):
        cases.append((gat(**{a: P}), b"given together"))
        cases.append((gat(**{b: P}), b"given together"))
    for who in ("xyz", "labels", "grid", "votes", "stats"):
        cases.append((vot(**{who: None}), b"null pointer"))
    for who in ("votes", "label_out", "share_out", "stats"):
        cases.append((fin(**{who: None}), b"null pointer"))
    for n in (-1, 2 ** 31 + 1):
        cases += [(top(n=n), b"n must lie in [0, 2^31]"), (gat(n=n), b"n must lie in [0, 2^31]"), (vot(n=n), b"n must lie in [0, 2^31]")]
    for r in (-1, 8):
        cases += [(top(radius=r), b"radius must lie in [0, 7]"), (vot(radius=r), b"radius must lie in [0, 7]")]
    for c in (0, 256, -3):
        cases += [(vot(n_classes=c), b"n_classes must lie in [1, 255]"), (fin(n_classes=c), b"n_classes must lie in [1, 255]")]
    for kw in (dict(ioff=2 ** 31 - 5, out_w=5), dict(joff=2 ** 31 - 4, out_h=4), dict(ioff=1, out_w=2 ** 31 - 1)):
        cases += [(top(grid=_grid(**kw)), b"beyond int32"), (vot(grid=_grid(**kw)), b"beyond int32")]
    for kw in (dict(res=0.0), dict(res=NAN), dict(res=INF), dict(xoff=NAN), dict(yoff=INF), dict(xsize=0), dict(ysize=-1), dict(out_w=0),
               dict(out_h=0)):
        cases += [(top(grid=_grid(**kw)), b"grid needs"), (vot(grid=_grid(**kw)), b"grid needs")]
    for q in (0.0, -R.Q, INF, NAN):
        cases += [(top(q=q), b"q > 0 and finite"), (gat(q=q), b"q > 0 and finite")]
    for z0 in (INF, NAN):
        cases += [(top(z0=z0), b"z0 finite"), (gat(z0=z0), b"z0 finite")]
    for index0, n in ((-1, 3), (2 ** 32 - 3, 3), (2 ** 32, 0), (2 ** 31, 2 ** 31)):
        cases += [(top(index0=index0, n=n), b"index0 + n <= 2^32 - 1"), (gat(index0=index0, n=n), b"index0 + n <= 2^32 - 1")]
    for cells in (0, -7):
        cases += [(gat(cells=cells), b"cells must be >= 1"), (fin(cells=cells), b"cells must be >= 1")]
    return cases


def test_every_refusal_returns_a_code_and_a_message_without_a_gpu():
    from snerf_amd import _lib
    L = _lib.lib()
    cases = _refusals()
    assert len(cases) == 86
    for (name, args), msg in cases:
        args = [C.byref(a) if isinstance(a, C.Structure) else a for a in args]
        rc = getattr(L, name)(*args)
        err = L.snerf_last_error()
        assert rc != 0 and msg in err and name.encode() in err, (name, args, rc, err)
    # through the binding: the library's message, as the host layer's ValueError
    with pytest.raises(ValueError, match=r"snerf_ortho_top failed \(code 1\): .*radius must lie in \[0, 7\]"):
        _lib.check(L.snerf_ortho_top(P, 3, 0, C.byref(_grid()), 9, 0.0, R.Q, P, P, None), "snerf_ortho_top", ValueError)


def test_zero_points_are_legal_and_launch_nothing():
    """n = 0 returns 0 before any launch -- also with null point arrays, and on a machine without a GPU"""
    from snerf_amd import _lib
    L = _lib.lib()
    g = C.byref(_grid())
    assert L.snerf_ortho_top(None, 0, 0, g, 0, 0.0, R.Q, P, P, None) == 0
    assert L.snerf_ortho_top(None, 0, 2 ** 32 - 1, g, 7, 0.0, R.Q, P, P, None) == 0
    assert L.snerf_ortho_votes(None, None, 0, g, 0, 255, P, P, None) == 0
    assert L.snerf_ortho_gather(P, 20, 5, 0, 0.0, R.Q, None, None, None, P, P, None, None, None, None) == 0


def test_key_round_trip():
    for k in (-2 ** 31, -1, 0, 2 ** 31 - 1):
        for index in (0, 2 ** 32 - 2):
            key = R.encode(k, index)
            assert 0 < key < 2 ** 64 and R.decode(key) == (k, index)
            assert key == ((k + 2 ** 31) << 32) | (0xFFFFFFFF - index)
    assert R.decode(0) is None
    assert R.encode(-2 ** 31, 2 ** 32 - 2) == 1                      # the smallest key there is: 0 stays free for "no point"
    # order: altitude first, then the LOWER index
    assert R.encode(1, 7) > R.encode(0, 0) and R.encode(5, 3) > R.encode(5, 4) and R.encode(-1, 0) < R.encode(0, 2 ** 32 - 2)
    # ties to even, and the edges of the range
    kq, ok = R.quantise(np.array([0.5 * R.Q, 1.5 * R.Q, -0.5 * R.Q, 32768.0 - R.Q, 32768.0 - 0.4 * R.Q, -32768.0, -32768.0 - R.Q,
                                  np.nan, np.inf, -np.inf]))
    assert kq[:4].tolist() == [0.0, 2.0, -0.0, 2.0 ** 31 - 1] and ok.tolist() == [True] * 4 + [False, True] + [False] * 4


def _random_cloud(n, w, h, res, seed, pad=1.5, labels=5):
    rng = np.random.default_rng(seed)
    xyz = np.stack([rng.uniform(-pad * res, (w + pad) * res, n), rng.uniform(-pad * res, (h + pad) * res, n),
                    np.round(rng.normal(12.0, 3.0, n), 1)], 1)            # rounded altitudes: ties do occur
    lab = rng.integers(-1, labels + 1, n)
    return xyz, lab


@pytest.mark.parametrize("radius", (0, 1, 2))
@pytest.mark.parametrize("window", (None, (2, 1, 6, 5), (-2, -1, 20, 30)))
def test_loop_and_ufunc_forms_of_the_restatement_agree(radius, window):
    w, h, res = 11, 9, 0.5
    g = R.grid(100.0, 200.0 + h * res, res, w, h, *(window or (0, 0, None, None)))
    xyz, lab = _random_cloud(700, w, h, res, 3 + radius)
    xyz[:, 0] += 100.0
    xyz[:, 1] += 200.0
    xyz[5] = [np.nan, 201.0, 3.0]
    xyz[6] = [101.0, np.inf, 3.0]
    xyz[7, 2] = np.nan
    xyz[8, 2] = 4.0e4
    xyz[9, 2] = -np.inf
    xyz[10:14, :2] = [100.0 + 2 * res, 200.0 + 3 * res]       # on a cell corner
    t0, s0 = R.top_loop(xyz, g, radius, index0=40)
    t1, s1 = R.top_at(xyz, g, radius, index0=40)
    assert np.array_equal(t0, t1) and np.array_equal(s0, s1) and int(s0[0]) == 3 and 0 < int(s0[1]) < 700
    assert (t0 != 0).any()
    # chunked, in reverse order: the same words
    t2, s2 = None, None
    for lo in (400, 0):
        t2, s2 = R.top_at(xyz[lo:lo + 400 if lo == 0 else None], g, radius, index0=40 + lo, top=t2, stats=s2)
    assert np.array_equal(t2, t0) and np.array_equal(s2, s0)
    v0, vs0 = R.votes_loop(xyz, lab, g, 5, radius)
    v1, vs1 = R.votes_at(xyz, lab, g, 5, radius)
    assert np.array_equal(v0, v1) and np.array_equal(vs0, vs1) and int(vs0[0]) >= 2
    lab_, share, st = R.votes_finish(v0)
    tot = v0.sum(0)
    assert np.array_equal(lab_ == R.NO_LABEL, tot == 0) and np.array_equal(np.isnan(share), tot == 0) and int(st[1]) == tot.max()


def test_restated_gather_takes_each_cell_from_its_own_image():
    g = R.grid(0.0, 2.0, 0.5, 5, 4)
    a = np.array([[0.1, 1.9, 5.0], [0.6, 1.9, 5.0]])
    b = np.array([[0.1, 1.9, 6.0], [1.1, 1.9, 1.0]])
    top, _ = R.top_loop(a, g, 0, 0)
    top, _ = R.top_loop(b, g, 0, 2, top=top)
    out = R.gather(top, 0, 2, labels=np.array([7, 300]))
    out = R.gather(top, 2, 2, labels=np.array([-1, 254]), out=out)
    assert out["index"][:3].tolist() == [2, 1, 3] and out["index"][3] == -1
    assert out["label"][:4].tolist() == [255, 255, 254, 255] and out["alt"][:3].tolist() == [6.0, 5.0, 1.0] and np.isnan(out["alt"][3])


# ---- GeoTIFF writer ------------------------------------------------------------------------------------------------------------
def test_save_geotiff_round_trips_float32_with_nans(tmp_path):
    from snerf_amd.eval.utils.dsm import DsmGrid
    from snerf_amd.framework.util import img_utils as I
    grid = DsmGrid(435012.5, 3354988.25, 0.5, 7, 5)
    rng = np.random.default_rng(1)
    a = rng.normal(10.0, 30.0, (5, 7)).astype(np.float32)
    a[1, 2] = a[4, 6] = np.nan
    a[0, 0] = -0.0
    fp = str(tmp_path / "a.tif")
    assert I.save_geotiff(fp, a, grid, "17R") == fp
    back, gt = I.load_dsm_geotiff(fp)
    assert back.dtype == np.float32 and np.array_equal(back.view(np.uint32), a.view(np.uint32))
    assert gt == (grid.xoff, grid.yoff, grid.resolution, grid.resolution)
    from PIL import Image
    with Image.open(fp) as im:
        assert im.mode == "F" and im.tag_v2[259] == 1                   # uncompressed
        assert tuple(im.tag_v2[I.TAG_GEO_KEY_DIRECTORY]) == (1, 1, 0, 3, 1024, 0, 1, 1, 1025, 0, 1, 1, 3072, 0, 1, 32617)
    import torch
    I.save_geotiff(fp, torch.from_numpy(a), grid)                       # a tensor; no zone: no GeoKeyDirectory
    back, gt = I.load_dsm_geotiff(fp)
    assert np.array_equal(back.view(np.uint32), a.view(np.uint32)) and gt == (grid.xoff, grid.yoff, 0.5, 0.5)
    with Image.open(fp) as im:
        assert I.TAG_GEO_KEY_DIRECTORY not in im.tag_v2
    assert I.utm_epsg("17R") == 32617 and I.utm_epsg("33H") == 32733 and I.utm_epsg("1N") == 32601
    for bad in (a.astype(np.float64), a[:4], np.zeros((5, 7, 4), np.uint8)):
        with pytest.raises(ValueError, match="save_geotiff"):
            I.save_geotiff(fp, bad, grid)


def test_save_geotiff_uint8_and_rgb_reopen_with_the_three_tags(tmp_path):
    from PIL import Image
    from snerf_amd.eval.utils.dsm import DsmGrid
    from snerf_amd.framework.util import img_utils as I
    grid = DsmGrid(-1200.25, 77.5, 0.25, 6, 4)
    rng = np.random.default_rng(2)
    for name, a, mode in (("l.tif", rng.integers(0, 256, (4, 6)).astype(np.uint8), "L"),
                          ("rgb.tif", rng.integers(0, 256, (4, 6, 3)).astype(np.uint8), "RGB")):
        fp = str(tmp_path / name)
        I.save_geotiff(fp, a, grid, "56J")
        with Image.open(fp) as im:
            im.load()
            assert im.mode == mode and np.array_equal(np.array(im), a)
            assert tuple(im.tag_v2[I.TAG_MODEL_PIXEL_SCALE]) == (0.25, 0.25, 0.0)
            assert tuple(im.tag_v2[I.TAG_MODEL_TIEPOINT]) == (0.0, 0.0, 0.0, -1200.25, 77.5, 0.0)
            assert tuple(im.tag_v2[I.TAG_GEO_KEY_DIRECTORY])[-4:] == (3072, 0, 1, 32756)
    back, gt = I.load_dsm_geotiff(str(tmp_path / "l.tif"))              # the reader of the masks takes the uint8 file too
    assert back.dtype == np.uint8 and gt == (-1200.25, 77.5, 0.25, 0.25)
