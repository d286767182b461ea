"""The orthorectifier on the device (csrc/orthorect.hip, eval/utils/orthorect.py, eval/ortho.py export_rectified).

Geometry: col_row is, bit for bit, snerf_geo_points (world -> scene, lla_out) followed by snerf_rpc_project on the same cell
centres -- the same device functions without contraction -- and within 1e-6 pixel of the numpy chain (tests/orthorect_numpy.py
project_cells; the bar of tests/test_gpu_scene.py's projection check).  Everything downstream -- states, colours, labels, sums, counts,
votes, totals and the two finishes -- equals, BIT FOR BIT, the restatement's second half fed the device's own col_row and the cast's
own lit_out.  The images: the five of tests/golden/scene_small and two tiny ones (1 x 1 and 2 x 1 pixels) cut out of the first."""
import copy
import ctypes as C
import json
import math
import os
import types

import numpy as np
import pytest
import torch

from snerf_amd import _lib
from snerf_amd.baseline.components.camera_models import rpc_struct, struct_to_device
from snerf_amd.eval.utils import orthorect as R
from snerf_amd.framework.util.conversions import zone_central_meridian
from tests import orthorect_numpy as N
from tests import shadow_numpy as SN
from tests.test_gpu_geo import DSM_DIR
from tests.test_gpu_nadir import _same, scene       # noqa: F401  (the seeded, untrained semantic model on the fixture scene)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LON0 = zone_central_meridian(N.ZONE)
PAD = 64            # elements behind every device buffer, which must keep their fill
FILL = 0xA5


def _images():
    """[(rpc dict, row0, w, h)]: the fixture's five images, then a 1 x 1 and a 2 x 1 image -- pixel (20, 18) and pixels (7, 30),
    (8, 30) of the first image as images of their own, their rows of the bank addressed through row0"""
    sc = N.fixture_scene()
    out = [(m["rpc"], row0, w, h) for m, (row0, w, h) in zip(sc["metas"], sc["images"])]
    rpc, _, w0, _ = out[0]
    for (col, row, w, h) in ((20, 18, 1, 1), (7, 30, 2, 1)):
        tiny = copy.deepcopy(rpc)
        tiny["col_offset"] -= col
        tiny["row_offset"] -= row
        out.append((tiny, row * w0 + col, w, h))
    return out


IMAGES = _images()


def _filled(n, dtype, zero=False, fill=FILL):
    """n elements and PAD behind them, every byte `fill`; with `zero` the n elements are zeroed (an accumulator)"""
    t = torch.empty(n + PAD, dtype=dtype, device=DEV)
    t.view(torch.uint8).fill_(fill)
    if zero:
        t[:n].zero_()
    return t


def _tail_kept(t, n, fill=FILL):
    return bool((t[n:].view(torch.uint8) == fill).all())


def _table(images):
    table = (_lib.SnerfRectImage * len(images))()
    for k, (rpc, row0, w, h) in enumerate(images):
        table[k].rpc, table[k].row0, table[k].w, table[k].h = rpc_struct(rpc), row0, w, h
    return table


def _grid_struct(grid, lattice=None):
    xoff, yoff, res, ioff, joff, w, h = grid
    xs, ys = lattice if lattice is not None else (ioff + w, joff + h)
    return _lib.SnerfDsmGrid(xoff, yoff, res, xs, ys, ioff, joff, w, h)


class Call:
    """one snerf_orthorectify call on padded, pre-filled buffers; .np(key) gives the written part as numpy"""

    def __init__(self, grid, dsm, images, n_classes=N.N_CLASSES, labels=True, visible=None, acc=None, outputs=True, lattice=None, fill=FILL,
                 **override):
        sc = N.fixture_scene()
        self.cells, self.n, self.C, self.fill = grid[5] * grid[6], len(images), n_classes, fill
        cells, n = self.cells, self.n
        self.dsm = torch.from_numpy(np.ascontiguousarray(dsm, np.float32).reshape(-1)).to(DEV)
        self.rgbs, self.labels = torch.from_numpy(sc["rgbs"]).to(DEV), torch.from_numpy(sc["labels"]).to(DEV) if labels else None
        self.visible = torch.from_numpy(np.ascontiguousarray(visible, np.uint8).reshape(n, cells)).to(DEV) if visible is not None else None
        if acc is None:
            acc = {"sum": _filled(3 * cells, torch.int64, True, fill), "count": _filled(cells, torch.int32, True, fill),
                   "votes": _filled(n_classes * cells, torch.int32, True, fill) if labels else None,
                   "stats": _filled(4, torch.int64, True, fill)}
        self.acc = acc
        self.out = {"col_row": _filled(2 * n * cells, torch.float64, fill=fill), "rgb": _filled(3 * n * cells, torch.float32, fill=fill),
                    "label": _filled(n * cells, torch.uint8, fill=fill), "state": _filled(n * cells, torch.uint8, fill=fill)} if outputs else dict.fromkeys(
                        ("col_row", "rgb", "label", "state"))
        table = _table(images)
        self.args = dict(dsm=self.dsm, grid=_grid_struct(grid, lattice), lon0=LON0, south=0, host=table, dev=struct_to_device(table, DEV),
                         n_images=n, rgbs=self.rgbs, labels=self.labels, n_rows=sc["rgbs"].shape[0], n_classes=n_classes,
                         visible=self.visible, sum=acc["sum"], count=acc["count"], votes=acc["votes"], col_row=self.out["col_row"],
                         rgb_out=self.out["rgb"], label_out=self.out["label"], state_out=self.out["state"], stats=acc["stats"])
        self.args.update(override)

    def run(self):
        _lib.call("snerf_orthorectify", *self.args.values(), device=DEV, exc=ValueError)
        return self

    def tensor(self, key):
        """the written part of a buffer, shaped"""
        cells, n = self.cells, self.n
        if key in self.out:
            t, shape = self.out[key], {"col_row": (n, 2, cells), "rgb": (n, 3, cells), "label": (n, cells), "state": (n, cells)}[key]
        else:
            t, shape = self.acc[key], {"sum": (3, cells), "count": (cells,), "votes": (self.C, cells), "stats": (4,)}[key]
        return t[:int(np.prod(shape))].reshape(shape)

    def np(self, key):
        a = self.tensor(key).cpu().numpy()
        return a.view({"count": np.uint32, "votes": np.uint32, "stats": np.uint64}.get(key, a.dtype))

    def tails_kept(self):
        bufs = [(self.out[k], s * self.n * self.cells) for k, s in (("col_row", 2), ("rgb", 3), ("label", 1), ("state", 1)) if self.out[k] is not None]
        bufs += [(self.acc["sum"], 3 * self.cells), (self.acc["count"], self.cells), (self.acc["stats"], 4)]
        if self.acc["votes"] is not None:
            bufs.append((self.acc["votes"], self.C * self.cells))
        return all(_tail_kept(t, n, self.fill) for t, n in bufs)


def _bits(a):
    return np.ascontiguousarray(a).view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _cast(dsm, rows):
    """snerf_shadow_cast's lit_out of `dsm` under the rows, on the device: (n, cells) u8 numpy"""
    t = torch.from_numpy(np.ascontiguousarray(dsm, np.float32)).to(DEV)
    return R.visibility(t, rows).cpu().numpy().reshape(len(rows), -1)


def _rows(images, res):
    """the view rows of `images` at the first image's altitude range (the tiny images look along the first image's line of sight)"""
    m = N.fixture_scene()["metas"]
    alt = {id(mm["rpc"]): (mm["min_alt"], mm["max_alt"]) for mm in m}
    return np.stack([N.view_row(rpc, w, h, *alt.get(id(rpc), (m[0]["min_alt"], m[0]["max_alt"])), N.ZONE, res) for rpc, _, w, h in images])


def _assert_call(call, grid, dsm, images, visible, labels=True, n_classes=N.N_CLASSES):
    """everything downstream of col_row against the restatement fed the device's col_row; returns the restatement's result"""
    sc = N.fixture_scene()
    col_row = call.np("col_row")
    want = N.sample_and_fuse(col_row, dsm, [im[1:] for im in images], sc["rgbs"], sc["labels"] if labels else None, n_classes, visible)
    assert np.array_equal(call.np("state"), want["state"])
    assert np.array_equal(_bits(call.np("rgb")), _bits(want["rgb"]))
    assert np.array_equal(call.np("label"), want["label"])
    for key in ("sum", "count", "stats") + (("votes",) if labels else ()):
        assert np.array_equal(call.np(key), want["acc"][key]), key
    assert call.tails_kept()
    hole = ~np.isfinite(np.asarray(dsm, np.float32).reshape(-1))
    assert np.isnan(col_row[:, :, hole]).all() and np.isfinite(col_row[:, :, ~hole]).all()
    return want


# ---- geometry --------------------------------------------------------------------------------------------------------------------
def _device_chain(grid, dsm, rpc):
    """snerf_geo_points (direction 1, lla_out) then snerf_rpc_project on the cell centres: (2, cells) fp64"""
    from snerf_amd.baseline.components.camera_models import RPCModel
    east, north = N.cell_centres(grid)
    alt = np.asarray(dsm, np.float32).reshape(-1).astype(np.float64)
    enu = torch.from_numpy(np.stack([east, north, np.where(np.isfinite(alt), alt, 0.0)], 1)).to(DEV)
    p = _lib.SnerfGeoParams((C.c_double * 3)(0.0, 0.0, 0.0), 1.0, LON0, 0, _lib.GEO_TO_SCENE)
    xyz, lla = torch.empty_like(enu), torch.empty_like(enu)
    stats = torch.tensor([-1, 0, -1, 0, 0, 0, 0, 0], dtype=torch.int64, device=DEV)
    _lib.call("snerf_geo_points", enu, enu.shape[0], p, xyz, lla, stats)
    col, row = RPCModel(rpc, device=DEV).projection(lla[:, 1], lla[:, 0], torch.from_numpy(alt).to(DEV))
    return np.stack([col.cpu().numpy(), row.cpu().numpy()])


def test_col_row_is_the_device_chain_bit_for_bit_and_the_numpy_chain_within_1e_6_pixel():
    grid = N.fixture_lattice()
    dsm = N.block_dsm(grid, holes=True)
    ok = np.isfinite(dsm).reshape(-1)
    call = Call(grid, dsm, IMAGES).run()
    got = call.np("col_row")
    worst = 0.0
    for k, (rpc, _, w, h) in enumerate(IMAGES):
        chain = _device_chain(grid, dsm, rpc)
        assert np.array_equal(_bits(got[k][:, ok]), _bits(chain[:, ok])), k
        want = N.project_cells(grid, dsm, rpc, N.ZONE)
        worst = max(worst, float(np.abs(got[k][:, ok] - want[:, ok]).max()))
        assert np.isnan(got[k][:, ~ok]).all() and np.isnan(want[:, ~ok]).all()
    print(f"col_row against the numpy chain: max |difference| = {worst:.3e} pixel (bar 1e-6)")
    assert worst <= 1e-6


# ---- everything downstream, over the shapes ------------------------------------------------------------------------------------------
FINE = N.fixture_lattice(0.25)          # 344 x 360 cells: a 257 x 1 row fits
SHAPES = {
    "lattice-43x45": (N.fixture_lattice(), None),
    "1-cell": (N.fixture_lattice(), (21, 22, 1, 1)),
    "255-cells": (N.fixture_lattice(), (9, 11, 17, 15)),
    "256-cells": (N.fixture_lattice(), (20, 5, 16, 16)),
    "257-cells": (FINE, (40, 150, 257, 1)),
    "513-cells-1x1-image": (FINE, (143, 157, 27, 19)),         # around pixel (20, 18) of the first image: the 1 x 1 image's footprint
    "589-cells-2x1-image": (FINE, (52, 258, 31, 19)),          # around pixels (7, 30), (8, 30): the 2 x 1 image's footprint
}


def _window(lattice, window):
    if window is None:
        return lattice, (lattice[5], lattice[6])
    return lattice[:3] + tuple(window), (lattice[5], lattice[6])


@pytest.mark.parametrize("shape", list(SHAPES))
def test_every_output_equals_the_restatement_bit_for_bit(shape):
    grid, lattice = _window(*SHAPES[shape])
    dsm = N.block_dsm(grid, holes=grid[5] * grid[6] > 3)
    vis = _cast(dsm, _rows(IMAGES, grid[2]))
    call = Call(grid, dsm, IMAGES, visible=vis, lattice=lattice).run()
    want = _assert_call(call, grid, dsm, IMAGES, vis)
    totals = np.stack([(want["state"] == s).sum(1) for s in range(4)], 1)
    assert (totals.sum(1) == grid[5] * grid[6]).all() and totals[:, N.SEEN].sum() > 0
    for name, k, w in (("513-cells-1x1-image", 5, 1), ("589-cells-2x1-image", 6, 2)):
        if shape == name:
            assert totals[k, N.SEEN] >= 16 * w                            # a 2 m pixel holds about 64 cells of 0.25 m
            cr = call.np("col_row")[k][:, want["state"][k] == N.SEEN]
            assert cr[0].min() < 0.0 and cr[0].max() > w - 1.0 and cr[1].min() < 0.0 < cr[1].max()      # every clamped neighbour is taken
    if shape == "lattice-43x45":
        assert totals[:5, N.HIDDEN].max() >= 20 and totals[:5, N.OUTSIDE].max() >= 20 and totals[:, N.HOLE].min() == 3
        # the finishes, used as they are, against the restatement's
        mos = N.mosaic(want["acc"])
        cells = call.cells
        rgb = torch.empty((3, cells), dtype=torch.float32, device=DEV)
        stats = torch.zeros(4, dtype=torch.int64, device=DEV)
        for ch in range(3):
            _lib.call("snerf_dsm_finish", call.acc["count"], call.acc["sum"][ch * cells:], cells, 0.0, 2.0 ** -24, rgb[ch], stats)
        assert np.array_equal(_bits(rgb.cpu().numpy()), _bits(mos["rgb"]))
        label, share, vstats = R.finish_votes(call.acc["votes"][:N.N_CLASSES * cells], grid[6], grid[5])
        assert np.array_equal(label.cpu().numpy().reshape(-1), mos["label"])
        assert np.array_equal(_bits(share.cpu().numpy().reshape(-1)), _bits(mos["share"]))
        assert int(vstats[1]) == int(want["acc"]["votes"].sum(0).max()) <= 7


def test_the_grid_stride_loop_runs_twice():
    """more cells than 8192 workgroups of 256 threads hold: one image, no labels, no visibility plane"""
    grid = N.fixture_lattice(0.059)
    cells = grid[5] * grid[6]
    assert 8192 * 256 < cells < 2 * 8192 * 256
    dsm = N.block_dsm(grid, holes=True)
    images = IMAGES[2:3]
    call = Call(grid, dsm, images, labels=False).run()
    want = _assert_call(call, grid, dsm, images, None, labels=False)
    assert (want["state"][0, 8192 * 256:] == N.SEEN).any()


@pytest.mark.parametrize("n_images", (1, 2, 64))
def test_one_two_and_sixty_four_images(n_images):
    grid = N.fixture_lattice()
    dsm = N.block_dsm(grid, holes=True)
    images = [IMAGES[k % len(IMAGES)] for k in range(n_images)]
    vis = _cast(dsm, _rows(images, grid[2]))
    want = _assert_call(Call(grid, dsm, images, visible=vis).run(), grid, dsm, images, vis)
    assert int(want["acc"]["count"].max()) >= min(n_images, 5)


@pytest.mark.parametrize("n_classes,labels,visible", [(1, True, True), (5, True, False), (255, True, True), (5, False, True), (5, False, False)],
                         ids=["C1", "C5-no-visibility", "C255", "no-labels", "no-labels-no-visibility"])
def test_class_counts_and_absent_planes(n_classes, labels, visible):
    grid = N.fixture_lattice()
    dsm = N.block_dsm(grid, holes=True)
    vis = _cast(dsm, _rows(IMAGES, grid[2])) if visible else None
    call = Call(grid, dsm, IMAGES, n_classes=n_classes, labels=labels, visible=vis).run()
    want = _assert_call(call, grid, dsm, IMAGES, vis, labels=labels, n_classes=n_classes)
    if not labels:
        assert (call.np("label") == N.NO_LABEL).all()
    elif n_classes == 1:      # labels 1 .. 4 do not vote, and still show in the per-image planes
        seen = want["state"] == N.SEEN
        assert want["acc"]["votes"].sum() < seen.sum() and set(np.unique(want["label"][seen])) == {0, 1, 2, 3, 4}
    if not visible:
        assert not (want["state"] == N.HIDDEN).any()


def test_a_window_is_the_same_cells_of_the_full_lattice():
    full = N.fixture_lattice()
    dsm = N.block_dsm(full, holes=True)
    vis = _cast(dsm, _rows(IMAGES, full[2]))
    whole = Call(full, dsm, IMAGES, visible=vis).run()
    ioff, joff, w, h = 7, 9, 20, 15
    grid = full[:3] + (ioff, joff, w, h)
    sub = np.ascontiguousarray(dsm[joff:joff + h, ioff:ioff + w])
    vsub = np.ascontiguousarray(vis.reshape(-1, full[6], full[5])[:, joff:joff + h, ioff:ioff + w])
    part = Call(grid, sub, IMAGES, visible=vsub, lattice=(full[5], full[6])).run()
    _assert_call(part, grid, sub, IMAGES, vsub.reshape(len(IMAGES), -1))
    for key, lead in (("col_row", (7, 2)), ("rgb", (7, 3)), ("label", (7,)), ("state", (7,)), ("sum", (3,)), ("count", ()), ("votes", (5,))):
        a = whole.np(key).reshape(lead + (full[6], full[5]))[..., joff:joff + h, ioff:ioff + w].reshape(lead + (-1,))
        b = part.np(key)
        assert a.tobytes() == np.ascontiguousarray(b).tobytes(), key


def test_two_calls_and_reversed_images_give_the_words_of_one_call():
    grid = N.fixture_lattice()
    dsm = N.block_dsm(grid, holes=True)
    vis = _cast(dsm, _rows(IMAGES, grid[2]))
    one = Call(grid, dsm, IMAGES, visible=vis).run()
    for order, cut in ((list(range(7)), 3), (list(range(7))[::-1], 7), ([4, 6, 0, 2, 5, 1, 3], 1)):
        first, second = order[:cut], order[cut:]
        a = Call(grid, dsm, [IMAGES[k] for k in first], visible=vis[first]).run()
        if second:
            Call(grid, dsm, [IMAGES[k] for k in second], visible=vis[second], acc=a.acc).run()
        for key in ("sum", "count", "votes", "stats"):
            assert np.array_equal(a.np(key), one.np(key)), (order, cut, key)
        assert a.tails_kept()


def test_hidden_cells_are_the_cells_the_numpy_march_shadows_under_the_view_row():
    grid = N.fixture_lattice()
    dsm = N.block_dsm(grid)
    rows = _rows(IMAGES[:5], grid[2])
    assert np.allclose(rows, N.fixture_rows(), rtol=0, atol=0)
    # the host layer's rows, from the device's localisation, against the numpy rows
    sc = N.fixture_scene()
    from snerf_amd.baseline.components.camera_models import RPCModel
    geo = types.SimpleNamespace(zone_string="17R")           # view_rows reads the zone alone
    got = R.view_rows([RPCModel(m["rpc"], device=DEV) for m in sc["metas"]], [m["min_alt"] for m in sc["metas"]],
                      [m["max_alt"] for m in sc["metas"]], [(m["width"], m["height"]) for m in sc["metas"]], geo, grid[2])
    # the two localisations agree to 1e-12 normalised (tests/test_gpu_scene.py) and the two UTM series to a few ulp of a 3.4e6 m
    # northing, 5e-10 m each, over the 10 m and more a line of sight travels: 1e-9 relative; the bar leaves a factor of ten
    print(f"view_rows against the numpy rows: max |difference| = {np.abs(got - rows).max():.3e}")
    assert np.abs(got - rows).max() <= 1e-8 * np.abs(rows).max()
    vis = _cast(dsm, rows)
    lit, _ = SN.cast(dsm, rows)
    assert np.array_equal(vis, lit.reshape(5, -1))
    with_, without = Call(grid, dsm, IMAGES[:5], visible=vis).run(), Call(grid, dsm, IMAGES[:5]).run()
    inside = without.np("state") == N.SEEN
    hidden = with_.np("state") == N.HIDDEN
    assert np.array_equal(hidden, inside & (lit.reshape(5, -1) == 0)) and hidden.sum(1).max() >= 20
    # a nadir image gets no cast: its plane is all 1
    t = torch.from_numpy(dsm).to(DEV)
    mixed = R.visibility(t, np.stack([rows[0], np.full(3, np.nan), rows[1]]))
    assert torch.equal(mixed[0].cpu(), torch.from_numpy(lit[0])) and bool((mixed[1] == 1).all()) and torch.equal(mixed[2].cpu(), torch.from_numpy(lit[1]))


# ---- memory and refusals -----------------------------------------------------------------------------------------------------------
def test_null_outputs_are_not_touched_and_nothing_is_written_behind_the_cells():
    grid = N.fixture_lattice()
    dsm = N.block_dsm(grid, holes=True)
    vis = _cast(dsm, _rows(IMAGES, grid[2]))
    full = Call(grid, dsm, IMAGES, visible=vis).run()
    bare = Call(grid, dsm, IMAGES, visible=vis, outputs=False).run()
    for key in ("sum", "count", "votes", "stats"):
        assert np.array_equal(bare.np(key), full.np(key)), key
    assert bare.tails_kept() and full.tails_kept()
    only_state = Call(grid, dsm, IMAGES, visible=vis)
    only_state.args.update(col_row=None, rgb_out=None, label_out=None)
    only_state.run()
    assert np.array_equal(only_state.np("state"), full.np("state"))
    for key, size in (("col_row", 2), ("rgb", 3), ("label", 1)):
        assert bool((only_state.out[key].view(torch.uint8) == FILL).all()), key       # not passed: not written


def test_no_output_depends_on_bytes_the_library_did_not_write():
    """the entry under the fills of tests/test_gpu_fill.py: the per-image planes are pure outputs (filled before the call), the sums,
    counts, votes and totals accumulators the caller zeroes; two runs under each fill and the three fills are bit-identical"""
    from tests.test_gpu_fill import run_filled
    grid = N.fixture_lattice()
    dsm = N.block_dsm(grid, holes=True)
    vis = _cast(dsm, _rows(IMAGES, grid[2]))

    def run(fill):
        call = Call(grid, dsm, IMAGES, visible=vis, fill=fill).run()
        assert call.tails_kept()
        return {k: call.tensor(k).clone() for k in ("col_row", "rgb", "label", "state", "sum", "count", "votes", "stats")}

    r = run_filled(run)[0xFF]
    want = N.sample_and_fuse(r["col_row"].cpu().numpy(), dsm, [im[1:] for im in IMAGES], N.fixture_scene()["rgbs"], N.fixture_scene()["labels"],
                             N.N_CLASSES, vis)
    assert np.array_equal(r["state"].cpu().numpy(), want["state"]) and np.array_equal(r["sum"].cpu().numpy(), want["acc"]["sum"])


def _bad_image(**kw):
    images = list(IMAGES)
    rpc, row0, w, h = images[1]
    rpc = dict(rpc, **{k: v for k, v in kw.items() if k.endswith("_scale")})
    images[1] = (rpc, kw.get("row0", row0), kw.get("w", w), kw.get("h", h))
    t = _table(images)
    return {"host": t}


REFUSALS = [
    ({"dsm": None}, 3), ({"grid": None}, 3), ({"host": None}, 3), ({"dev": None}, 3), ({"rgbs": None}, 3), ({"sum": None}, 3),
    ({"count": None}, 3), ({"stats": None}, 3), ({"votes": None}, 3), ({"labels": None}, 3),
    ({"grid": _lib.SnerfDsmGrid(0.0, 0.0, 0.0, 43, 45, 0, 0, 43, 45)}, 1), ({"grid": _lib.SnerfDsmGrid(0.0, 0.0, 2.0, 43, 45, 0, 0, 0, 45)}, 1),
    ({"grid": _lib.SnerfDsmGrid(0.0, 0.0, 2.0, 43, 45, 2 ** 31 - 5, 0, 43, 45)}, 1),
    ({"grid": _lib.SnerfDsmGrid(0.0, 0.0, 2.0, 1 << 16, 1 << 15, 0, 0, 1 << 16, 1 << 15)}, 1),
    ({"n_images": 0}, 1), ({"n_images": 65}, 1), ({"n_classes": 0}, 1), ({"n_classes": 256}, 1), ({"n_rows": 0}, 1),
    ({"lon0": 3.2}, 1), ({"lon0": math.nan}, 1), ({"south": -1}, 1),
    (_bad_image(w=0), 1), (_bad_image(h=0), 1), (_bad_image(row0=-1), 1), (_bad_image(row0=5107 - 33 * 29 + 1), 1),
    (_bad_image(lat_scale=0.0), 1), (_bad_image(col_scale=math.nan), 1),
]


def test_every_refusal_returns_its_code_and_leaves_the_buffers_as_they_were():
    grid = N.fixture_lattice()
    dsm = N.block_dsm(grid)
    for override, code in REFUSALS:
        call = Call(grid, dsm, IMAGES, visible=np.ones((7, grid[5] * grid[6]), np.uint8))
        call.args.update(override)
        bufs = list(call.out.values()) + list(call.acc.values())
        before = [t.clone() for t in bufs]
        with pytest.raises(ValueError, match=rf"snerf_orthorectify failed \(code {code}\): snerf_orthorectify: "):
            call.run()
        assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(bufs, before)), override


# ---- end to end --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def truth():
    """the scene's lidar DSM on its ROI (tests/golden/scene_small_dsm)"""
    from snerf_amd.eval.utils import dsm as D
    from snerf_amd.framework.util import img_utils as I
    d = os.path.join(DSM_DIR, "dsm")
    g = I.load_dsm_ground_truth(os.path.join(d, "JAX_068_DSM.tif"), os.path.join(d, "JAX_068_DSM.txt"), os.path.join(d, "JAX_068_CLS.tif"))
    return {"roi": D.roi_grid(g["roi"]), "roi_meta": g["roi"], "gt": g["gt"].to(DEV)}


def test_rectify_on_the_lidar_dsm_is_the_restatement(scene, truth):      # noqa: F811
    c, pipe, ds, geo = scene
    roi, gt = truth["roi"], truth["gt"]
    images = R.dataset_images(ds)
    assert [im["name"] for im in images] == [it["name"] for it in ds.items] and all(im["semantic"].dtype == torch.uint8 for im in images)
    res = R.rectify(gt, roi, geo, images, n_classes=ds.semantic_n_classes, keep_images=True)
    h, w = gt.shape
    n = len(images)
    assert res["grid"] == roi and tuple(res["rgb"].shape) == (3, h, w) and tuple(res["images"]["rgb"].shape) == (n, 3, h, w)
    assert sum(res["states"].values()) == n * h * w and res["states"]["seen"] > 0
    # the restatement on the same inputs: the device's view rows, cast and projection
    grid = (roi.xoff, roi.yoff, roi.resolution, 0, 0, w, h)
    dsm = gt.cpu().numpy()
    metas = ds.metas
    vis = R.visibility(gt, res["view_rows"]).cpu().numpy().reshape(n, -1)
    sc_images, rgbs, labels, at = [], [], [], 0
    for im in images:
        sc_images.append((at, im["w"], im["h"]))
        rgbs.append(im["rgbs"].cpu().numpy())
        labels.append(im["semantic"].cpu().numpy().reshape(-1))
        at += im["w"] * im["h"]
    col_row = np.stack([_device_chain(grid, dsm, m["rpc"]) for m in metas])
    want = N.sample_and_fuse(col_row, dsm, sc_images, np.concatenate(rgbs), np.concatenate(labels), ds.semantic_n_classes, vis)
    assert np.array_equal(res["images"]["state"].cpu().numpy().reshape(n, -1), want["state"])
    assert np.array_equal(_bits(res["images"]["rgb"].cpu().numpy().reshape(n, 3, -1)), _bits(want["rgb"]))
    assert np.array_equal(res["images"]["label"].cpu().numpy().reshape(n, -1), want["label"])
    mos = N.mosaic(want["acc"])
    assert np.array_equal(_bits(res["rgb"].cpu().numpy().reshape(3, -1)), _bits(mos["rgb"]))
    assert np.array_equal(res["label_vote"].cpu().numpy().reshape(-1), mos["label"])
    assert np.array_equal(res["count"].cpu().numpy().reshape(-1).view(np.uint32), want["acc"]["count"])
    assert list(res["states"].values()) == want["acc"]["stats"].tolist()
    # copies of the images (no shared bank tensor) take the concatenating path and give the same map
    again = R.rectify(gt, roi, geo, [dict(im, rgbs=im["rgbs"].clone(), semantic=im["semantic"].clone()) for im in images],
                      n_classes=ds.semantic_n_classes)
    assert _same(again["rgb"], res["rgb"]) and _same(again["label_vote"], res["label_vote"]) and again["states"] == res["states"]
    flat = R.rectify(gt, roi, geo, images, occlusion=False)
    assert flat["states"]["hidden"] == 0 and flat["states"]["seen"] == res["states"]["seen"] + res["states"]["hidden"]
    assert "label_vote" not in flat and "view_rows" not in flat and "images" not in flat


def test_export_rectified_writes_its_files_and_scores_a_model_on_the_map(scene, truth, tmp_path):      # noqa: F811
    from snerf_amd.eval.ortho import export_rectified
    from snerf_amd.eval.utils import dsm as D
    from snerf_amd.eval.utils.ortho import nadir_products
    from snerf_amd.framework.util import img_utils as I
    from tests.test_gpu_nadir import OPTS
    c, pipe, ds, geo = scene
    W, H = 9, 7
    window = D.grid_struct(truth["roi"], (40, 50, W, H))
    prod = nadir_products(c, pipe.renderer, pipe.models, dataset=ds, geo=geo, grid=window, t=0, render_options=OPTS)
    out = export_rectified(c, ds, str(tmp_path), split="test", model_products=prod)
    names = [it["name"] for it in ds.items]
    stems = [f"{n}_{k}" for n in names for k in ("rgb", "state", "label")] + ["mosaic_rgb", "mosaic_label", "coverage", "vote_share"]
    want_files = {s + e for s in stems for e in (".png", ".tif")} | {"map_eval.json"}
    d = tmp_path / "rectified" / "test"
    assert set(out["files"]) == want_files == set(os.listdir(d))
    grid = out["grid"]
    assert grid == prod["grid"]
    tf = (grid.xoff, grid.yoff, grid.resolution, grid.resolution)
    for stem, plane in [("coverage", out["count"].float()), ("vote_share", out["vote_share"]), ("mosaic_label", out["label_vote"])] + [
            (f"{n}_state", out["images"]["state"][k]) for k, n in enumerate(names)] + [(f"{n}_label", out["images"]["label"][k]) for k, n in enumerate(names)]:
        a, got_tf = I.load_dsm_geotiff(out["files"][stem + ".tif"])
        assert got_tf == tf and a.dtype == plane.cpu().numpy().dtype and a.tobytes() == plane.cpu().numpy().tobytes(), stem
    from PIL import Image
    with Image.open(out["files"]["mosaic_rgb.tif"]) as im:
        px = np.array(im)
    want = torch.nan_to_num(out["rgb"], nan=0.0).mul(255).add(0.5).clamp(0, 255).to(torch.uint8).permute(1, 2, 0).cpu().numpy()
    assert np.array_equal(px, want)
    with open(out["files"]["map_eval.json"]) as f:
        doc = json.load(f)
    assert sorted(doc) == ["label", "rgb"] and doc["label"]["confusion"] == out["map_eval"]["label"]["confusion"]
    conf = np.array(doc["label"]["confusion"])
    assert conf.shape == (5, 5) and int(conf.sum()) == doc["label"]["label_cells"]
    both = (out["label_vote"] != 255) & (prod["label"] != 255)
    assert doc["label"]["label_cells"] == int(both.sum()) > 0
    assert doc["rgb"]["psnr_cells"] == int(torch.isfinite(out["rgb"]).all(0).sum()) > 0 and math.isfinite(doc["rgb"]["psnr"])
    print(f"map_eval on the untrained model: PSNR {doc['rgb']['psnr']:.2f} dB over {doc['rgb']['psnr_cells']} cells, accuracy "
          f"{doc['label']['accuracy']:.3f}, mIoU {doc['label']['mIoU']:.3f} over {doc['label']['label_cells']} cells (no bar)")
    # without a model map the scene's lidar DSM on its ROI is the surface, and nothing is scored; a scene without one says so
    with pytest.raises(ValueError, match="no ground-truth DSM on disk"):
        export_rectified(c, ds, str(tmp_path / "x"), split="test")
    with_gt = copy.copy(ds)
    with_gt.dsm = {"gt": truth["gt"], "roi": truth["roi_meta"], "geo": geo}
    lidar = export_rectified(c, with_gt, str(tmp_path / "lidar"), split="test")
    assert lidar["grid"] == truth["roi"] and "map_eval" not in lidar and set(lidar["files"]) == want_files - {"map_eval.json"}
    # a model map on another grid is refused
    other = dict(prod, grid=D.DsmGrid(grid.xoff + 1.0, grid.yoff, grid.resolution, W, H))
    with pytest.raises(ValueError, match="the model's products lie on"):
        export_rectified(c, ds, str(tmp_path / "x"), dsm=prod["dsm"], grid=prod["grid"], model_products=other)
