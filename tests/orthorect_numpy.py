"""NumPy restatement of snerf_orthorectify (tests only), written from include/snerf_orthorect.h, in
two halves:

project_cells -- steps 1 to 4: the cell centres of a window, tests/utm_inverse_numpy.to_latlon and tests/rpc_numpy's projection.
numpy's sin / cos are not the device's, so the kernel's col_row is held to this half within 1e-6 pixel (the bar of
tests/test_gpu_scene.py's projection check), and bit for bit to snerf_geo_points + snerf_rpc_project instead.

sample_and_fuse -- steps 5 to 7 on GIVEN (col, row): the states, the bilinear colour, the label, the integer sums, counts, votes and
the four totals.  Only fp64 + - * and comparisons, floor and rint, one rounding per operation, so fed the device's own col_row
it reproduces every other output of the kernel BIT FOR BIT (numpy evaluates `(1 - fx) * p00 + fx * p10` as four ufunc calls: no
contraction).

view_rows / mosaic restate the host layer's view direction and the two finishes (snerf_dsm_finish with z0 = 0, q = 2^-24 per
channel; snerf_ortho_votes_finish)."""
import functools
import json
import os

import numpy as np

from tests import rpc_numpy
from tests import utm_inverse_numpy as UI
from tests import utm_numpy as U

SEEN, HOLE, OUTSIDE, HIDDEN = 0, 1, 2, 3
NO_LABEL = 255
Q = 2.0 ** -24


def cell_centres(grid):
    """grid = (xoff, yoff, res, ioff, joff, out_w, out_h) -> (east, north), each (out_h * out_w) fp64, row-major, row 0 north"""
    xoff, yoff, res, ioff, joff, w, h = grid
    east = np.float64(xoff) + (np.arange(w, dtype=np.float64) + float(ioff) + 0.5) * np.float64(res)
    north = np.float64(yoff) - (np.arange(h, dtype=np.float64) + float(joff) + 0.5) * np.float64(res)
    return np.broadcast_to(east[None, :], (h, w)).reshape(-1).copy(), np.broadcast_to(north[:, None], (h, w)).reshape(-1).copy()


def project_cells(grid, dsm, rpc, zone, south=False):
    """steps 1 to 4 for one image: (2, cells) fp64 (col, row), NaN where the DSM is not finite"""
    east, north = cell_centres(grid)
    alt = np.asarray(dsm, np.float32).reshape(-1).astype(np.float64)
    ok = np.isfinite(alt)
    out = np.full((2, alt.size), np.nan)
    if ok.any():
        lat, lon = UI.to_latlon(east[ok], north[ok], zone, south)
        col, row = rpc_numpy.RPCModel(rpc).projection(lon, lat, alt[ok])
        out[0, ok], out[1, ok] = col, row
    return out


def new_acc(cells, n_classes=None):
    """zeroed accumulators: sum (3, cells) int64, count (cells) uint32, votes (n_classes, cells) uint32 or None, stats (4) uint64"""
    return {"sum": np.zeros((3, cells), np.int64), "count": np.zeros(cells, np.uint32),
            "votes": None if n_classes is None else np.zeros((n_classes, cells), np.uint32), "stats": np.zeros(4, np.uint64)}


def sample_and_fuse(col_row, dsm, images, rgbs, labels=None, n_classes=None, visible=None, acc=None):
    """steps 2 and 5 to 7 of one call.  col_row (n_images, 2, cells) fp64; dsm (cells) fp32 (only its holes are read); images: a
    list of (row0, w, h); rgbs (n_rows, 3) fp32; labels (n_rows) uint8 or None; visible (n_images, cells) uint8 or None; acc:
    new_acc's dict, added to IN PLACE (a zeroed one is made otherwise).
    Returns {"state" (n, cells) u8, "rgb" (n, 3, cells) f32, "label" (n, cells) u8, "acc"}."""
    col_row = np.asarray(col_row, np.float64)
    n, _, cells = col_row.shape
    rgbs = np.asarray(rgbs, np.float32).reshape(-1, 3)
    hole = ~np.isfinite(np.asarray(dsm, np.float32).reshape(-1))
    acc = new_acc(cells, n_classes if labels is not None else None) if acc is None else acc
    state = np.empty((n, cells), np.uint8)
    rgb = np.full((n, 3, cells), np.nan, np.float32)
    label = np.full((n, cells), NO_LABEL, np.uint8)
    one = np.float64(1.0)
    with np.errstate(invalid="ignore", over="ignore"):
        for k, (row0, w, h) in enumerate(images):
            col, row = col_row[k]
            ci, ri = np.floor(col + 0.5), np.floor(row + 0.5)
            inside = (ci >= 0.0) & (ci < float(w)) & (ri >= 0.0) & (ri < float(h))
            st = np.where(hole, HOLE, OUTSIDE).astype(np.uint8)
            hidden = ~hole & inside & (np.asarray(visible[k]).reshape(-1) != 1 if visible is not None else False)
            st[hidden] = HIDDEN
            s = np.nonzero(~hole & inside & ~hidden)[0]
            c0, r0 = np.floor(col[s]), np.floor(row[s])
            fx, fy = col[s] - c0, row[s] - r0
            x0, x1 = np.clip(c0.astype(np.int64), 0, w - 1), np.clip(c0.astype(np.int64) + 1, 0, w - 1)
            y0, y1 = np.clip(r0.astype(np.int64), 0, h - 1), np.clip(r0.astype(np.int64) + 1, 0, h - 1)
            v = np.empty((3, s.size))
            for ch in range(3):
                p = [rgbs[row0 + y * w + x, ch].astype(np.float64) for y, x in ((y0, x0), (y0, x1), (y1, x0), (y1, x1))]
                top = (one - fx) * p[0] + fx * p[1]
                bot = (one - fx) * p[2] + fx * p[3]
                v[ch] = (one - fy) * top + fy * bot
            fin = np.isfinite(v).all(0)
            s, v = s[fin], v[:, fin]
            st[s] = SEEN
            state[k] = st
            rgb[k][:, s] = v.astype(np.float32)
            q = np.rint(np.clip(v * 16777216.0, -2.0 ** 62, 2.0 ** 62)).astype(np.int64)
            acc["sum"][:, s] += q                                             # int64: wraps as the device's sums do
            acc["count"][s] += np.uint32(1)
            if labels is not None:
                lab = np.asarray(labels, np.uint8).reshape(-1)[row0 + ri[s].astype(np.int64) * w + ci[s].astype(np.int64)]
                label[k, s] = lab
                vote = lab < n_classes
                acc["votes"][lab[vote], s[vote]] += np.uint32(1)              # a cell occurs once in s: no repeated index
            for code in range(4):
                acc["stats"][code] += np.uint64(int(np.sum(st == code)))
    return {"state": state, "rgb": rgb, "label": label, "acc": acc}


def mosaic(acc):
    """the two finishes: {"rgb" (3, cells) f32 -- f32(0 + 2^-24 * sum / count), NaN where count = 0 --, "label" (cells) u8 -- the class
    with the most votes, the lowest on a tie, 255 without one --, "share" (cells) f32}"""
    cnt = acc["count"].astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        rgb = np.where(cnt > 0, 0.0 + Q * (acc["sum"].astype(np.float64) / cnt), np.nan).astype(np.float32)
        out = {"rgb": rgb}
        if acc["votes"] is not None:
            v = acc["votes"].astype(np.int64)
            total, best = v.sum(0), v.max(0)
            out["label"] = np.where(total > 0, v.argmax(0), NO_LABEL).astype(np.uint8)
            out["share"] = np.where(total > 0, best.astype(np.float64) / total.astype(np.float64), np.nan).astype(np.float32)
    return out


def view_row(rpc, w, h, alt_min, alt_max, zone, res, south=False, pixel=None):
    """the (ux, uy, rise) row of an image's line of sight, pointing towards the satellite: `pixel` (default the image centre)
    localised at alt_min and alt_max, both taken to UTM.  None for a nadir image (no horizontal travel)."""
    col, row = ((w - 1) / 2.0, (h - 1) / 2.0) if pixel is None else pixel
    cam = rpc_numpy.RPCModel(rpc)
    lon, lat = cam.localization(np.array([col, col]), np.array([row, row]), np.array([alt_min, alt_max], np.float64))
    east, north = U.from_latlon(lat, lon, zone, south)
    de, dn = east[1] - east[0], north[1] - north[0]
    dh = np.hypot(de, dn)
    if dh < 1e-9 * (alt_max - alt_min):
        return None
    return np.array([de / dh, -dn / dh, (alt_max - alt_min) / dh * res])


# ---- the fixture scene as both test files use it --------------------------------------------------------------------------------
SCENE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scene_small")
ZONE = 17
N_CLASSES = 5
ALT = 0.0            # the ground plane of the block DSM, and the altitude the lattice is built at
BLOCK_TOP = 30.0     # the block's altitude: "about 30 m tall"
RES = 2.0            # metres per cell: about one cell per pixel (the fixture's pixels are about 2 m wide)


@functools.lru_cache(maxsize=None)
def fixture_scene():
    """{"names", "metas", "images": [(row0, w, h)], "rgbs" (n_rows, 3) f32, "labels" (n_rows) u8}: the five images of
    tests/golden/scene_small, train split first, as the loaders decode them"""
    from PIL import Image
    with open(os.path.join(SCENE, "root.json")) as f:
        root = json.load(f)
    names = root["train_split"] + root["test_split"]
    metas, images, rgbs, labels, at = [], [], [], [], 0
    for name in names:
        with open(os.path.join(SCENE, "metas", name)) as f:
            m = json.load(f)
        w, h = int(m["width"]), int(m["height"])
        with Image.open(os.path.join(SCENE, "images", m["img"])) as im:
            px = np.array(im)
        with Image.open(os.path.join(SCENE, root["semantic_dp_own"], m["img"][:-7] + "CLS.tif")) as im:
            cls = np.array(im)
        assert px.shape == (h, w, 3) and px.dtype == np.uint8 and cls.shape == (h, w) and cls.dtype == np.uint8
        rgbs.append((px.reshape(-1, 3) / 255.0).astype(np.float32))
        labels.append(cls.reshape(-1))
        metas.append(m)
        images.append((at, w, h))
        at += w * h
    return {"names": names, "metas": metas, "images": images, "rgbs": np.concatenate(rgbs), "labels": np.concatenate(labels)}


def fixture_lattice(res=RES, alt=ALT):
    """(xoff, yoff, res, 0, 0, w, h): the lattice of `res` metres that covers the corners of the five images localised at `alt`"""
    east, north = [], []
    for m in fixture_scene()["metas"]:
        w, h = m["width"], m["height"]
        lon, lat = rpc_numpy.RPCModel(m["rpc"]).localization(np.array([0.0, w - 1.0, 0.0, w - 1.0]), np.array([0.0, 0.0, h - 1.0, h - 1.0]),
                                                             np.full(4, float(alt)))
        e, n = U.from_latlon(lat, lon, ZONE)
        east += e.tolist()
        north += n.tolist()
    xoff, yoff = np.floor(min(east) / res) * res, np.ceil(max(north) / res) * res
    return (float(xoff), float(yoff), float(res), 0, 0, int(np.ceil((max(east) - xoff) / res)), int(np.ceil((yoff - min(north)) / res)))


def block_dsm(grid, holes=False):
    """the plane at ALT with one block of BLOCK_TOP over the middle fifth of the window (and, with `holes`, a NaN and an infinite
    cell on the plane and a NaN cell on the block)"""
    w, h = grid[5], grid[6]
    dsm = np.full((h, w), ALT, np.float32)
    j0, j1, i0, i1 = (2 * h) // 5, max((3 * h) // 5, (2 * h) // 5 + 1), (2 * w) // 5, max((3 * w) // 5, (2 * w) // 5 + 1)
    dsm[j0:j1, i0:i1] = BLOCK_TOP
    if holes:
        dsm[h // 7, w // 3] = np.nan
        dsm[(5 * h) // 6, w // 2] = np.inf
        dsm[j0, i0] = np.nan
    return dsm


def fixture_rows(res=RES):
    """the view rows of the five images (view_row at the image centres)"""
    return np.stack([view_row(m["rpc"], m["width"], m["height"], m["min_alt"], m["max_alt"], ZONE, res) for m in fixture_scene()["metas"]])
