#!/usr/bin/env python3
"""The roof kernels (snerf_amd eval/utils/roofs.py, csrc/roofs.hip) on synthetic towns built here: --sides^2 cells at 0.5 m, a level
ground with buildings of 16 to 60 cells a side on a jittered street grid under flat, shed, gabled and hipped roofs (tan 0.5), plus a
noise of +-2 cm.  Nothing outside the repository is read.

Prints one JSON line.  Per side: the device time of snerf_roofs_normals at radius 1 and 4, of snerf_roofs_link (its three launches), of
snerf_roofs_moments and of snerf_roofs_residuals on the facets of the radius-1 normals, each over an event-bracketed window of --reps
back-to-back calls after a warm-up call; the whole roofs() call as the host sees it (launches + the host's plane solve + synchronise,
the median of --reps calls after a warm-up call) at radius 1 and 4; and beside them the only route to the normals without these
kernels: the numpy restatement of tests/roofs_numpy.py on the same raster on the host (one call; --no-host-route skips it)."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from _timing import wall_ms, warm_window_ms as window_ms  # noqa: E402
from snerf_amd import _lib  # noqa: E402
from snerf_amd.eval.utils import dsm as D  # noqa: E402
from snerf_amd.eval.utils import objects as OB  # noqa: E402
from snerf_amd.eval.utils import ortho as OR  # noqa: E402
from snerf_amd.eval.utils import roofs as RF  # noqa: E402
from snerf_amd.eval.utils import terrain as TR  # noqa: E402

RADII = (1, 4)
RES = 0.5


def tan2(deg):
    t = math.tan(math.radians(deg))
    return t * t


def town(side, seed=0):
    """-> (alt f32, label u8: 3 on the buildings)"""
    rng = np.random.default_rng(seed)
    alt = np.full((side, side), 3.0)
    label = np.zeros((side, side), np.uint8)
    pitch = 80
    for j0 in range(8, side - pitch, pitch):
        for i0 in range(8, side - pitch, pitch):
            nj, ni = (int(v) for v in rng.integers(16, 61, 2))
            dj, di = (int(v) for v in rng.integers(0, pitch - 64, 2))
            jj, ii = np.mgrid[0:nj, 0:ni]
            kind = int(rng.integers(0, 4))
            rise = (np.zeros((nj, ni)), jj, np.minimum(ii, ni - 1 - ii), np.minimum(np.minimum(jj, nj - 1 - jj), np.minimum(ii, ni - 1 - ii)))[kind]
            alt[j0 + dj:j0 + dj + nj, i0 + di:i0 + di + ni] = 3.0 + float(rng.integers(6, 41)) + 0.25 * rise
            label[j0 + dj:j0 + dj + nj, i0 + di:i0 + di + ni] = 3
    alt += rng.uniform(-0.02, 0.02, alt.shape)
    return alt.astype(np.float32), label


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sides", type=int, nargs="+", default=[2048])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-host-route", action="store_true", help="skip the numpy restatement on the host (a profiler run)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {}
    for side in a.sides:
        tag_ = f"s{side}"
        h_alt, h_label = town(side)
        alt, label = torch.from_numpy(h_alt).to(dev), torch.from_numpy(h_label).to(dev)
        grid = D.DsmGrid(500000.0, 4100000.0, RES, side, side)
        objects = OB.objects(label, alt, grid, classes=(3,), ground=(0,))
        ids, K = objects["ids"], objects["n"]
        key, _, _ = TR.keys(alt)
        out[f"{tag_}_objects"] = K
        se, sn = torch.empty_like(alt), torch.empty_like(alt)
        code = torch.empty((side, side), dtype=torch.uint8, device=dev)
        tag = torch.empty((side, side), dtype=torch.int32, device=dev)
        nstats = torch.zeros(4, dtype=torch.int64, device=dev)
        t5, t60 = tan2(5.0), tan2(60.0)
        for r in reversed(RADII):                                # radius 1 last: its tags feed the entries below
            out[f"{tag_}_normals_r{r}_ms"] = window_ms(
                lambda: _lib.call("snerf_roofs_normals", key, ids, side, side, K, r, OR.Q, RES, 1.0, 0.0, t5, t60, se, sn, code, tag, nstats), a.reps)
        parent = torch.empty(side * side, dtype=torch.int32, device=dev)
        lstats = torch.zeros(2, dtype=torch.int64, device=dev)
        out[f"{tag_}_link_ms"] = window_ms(lambda: _lib.call("snerf_roofs_link", tag, side, side, 4, parent, lstats), a.reps)
        fids, F = OB.ids_from_parent(parent, side, side)
        out[f"{tag_}_facets"] = F
        rows, mstats = RF.facet_rows(fids, F, parent, key, tag)
        planes = torch.from_numpy(RF.facet_table(rows, grid)["plane"]).to(dev)
        scratch = rows.clone()
        out[f"{tag_}_moments_ms"] = window_ms(
            lambda: _lib.call("snerf_roofs_moments", fids, parent.reshape(side, side), key, tag, side, side, F, 0, side, scratch, mstats), a.reps)
        residual = torch.empty_like(alt)
        rrows = torch.zeros((F, RF.RESIDUAL_WORDS), dtype=torch.int64, device=dev)
        rstats = torch.zeros(3, dtype=torch.int64, device=dev)
        out[f"{tag_}_residuals_ms"] = window_ms(
            lambda: _lib.call("snerf_roofs_residuals", fids, parent.reshape(side, side), key, side, side, F, planes, OR.Q, RF.UNIT, 0, side,
                              residual, rrows, rstats), a.reps)
        for r in RADII:
            res = None

            def whole():
                nonlocal res
                res = RF.roofs(alt, ids, K, grid, objects["table"], radius=r)
            out[f"{tag_}_roofs_r{r}_wall_ms"] = wall_ms(whole, a.reps)
            out[f"{tag_}_roofs_r{r}_kept_facets"] = res["n_facets"]
        if a.no_host_route:
            continue
        from tests import roofs_numpy as N
        h_key, h_ids = key.cpu().numpy(), ids.cpu().numpy()
        for r in RADII:
            t0 = time.perf_counter()
            host = N.normals(h_key, h_ids, K, r, OR.Q, RES)
            out[f"{tag_}_numpy_normals_r{r}_ms"] = (time.perf_counter() - t0) * 1e3
            if r == 1:
                out[f"{tag_}_numpy_matches"] = bool(np.array_equal(host[2], code.cpu().numpy()))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
