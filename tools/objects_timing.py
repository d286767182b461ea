#!/usr/bin/env python3
"""The objects kernels (snerf_amd eval/utils/objects.py, csrc/objects.hip) on synthetic towns built here: --sides^2 cells at 0.5 m,
ground class 0 at 3 m with a gentle slope, class-3 boxes of 12 to 60 cells a side on a jittered street grid (roofs 6 to 40 m above
the ground), class-4 blobs of 2 x 4 cells between them.  Nothing outside the repository is read.

Prints one JSON line.  Per side: the device time of snerf_objects_link (its three launches) at connectivity 4 and 8 and of
snerf_objects_stats at ring 0, 2 and 7, each over an event-bracketed window of --reps back-to-back calls; the stats launch on ONE
object that covers the raster (every wave's atomics land on one 128-byte row: the same-address extreme, with the atomics per
microsecond that row took) and on a checkerboard of single-cell objects (no lane shares a row with another); the whole objects()
call as the host sees it (launch + synchronise + the table, the median of --reps calls after a warm-up call); and beside them the
only route to the same table without these kernels: the device-to-host copy of label and altitude plus scipy.ndimage.label, when
scipy is installed (the per-object reductions would come on top of it)."""
import argparse
import json
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


def town(side, seed=0):
    rng = np.random.default_rng(seed)
    jj, ii = np.mgrid[0:side, 0:side]
    label = np.zeros((side, side), np.uint8)
    alt = (3.0 + (ii + 2 * jj) / 1024.0).astype(np.float32)
    pitch = 80
    for j0 in range(8, side - pitch, pitch):
        for i0 in range(8, side - pitch, pitch):
            nj, ni = rng.integers(12, 61, 2)
            dj, di = rng.integers(0, pitch - 64, 2)
            label[j0 + dj:j0 + dj + nj, i0 + di:i0 + di + ni] = 3
            alt[j0 + dj:j0 + dj + nj, i0 + di:i0 + di + ni] = 3.0 + float(rng.integers(6, 41))
            label[j0 + 68:j0 + 70, i0 + 4:i0 + 8] = 4
            alt[j0 + 68:j0 + 70, i0 + 4:i0 + 8] += 1.5
    return label, alt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sides", type=int, nargs="+", default=[512, 2048])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-host-route", action="store_true", help="skip the copy + scipy route (a profiler run)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {}
    for side in a.sides:
        tag = f"s{side}"
        h_label, h_alt = town(side)
        label, alt = torch.from_numpy(h_label).to(dev), torch.from_numpy(h_alt).to(dev)
        grid = D.DsmGrid(500000.0, 4100000.0, 0.5, side, side)
        members, ground = OB.class_table((3, 4)), OB.class_table((0,))
        parent = torch.empty(side * side, dtype=torch.int32, device=dev)
        lstats = torch.zeros(2, dtype=torch.int64, device=dev)
        for conn in (4, 8):
            out[f"{tag}_link{conn}_ms"] = window_ms(
                lambda: _lib.call("snerf_objects_link", label, side, side, members, conn, parent, lstats), a.reps)
        ids, K = OB.components(label, (3, 4), 4)
        out[f"{tag}_objects"] = K
        out[f"{tag}_object_cells"] = int((ids > 0).sum())
        rows, stats = OB.new_rows(K, dev), torch.zeros(4, dtype=torch.int64, device=dev)

        def stats_ms(ids, K, label, rows, ring):
            return window_ms(lambda: _lib.call("snerf_objects_stats", ids, label, alt, side, side, K, ground, ring, OR.Z0, OR.Q, 0, side,
                                               rows, stats), a.reps)
        for ring in (0, 2, 7):
            out[f"{tag}_stats_r{ring}_ms"] = stats_ms(ids, K, label, rows, ring)
        # the two extremes of the wave reduction, without a ring: the atomics alone
        one = torch.ones_like(ids)
        row1 = OB.new_rows(1, dev)
        ms = stats_ms(one, 1, torch.full_like(label, 3), row1, 0)
        out[f"{tag}_stats_one_object_ms"] = ms
        out[f"{tag}_stats_one_object_atomics_per_us"] = (side * side / 64) * 12 / (ms * 1e3)      # a wave: 12 no-return atomics
        checker = (torch.arange(side, device=dev)[:, None] + torch.arange(side, device=dev)[None, :]) % 2 == 0
        single = torch.where(checker, torch.cumsum(checker.reshape(-1).int(), 0, dtype=torch.int32).reshape(side, side),
                             torch.zeros_like(ids))
        n_single = int(single.max())
        ms = stats_ms(single, n_single, torch.full_like(label, 3), OB.new_rows(n_single, dev), 0)
        out[f"{tag}_stats_single_cells_ms"] = ms
        out[f"{tag}_stats_single_cells_atomics_per_us"] = n_single * 13 / (ms * 1e3)      # per object 13: the perimeter word too
        out[f"{tag}_objects_wall_ms"] = wall_ms(lambda: OB.objects(label, alt, grid, (3, 4), (0,)), a.reps)
        if a.no_host_route:
            continue
        try:
            from scipy import ndimage
        except ImportError:
            continue
        t0 = time.perf_counter()
        hl, ha = label.cpu().numpy(), alt.cpu().numpy()
        t1 = time.perf_counter()
        n_host = sum(ndimage.label(hl == c)[1] for c in (3, 4))
        t2 = time.perf_counter()
        out[f"{tag}_copy_to_host_ms"] = (t1 - t0) * 1e3
        out[f"{tag}_scipy_label_ms"] = (t2 - t1) * 1e3
        out[f"{tag}_same_count"] = bool(n_host == K) and ha.shape == hl.shape
    print(json.dumps(out))


if __name__ == "__main__":
    main()
