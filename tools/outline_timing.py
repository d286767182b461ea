#!/usr/bin/env python3
"""The outline kernels (snerf_amd eval/utils/outline.py, csrc/outline.hip) on rasters built here: the synthetic town of
tools/objects_timing.py (--sides^2 cells: a few hundred rectangles and blobs, short rings) and a square spiral one cell wide with one
cell between its turns (ONE object and ONE ring about as long as the raster has cells: the deepest jump chain and every emit atomic on
one row).  Nothing outside the repository is read.

Prints one JSON line.  Per side and raster: the edges, rings, vertices and jump rounds; the device time of snerf_outline_sides,
snerf_outline_link, snerf_outline_rank (its 2 R + 4 launches) and snerf_outline_emit, each over an event-bracketed window of --reps
back-to-back calls after a warm-up call; and the whole rings() call as the host sees it (launches, the three synchronising reads, the
torch plumbing between the entries and the copy of the result: the median of --reps calls after a warm-up call)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from _timing import wall_ms, warm_window_ms as window_ms  # noqa: E402
from objects_timing import town  # noqa: E402
from snerf_amd import _lib  # noqa: E402
from snerf_amd.eval.utils import objects as OB  # noqa: E402
from snerf_amd.eval.utils import outline as OL  # noqa: E402


def spiral(side):
    """rings at every second depth, each cut below its north-west corner and joined to the next one: a single 4-connected path"""
    jj, ii = np.mgrid[0:side, 0:side]
    depth = np.minimum(np.minimum(ii, jj), np.minimum(side - 1 - ii, side - 1 - jj))
    on = depth % 2 == 0
    for k in range(0, (side + 1) // 2, 2):
        inner = side - 2 * k                              # the ring at depth k is inner x inner cells
        if inner >= 3:
            on[k + 1, k] = False
        if inner >= 5:
            on[k + 2, k + 1] = True
    return np.where(on, 3, 0).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sides", type=int, nargs="+", default=[1024, 2048])
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {}
    for side in a.sides:
        for name, label in (("town", town(side)[0]), ("spiral", spiral(side))):
            tag = f"s{side}_{name}"
            ids, K = OB.components(torch.from_numpy(label).to(dev), (3, 4), 4)
            side_bits, sstats = OL.sides(ids, K)
            offsets, E = OL.offsets_of(side_bits)
            slot, nxt, flags, _ = OL.link(ids, side_bits, offsets, K, 4, E)
            ring, rank, ordinal, totals, _ = OL.rank_rings(nxt, flags)
            ring_row, vertex_offset, n_rings, V = OL.ring_rows(ring, totals)
            vertices, rows, _ = OL.emit(ids, slot, flags, ring, ordinal, ring_row, vertex_offset, n_rings, V)
            rounds = max(1, (max(E, 2) - 1).bit_length())
            out.update({f"{tag}_objects": K, f"{tag}_edges": E, f"{tag}_rings": n_rings, f"{tag}_vertices": V, f"{tag}_rounds": rounds,
                        f"{tag}_longest_ring": int(totals[:, 0].max()) if E else 0})
            s4, s2 = torch.zeros(4, dtype=torch.int64, device=dev), torch.zeros(2, dtype=torch.int64, device=dev)
            ws = torch.empty(OL.workspace_bytes(E) // 4, dtype=torch.int32, device=dev)
            out[f"{tag}_sides_ms"] = window_ms(lambda: _lib.call("snerf_outline_sides", ids, side, side, K, side_bits, s4), a.reps)
            out[f"{tag}_link_ms"] = window_ms(
                lambda: _lib.call("snerf_outline_link", ids, side_bits, offsets, side, side, K, 4, E, slot, nxt, flags, s2), a.reps)
            out[f"{tag}_rank_ms"] = window_ms(
                lambda: _lib.call("snerf_outline_rank", nxt, flags, E, ring, rank, ordinal, totals, ws, 4 * ws.numel(), s2), a.reps)
            out[f"{tag}_emit_ms"] = window_ms(
                lambda: _lib.call("snerf_outline_emit", ids, slot, flags, ring, ordinal, ring_row, vertex_offset, side, side, E, n_rings, V,
                                  vertices, rows, s2), a.reps)
            out[f"{tag}_rings_wall_ms"] = wall_ms(lambda: OL.rings(ids, K, 4), a.reps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
