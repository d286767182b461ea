#!/usr/bin/env python3
"""The roof-line kernels (snerf_amd eval/utils/roofs.py grow, eval/utils/arcs.py, csrc/rooflines.hip) on the synthetic towns of
tools/roofs_timing.py: --sides^2 cells at 0.5 m (2048^2: 625 buildings).  Nothing outside the repository is read.

Prints one JSON line.  Per side: the kept facets of roofs() at radius 1, the device time of one snerf_roofs_grow call of 8 rounds and the
whole roofs.grow call as the host sees it (batches of 8 rounds, one read of the counters a batch); on the grown raster the device time
of snerf_arcs_first, snerf_arcs_mark and snerf_arcs_fold, each over an event-bracketed window of --reps back-to-back calls after a
warm-up call; and the whole arcs() call as the host sees it (the outline entries, the three arc entries, the cumulative sums between
them, the copies to the host and the checks of the pairing; the median of --reps calls after a warm-up call)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from _timing import wall_ms, warm_window_ms as window_ms  # noqa: E402
from roofs_timing import RES, town  # noqa: E402
from snerf_amd import _lib  # noqa: E402
from snerf_amd.eval.utils import arcs as AR  # noqa: E402
from snerf_amd.eval.utils import dsm as D  # noqa: E402
from snerf_amd.eval.utils import objects as OB  # noqa: E402
from snerf_amd.eval.utils import ortho as OR  # noqa: E402
from snerf_amd.eval.utils import outline as OL  # noqa: E402
from snerf_amd.eval.utils import roofs as RF  # noqa: E402
from snerf_amd.eval.utils import terrain as TR  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sides", type=int, nargs="+", default=[2048])
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {}
    for side in a.sides:
        tag = f"s{side}"
        h_alt, h_label = town(side)
        alt, label = torch.from_numpy(h_alt).to(dev), torch.from_numpy(h_label).to(dev)
        grid = D.DsmGrid(500000.0, 4100000.0, RES, side, side)
        objects = OB.objects(label, alt, grid, classes=(3,), ground=(0,))
        ids, K = objects["ids"], objects["n"]
        key, _, _ = TR.keys(alt)
        res = RF.roofs(alt, ids, K, grid, objects["table"])
        fids, table, F = res["facet_ids"], res["facets"], res["n_facets"]
        out[f"{tag}_objects"], out[f"{tag}_kept_facets"] = K, F
        out[f"{tag}_cells_without_facet"] = int(((fids == 0) & (ids > 0)).sum())
        planes = torch.from_numpy(table["plane"]).to(dev)
        root = torch.from_numpy(table["root"].astype("int32")).to(dev)
        buf_a, buf_b = torch.empty_like(fids), torch.empty_like(fids)
        gstats = torch.zeros(RF.GROW_BATCH + 1, dtype=torch.int64, device=dev)
        max_rq = int(0.25 / (OR.Q * RF.UNIT))
        out[f"{tag}_grow_8_rounds_ms"] = window_ms(
            lambda: _lib.call("snerf_roofs_grow", fids, ids, key, root, planes, side, side, F, RF.UNIT, max_rq, RF.GROW_BATCH, buf_a, buf_b,
                              gstats), a.reps)
        grown = None

        def whole_grow():
            nonlocal grown
            grown = RF.grow(fids, ids, key, table)
        out[f"{tag}_grow_wall_ms"] = wall_ms(whole_grow, a.reps)
        grown, gained, rounds = grown
        out[f"{tag}_grow_rounds"], out[f"{tag}_grown_cells"] = rounds, int(gained.sum())
        out[f"{tag}_cells_left_without_facet"] = int(((grown == 0) & (ids > 0)).sum())
        side_bits, _ = OL.sides(grown, F)
        offsets, E = OL.offsets_of(side_bits)
        slot, nxt, flags, _ = OL.link(grown, side_bits, offsets, F, 4, E)
        ring, rank, _, totals, _ = OL.rank_rings(nxt, flags)
        out[f"{tag}_edges"] = E
        node = torch.empty(E, dtype=torch.int32, device=dev)
        first_word = torch.full((E,), AR.NO_FIRST, dtype=torch.int32, device=dev)
        stats = torch.zeros(4, dtype=torch.int64, device=dev)
        out[f"{tag}_first_ms"] = window_ms(
            lambda: _lib.call("snerf_arcs_first", grown, slot, ring, rank, side, side, F, E, node, first_word, stats), a.reps)
        ring_row, ring_base, n_rings = AR.ring_base_of(ring, totals)
        bufs = tuple(torch.empty(E, dtype=torch.int32, device=dev) for _ in range(6))
        out[f"{tag}_mark_ms"] = window_ms(
            lambda: _lib.call("snerf_arcs_mark", grown, side_bits, offsets, slot, flags, ring, rank, totals, node, first_word, ring_row, ring_base,
                              side, side, F, E, n_rings, *bufs, stats), a.reps)
        left, twin, pos_of, order, hf, vf = bufs
        arc_of, ordinal, last, vertex_offset, A, V = AR.between(order, hf, vf, node)
        out[f"{tag}_rings"], out[f"{tag}_arcs"], out[f"{tag}_arc_vertices"] = n_rings, A, V
        vertices = torch.empty((V, 2), dtype=torch.int32, device=dev)
        rows = torch.zeros((A, AR.ROW_WORDS), dtype=torch.int64, device=dev)
        out[f"{tag}_fold_ms"] = window_ms(
            lambda: _lib.call("snerf_arcs_fold", grown, key, slot, ring, left, twin, pos_of, node, ring_row, order, hf, vf, arc_of, ordinal, last,
                              vertex_offset, side, side, E, A, n_rings, V, vertices, rows, stats), a.reps)
        result = None

        def whole_arcs():
            nonlocal result
            result = AR.arcs(grown, F, 4, key=key)
        out[f"{tag}_arcs_wall_ms"] = wall_ms(whole_arcs, a.reps)
        out[f"{tag}_arcs_with_twin"] = int((result["twin"] >= 0).sum())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
