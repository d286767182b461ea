#!/usr/bin/env python3
"""The solar kernels (snerf_amd eval/utils/solar.py, csrc/solar.hip) on the synthetic towns of tools/roofs_timing.py: --sides^2 cells
at 0.5 m.  Nothing outside the repository is read; the measurement needs a GPU and has no fallback.

Prints one JSON line.  Per side, each figure the device time per call over an event-bracketed window of back-to-back calls after a
warm-up call: --reps calls of the horizon, the year and the cast shadows, --fast-reps calls of the entries that take a fraction of a
millisecond:
    horizon_d64_ms, horizon_d64_100m_ms   snerf_solar_horizon at D = 64 over the whole raster and under max_dist = 100 m
    svf_d64_ms                            snerf_solar_svf on those planes
    irradiate_64_ms                       snerf_solar_irradiate under 64 suns, with slopes
    irradiate_year_ms, year_suns          irradiate() over the suns of sun_path (hourly, every day, above 5 degrees): its calls of 64
    cast_64_ms                            snerf_shadow_cast under the same 64 suns
    break_even_suns                       the sun count at which the horizon map is the cheaper way to the lit masks:
                                          horizon_d64_ms / (cast_64_ms - irradiate_64_ms) * 64
and, on the smallest side only, "disagree_d{16,64,256}": the share of (cell, sun) pairs where the horizon interpolated between the
sectors decides otherwise than cast_shadows, over 64 suns of the year placed between the sectors -- a record, without a bar."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from _timing import warm_window_ms as window_ms  # noqa: E402
from roofs_timing import RES, town  # noqa: E402
from snerf_amd.eval.utils import shadow as S  # noqa: E402
from snerf_amd.eval.utils import solar as SO  # noqa: E402

LAT, LON, YEAR = 30.3, -81.7, 2021


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sides", type=int, nargs="+", default=[1024, 2048])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fast-reps", type=int, default=200)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("solar_timing: no GPU (there is no fallback: a CPU run measures nothing)")
    dev = torch.device("cuda:0")
    year, hours = SO.sun_path(LAT, LON, YEAR)
    pick = np.linspace(0, len(year) - 1, 64).astype(int)          # 64 suns spread over the year: low and high, every azimuth it has
    suns64 = year[pick]
    out = {"year_suns": len(year)}
    for side in sorted(a.sides):
        tag = f"s{side}"
        alt = torch.from_numpy(town(side)[0]).to(dev)
        rng = np.random.default_rng(side)
        se, sn = (torch.from_numpy(rng.uniform(-0.5, 0.5, (side, side)).astype(np.float32)).to(dev) for _ in range(2))
        hor = None

        def run_horizon(max_dist_m):
            nonlocal hor
            hor = SO.horizon(alt, RES, 64, max_dist_m=max_dist_m, z_top=z_top)
        z_top = float(alt.max())                                  # read once: the timed calls make no host read
        out[f"{tag}_horizon_d64_100m_ms"] = window_ms(lambda: run_horizon(100.0), a.reps)
        out[f"{tag}_horizon_d64_ms"] = window_ms(lambda: run_horizon(None), a.reps)
        out[f"{tag}_svf_d64_ms"] = window_ms(lambda: SO.sky_view(hor, RES), a.fast_reps)
        table64 = SO.sun_table(suns64, np.ones(64), 64, RES)
        table_year = SO.sun_table(year, hours, 64, RES)
        direct = torch.zeros((side, side), dtype=torch.float64, device=dev)
        count = torch.zeros((side, side), dtype=torch.int32, device=dev)
        out[f"{tag}_irradiate_64_ms"] = window_ms(lambda: SO.irradiate_rows(hor, table64, se, sn, direct, count), a.fast_reps)
        out[f"{tag}_irradiate_year_ms"] = window_ms(lambda: SO.irradiate_rows(hor, table_year, se, sn, direct, count), a.reps)
        rows64 = S.sun_rows(suns64, RES)
        out[f"{tag}_cast_64_ms"] = window_ms(lambda: S.cast_rows(alt, rows64, 0.0, z_top), a.reps)
        saved = out[f"{tag}_cast_64_ms"] - out[f"{tag}_irradiate_64_ms"]
        out[f"{tag}_break_even_suns"] = out[f"{tag}_horizon_d64_ms"] / saved * 64 if saved > 0 else None
        if side != min(a.sides):
            continue
        lit = S.cast_rows(alt, rows64, 0.0, z_top)
        known = lit[0] != S.UNKNOWN
        for D in (16, 64, 256):
            planes = SO.horizon(alt, RES, D, z_top=z_top)
            table = SO.sun_table(suns64, np.ones(64), D, RES)
            differ = 0
            for k in range(64):
                _, c = SO.irradiate_rows(planes, table[k:k + 1])
                differ += int(((c == 1) != (lit[k] == 1))[known].sum())
            out[f"{tag}_disagree_d{D}"] = differ / (64 * int(known.sum()))
            out[f"{tag}_between_sectors_d{D}"] = int((table[:, 1] != 0.0).sum())
            del planes
    print(json.dumps(out))


if __name__ == "__main__":
    main()
