#!/usr/bin/env python3
"""Generate the golden vectors of the depth resampling by running the REFERENCE's own `sample_pdf`
(framework/components/rendering.py:8-51) on synthetic coarse depths and weights.

Run where the reference is (it never travels to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 SNERF_REFERENCE=<checkout of the reference> python tools/gen_golden_resample.py

Writes tests/golden/resample_<det|rand>_<N>x<S>x<Ni>.npz for (N, S, Ni) = (64, 64, 64), (16, 7, 5), (8, 130, 200):
  z        (N, S)  fp32  coarse depths, non-decreasing along a ray (jittered strata of a near-far interval)
  weights  (N, S)  fp32  the proposal pass's weights; sample_pdf sees the interior ones, weights[:, 1:-1]
  family   (N,)    uint8 0 = random positive, 1 = peaked (three neighbouring non-zero weights, exact zeros elsewhere: what a
                         surface gives), 2 = all zero
  u        (N, Ni) fp32  the uniforms (`rand` files only; a `det` file has none: det=True, torch.linspace(0, 1, Ni))
  ref64    (N, Ni) fp64  sample_pdf(bins, weights, Ni, det) under torch.set_default_dtype(torch.float64), with
                         bins = 0.5 * (z[:, :-1] + z[:, 1:]) formed in fp64 from the fp32 depths
  ref32    (N, Ni) fp32  the same call in the reference's everyday arithmetic: fp32 bins, fp32 weights, default dtype fp32
  seed                   the seed of the case

The uniforms: sample_pdf draws them itself (torch.rand(N, Ni)).  The library takes fp32 uniforms, so for the `rand` files
torch.rand is replaced for the length of the call by a function that hands out the case's fp32 uniforms (as fp64 under the fp64
default, exactly): both sides then see the same numbers.  Everything else of sample_pdf runs as it stands.

The sub-eps share: tests/test_resample_cpu.py compares a sample with ref64 to 1 fp32 ulp where the reference's pdf of its bin
is >= 2 eps, and only asks for the same bin below that (there the reference's `denom < eps` rule may pin the sample to the bin's
left edge, the library interpolates).  At most 5 % of a case's samples may fall under the second rule; this generator asserts
the share per case, draws the next seed where a case exceeds 3 %, and prints the shares (DESIGN.md section 5p records them)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("SNERF_REFERENCE", "/root/reference")
OUT = os.path.join(ROOT, "tests", "golden")
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)

from tests import resample_numpy as RN  # noqa: E402

sys.path.insert(0, REF)
from framework.components.rendering import sample_pdf  # noqa: E402

CASES = ((64, 64, 64), (16, 7, 5), (8, 130, 200))
EPS = 1e-5
SHARE_WANTED = 0.03


def synth(rng, N, S):
    near = rng.uniform(0.1, 2.0, (N, 1))
    far = near + rng.uniform(0.5, 4.0, (N, 1))
    strata = (np.arange(S)[None, :] + rng.random((N, S))) / S
    z = np.sort((near + (far - near) * strata).astype(np.float32), axis=1)
    family = (np.arange(N) * 3 // N).astype(np.uint8)
    w = np.zeros((N, S), np.float32)
    for n in range(N):
        if family[n] == 0:
            r = rng.random(S) ** 3
            w[n] = (r / r.sum() * rng.uniform(0.3, 1.0)).astype(np.float32)
        elif family[n] == 1:
            k0 = int(rng.integers(1, S - 3))                     # the first of three neighbouring interior samples
            p = rng.uniform(0.1, 1.0, 3)
            w[n, k0:k0 + 3] = (p / p.sum() * rng.uniform(0.2, 1.0)).astype(np.float32)
    return z, w, family


def run_reference(z, w, Ni, u):
    """-> (ref64, ref32); u = None: det=True"""
    real_rand = torch.rand
    out = []
    for dt in (torch.float64, torch.float32):
        torch.set_default_dtype(dt)
        try:
            zt = torch.from_numpy(z).to(dt)
            bins = 0.5 * (zt[:, :-1] + zt[:, 1:])
            wt = torch.from_numpy(w[:, 1:-1].copy()).to(dt)
            if u is not None:
                torch.rand = lambda *a, **k: torch.from_numpy(u).to(torch.get_default_dtype())
            out.append(sample_pdf(bins, wt, Ni, det=u is None).numpy())
        finally:
            torch.rand = real_rand
            torch.set_default_dtype(torch.float32)
    return out[0], out[1]


def sub_eps_share(w, Ni, u):
    """the share of the samples whose bin has a reference pdf below 2 eps (the rule tests/test_resample_cpu.py applies)"""
    wd = w[:, 1:-1].astype(np.float64) + EPS
    pdf = wd / wd.sum(1, keepdims=True)
    cdf = np.concatenate([np.zeros((w.shape[0], 1)), np.cumsum(pdf, 1)], 1)
    ud = np.broadcast_to(np.linspace(0.0, 1.0, Ni), (w.shape[0], Ni)) if u is None else u.astype(np.float64)
    k = np.stack([np.clip(np.searchsorted(cdf[n], ud[n], side="right") - 1, 0, pdf.shape[1] - 1) for n in range(w.shape[0])])
    return float((np.take_along_axis(pdf, k, 1) < 2 * EPS).mean())


def main():
    os.makedirs(OUT, exist_ok=True)
    total = 0
    for N, S, Ni in CASES:
        for det in (True, False):
            seed = 1000 * S + Ni + (0 if det else 500000)
            while True:
                rng = np.random.default_rng(seed)
                z, w, family = synth(rng, N, S)
                u = None if det else torch.rand(N, Ni, generator=torch.Generator().manual_seed(seed), dtype=torch.float32).numpy()
                share = sub_eps_share(w, Ni, u)
                if share <= SHARE_WANTED:
                    break
                seed += 1
            ref64, ref32 = run_reference(z, w, Ni, u)
            assert ref64.dtype == np.float64 and ref32.dtype == np.float32 and ref64.shape == (N, Ni)
            ours = RN.fine_samples(z, w, Ni, u)
            ulp32 = np.abs(ref32.astype(np.float64) - ref64) / np.spacing(np.abs(ref64).astype(np.float32)).astype(np.float64)
            ulp_ours = np.abs(ours.astype(np.float64) - ref64) / np.spacing(np.abs(ref64).astype(np.float32)).astype(np.float64)
            name = f"resample_{'det' if det else 'rand'}_{N}x{S}x{Ni}.npz"
            arrays = {"z": z, "weights": w, "family": family, "ref64": ref64, "ref32": ref32, "seed": np.int64(seed)}
            if u is not None:
                arrays["u"] = u
            np.savez_compressed(os.path.join(OUT, name), **arrays)
            size = os.path.getsize(os.path.join(OUT, name))
            total += size
            print(f"{name}: seed {seed}, sub-eps share {100 * share:.2f} %, reference fp32 vs its fp64: max {ulp32.max():.1f} ulp, "
                  f"restatement vs reference fp64: max {ulp_ours.max():.3f} ulp (median {np.median(ulp_ours):.3f}), {size} bytes")
    print(f"total {total} bytes")


if __name__ == "__main__":
    main()
