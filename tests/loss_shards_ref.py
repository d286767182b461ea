"""Shard-invariance of the two-phase loss: the seeded cases, the shard splits and the fp64 reference that
tests/test_loss_shards_cpu.py (no GPU) and tests/test_gpu_loss_shards.py share.  Nothing here touches the HIP library.

A "shard" is a contiguous slice [lo, hi) of the rays of one batch (parallel.frame_shard, GpuRayBank.batch): what one rank of a
data-parallel step renders and hands to snerf_loss_partial.  Some shards of every case are doctored so that they could never
have run alone -- no ray that counts for the cross-entropy, or no car ray for L_t: both means are 0 / 0 on such a shard and
must come out finite and exact once the 16 totals are summed over the shards."""
import dataclasses
import functools

import torch

from oracle import snerf_oracle as O
from snerf_amd.loss_ops import LossSpec

CAR = 4          # OracleCfg.car_index / LossSpec.car_label
TERM_BAR = 1e-5  # |term - oracle| <= TERM_BAR * max(1, |oracle|): tests/test_gpu_pipeline.py _loss_modules_vs_oracle
GRAD_BAR = 2e-5  # rel_err of a gradient against the oracle's: same place

RENDERED = ("rgb", "weights", "beta", "beta_semantic", "semantic_logits", "sun_sc", "depth")   # loss_ops._DIFF


def equal_bounds(n, world):
    assert n % world == 0
    return [(r * (n // world), (r + 1) * (n // world)) for r in range(world)]


def size_bounds(sizes):
    out, lo = [], 0
    for s in sizes:
        out.append((lo, lo + s))
        lo += s
    return out


def frame_bounds(n, world):
    """parallel.frame_shard(n, r, world) for every r, restated: ceil(n / world) rays per rank, the ragged tail (possibly nothing) last"""
    per = -(-n // world)
    return [(min(r * per, n), min(r * per + per, n)) for r in range(world)]


# (N, S, C, bounds): the shapes and splits of the GPU test, in its order
ROWS = (
    (616, 16, 5, equal_bounds(616, 8)),       # ragged against the 4-ray workgroups; reduce_cols
    (616, 100, 64, equal_bounds(616, 8)),     # S no multiple of 64; every lane of the logit gradient
    (72, 64, 16, equal_bounds(72, 8)),        # every shard <= 64 partial rows: reduce_rows
    (613, 64, 5, frame_bounds(613, 8)),       # 7 x 77 + 74: unequal shards
    (9, 16, 5, frame_bounds(9, 8)),           # 2, 2, 2, 2, 1, 0, 0, 0: one-ray and empty shards
    (616, 64, 5, size_bounds([1, 615])),      # grossly unequal
    (1040, 16, 5, size_bounds([1025, 15])),   # one shard past the 1024 waves of loss_blocks: the ray loop strides
)
SEED = 2024
MODULE_SPECS = ("snerf", "snerf_nosc", "satnerf", "depth_w", "depth_1", "sem_ign", "sem_nomask", "semunc", "semunc_detach",
                "semunc_sbeta", "car")


def _rand_results(N, S, C, seed):
    """the rendered tensors of tests/test_gpu_pipeline.py _rand_results, beta_semantic_coarse included"""
    g = torch.Generator().manual_seed(seed)
    return {"rgb_coarse": torch.rand(N, 3, generator=g), "weights_coarse": torch.rand(N, S, generator=g) * 0.1,
            "beta_coarse": torch.rand(N, S, 1, generator=g) + 0.01, "semantic_logits_coarse": torch.rand(N, C, generator=g) * 3,
            "depth_coarse": torch.rand(N, generator=g), "sun_sc_coarse": torch.rand(N, S, 1, generator=g),
            "transparency_sc_coarse": torch.rand(N, S, generator=g), "weights_sc_coarse": torch.rand(N, S, generator=g) * 0.1,
            "beta_semantic_coarse": torch.rand(N, S, 1, generator=g) + 0.01}


def build_case(N, S, C, bounds, seed):
    """-> {"results", "gt", "labels" (N, 1) int64, "mask" (N,) bool, "depth_gt", "depth_w", "bounds", "N", "S", "C"}, CPU fp32.
    Doctored, where the split has that shard: shard 0 all car and unmasked (no CE-valid ray under ignore_car_index), shard 2 all
    masked out (nothing valid, no car), shard 5 without a car ray (label 4 -> 0), the first ray of shard 1 a car ray."""
    g = torch.Generator().manual_seed(seed + 1)
    gt = torch.rand(N, 3, generator=g)
    labels = torch.randint(0, C, (N, 1), generator=g)
    mask = torch.rand(N, generator=g) > 0.3
    depth_gt, depth_w = torch.rand(N, generator=g), torch.rand(N, generator=g)
    if C != 5:   # car rays on every draw (tests/test_gpu_pipeline.py _loss_modules_vs_oracle)
        labels[::6] = CAR

    def shard(k):
        return bounds[k] if k < len(bounds) else (0, 0)
    lo, hi = shard(0)
    labels[lo:hi] = CAR
    mask[lo:hi] = True
    lo, hi = shard(2)
    mask[lo:hi] = False
    lo, hi = shard(5)
    labels[lo:hi] = torch.where(labels[lo:hi] == CAR, torch.zeros_like(labels[lo:hi]), labels[lo:hi])
    lo, hi = shard(1)
    if hi > lo:
        labels[lo] = CAR
        mask[lo] = True
    return {"results": _rand_results(N, S, C, seed), "gt": gt, "labels": labels, "mask": mask, "depth_gt": depth_gt,
            "depth_w": depth_w, "bounds": list(bounds), "N": N, "S": S, "C": C}


@functools.lru_cache(maxsize=None)
def row_case(i):
    N, S, C, bounds = ROWS[i]
    return build_case(N, S, C, bounds, SEED + i)


def shard_counts(case, ignore_index=CAR):
    """per shard: (rays that count for the CE, car rays of L_t)"""
    y, m = case["labels"][:, 0], case["mask"]
    return [(int((m[lo:hi] & (y[lo:hi] != ignore_index)).sum()), int((m[lo:hi] & (y[lo:hi] == CAR)).sum())) for lo, hi in case["bounds"]]


def spec_for(name, n_classes=5):
    """-> (LossSpec, OracleCfg kwargs) of the eleven cases of _loss_modules_vs_oracle, or of "everything".  Keys of the kwargs that
    start with "_" are for oracle_fp64, not for OracleCfg: _fns (which oracle losses make up the case), _mask / _depth_w (False:
    the case passes no mask / the scalar weight 1)."""
    sem = dict(lambda_s=0.04, n_classes=n_classes)
    table = {
        "snerf": (LossSpec(color_mode=1, has_sc=True, sc_lambda=0.05), {"_fns": ("snerf",)}),
        "snerf_nosc": (LossSpec(color_mode=1), {"sc_lambda": 0.0, "_fns": ("snerf",)}),
        "satnerf": (LossSpec(color_mode=2, has_sc=True, sc_lambda=0.05), {"_fns": ("satnerf",)}),
        "depth_w": (LossSpec(has_depth=True, ds_lambda=1000.0), {"_fns": ("depth",)}),
        "depth_1": (LossSpec(has_depth=True, ds_lambda=1000.0), {"_fns": ("depth",), "_depth_w": False}),
        "sem_ign": (LossSpec(sem_mode=1, ignore_index=CAR, **sem), {"ignore_car_index": True, "_fns": ("sem",)}),
        "sem_nomask": (LossSpec(sem_mode=1, **sem), {"ignore_car_index": False, "_fns": ("sem",), "_mask": False}),
        "semunc": (LossSpec(sem_mode=2, ignore_index=CAR, **sem), {"ignore_car_index": True, "_fns": ("semunc",)}),
        "semunc_detach": (LossSpec(sem_mode=2, ignore_index=CAR, detach_beta_for_s=True, **sem),
                          {"ignore_car_index": True, "detach_beta_for_s": True, "_fns": ("semunc",)}),
        "semunc_sbeta": (LossSpec(sem_mode=2, ignore_index=CAR, use_sbeta=True, **sem), {"ignore_car_index": True, "_fns": ("semunc",)}),
        "car": (LossSpec(car_reg=True, car_label=CAR, lambda_c=0.1), {"lambda_c": 0.1, "_fns": ("car",)}),
        # every term on: SatNerfLoss + solar correction, beta-weighted CE with its own beta head, L_t, weighted depth
        "everything": (LossSpec(color_mode=2, has_sc=True, sc_lambda=0.05, sem_mode=2, ignore_index=CAR, use_sbeta=True,
                                car_reg=True, car_label=CAR, lambda_c=0.1, has_depth=True, ds_lambda=1000.0, **sem),
                       {"ignore_car_index": True, "lambda_c": 0.1, "_fns": ("satnerf", "semunc", "car", "depth")}),
    }
    return table[name]


def without_depth(pair):
    """the training step's three merged modules (colour, semantic, L_t): "everything" less the depth term"""
    spec, kw = pair
    return dataclasses.replace(spec, has_depth=False, ds_lambda=0.0), dict(kw, _fns=tuple(f for f in kw["_fns"] if f != "depth"))


def _loss_dict(res, case, pair, sl=slice(None)):
    """the oracle's loss_dict of the case's modules on the rays `sl` of `res`"""
    spec, kw = pair
    cfg = O.OracleCfg(n_samples=case["S"], **{k: v for k, v in kw.items() if not k.startswith("_")})
    dt = res["rgb_coarse"].dtype
    r = {k: v[sl] for k, v in res.items() if k != "beta_semantic_coarse" or spec.use_sbeta}
    labels = case["labels"][sl]
    mask = case["mask"][sl] if kw.get("_mask", True) else None
    d = {}
    for fn in kw["_fns"]:
        if fn == "snerf":
            d.update(O.snerf_loss(r, case["gt"][sl].to(dt), cfg))
        elif fn == "satnerf":
            d.update(O.satnerf_loss(r, case["gt"][sl].to(dt), cfg))
        elif fn == "depth":
            d.update(O.depth_loss(r, case["depth_gt"][sl].to(dt), case["depth_w"][sl].to(dt) if kw.get("_depth_w", True) else 1.0, cfg))
        elif fn == "sem":
            d.update(O.semantic_loss(r, labels, mask, cfg))
        elif fn == "semunc":
            d.update(O.semantic_uncertainty_loss(r, labels, mask, cfg))
        elif fn == "car":
            d.update(O.car_reg_loss(r, labels, mask, cfg))
    return d


def _leaves(case, dtype):
    return {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in case["results"].items()}


def _grads(leaves):
    """{rendered tensor: (N, -1) gradient, zeros where the loss does not reach it}; the two detached sc inputs are not outputs"""
    out = {}
    for k in RENDERED:
        v = leaves[k + "_coarse"]
        out[k] = (v.grad if v.grad is not None else torch.zeros_like(v)).detach().reshape(v.shape[0], -1)
    return out


def oracle_fp64(case, pair, dtype=torch.float64):
    """loss_dict ({key: float}) and d O.total_loss / d rendered tensor ({name: (N, -1) tensor}) on the union batch, from the
    loss functions of oracle/snerf_oracle.py on `dtype` copies"""
    leaves = _leaves(case, dtype)
    d = _loss_dict(leaves, case, pair)
    O.total_loss(d).backward()
    return {k: float(v.detach()) for k, v in d.items()}, _grads(leaves)


def oracle_sharded_fp64(case, pair):
    """The same, shard by shard: every mean of the oracle on a shard is turned back into its numerator (mean x count; 0 where the
    count is 0), numerators and counts are summed over the shards and divided once.  Returns what oracle_fp64 returns.  The
    per-ray factor 1 / (2 beta^2) of the beta-weighted CE is a mean of its own (over all rays, not over the CE-valid ones): on a
    shard it is the oracle's uncertainty loss over its plain CE loss with every ray made valid (label 0, no mask, no ignore)."""
    spec, kw = pair
    leaves = _leaves(case, torch.float64)
    y, m = case["labels"][:, 0], (case["mask"] if kw.get("_mask", True) else torch.ones(case["N"], dtype=torch.bool))
    num, den = {}, {}

    def add(key, numerator, count):
        num[key] = num.get(key, 0.0) + numerator
        den[key] = den.get(key, 0) + count
    for lo, hi in case["bounds"]:
        n = hi - lo
        if n == 0:
            continue
        sl = slice(lo, hi)
        d = _loss_dict(leaves, case, pair, sl)
        # (the two log-beta terms are affine in a mean over all rays: the ray-weighted mean of the shards' values is the union's)
        for k in ("coarse_color", "coarse_logbeta", "coarse_sc_term2", "coarse_sc_term3", "coarse_ds", "coarse_semantic_logbeta"):
            if k in d:
                add(k, d[k] * n, n)
        n_ce = int((m[sl] & (y[sl] != spec.ignore_index)).sum())
        n_car = int((m[sl] & (y[sl] == CAR)).sum())
        if "coarse_car_reg_loss" in d:
            add("coarse_car_reg_loss", d["coarse_car_reg_loss"] * n_car if n_car else 0.0, n_car)
        if spec.sem_mode:
            ce_pair = (dataclasses.replace(spec, sem_mode=1), dict(kw, _fns=("sem",)))
            add("ce", _loss_dict(leaves, case, ce_pair, sl)["coarse_semantic"] * n_ce if n_ce else 0.0, n_ce)
        if spec.sem_mode == 2:
            every = dict(case, labels=torch.zeros_like(case["labels"]))
            okw = dict(kw, ignore_car_index=False, _mask=False)
            unc = _loss_dict(leaves, every, (spec, dict(okw, _fns=("semunc",))), sl)["coarse_semantic"]
            ce = _loss_dict(leaves, every, (spec, dict(okw, _fns=("sem",))), sl)["coarse_semantic"]
            add("invb", unc / ce * n, n)
    out = {k: num[k] / den[k] for k in num if k not in ("ce", "invb")}
    if spec.sem_mode == 1:
        out["coarse_semantic"] = num["ce"] / den["ce"]
    if spec.sem_mode == 2:
        out["coarse_semantic"] = num["ce"] / den["ce"] * (num["invb"] / den["invb"])
    O.total_loss(out).backward()
    return {k: float(v.detach()) for k, v in out.items()}, _grads(leaves)
