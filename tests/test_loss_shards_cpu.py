"""The construction behind tests/test_gpu_loss_shards.py, checked without a GPU: the doctored shards are what they claim to be, the
fp64 reference is finite on every split, the fp32 oracle sits inside the bars the kernels are held to, and "summing numerators and
denominators over the shards" -- what the all-reduce of the 16 totals does -- reproduces the union evaluation in fp64."""
import pytest
import torch

from tests import loss_shards_ref as R
from tests.helpers import rel_err


def test_splits_are_the_ones_the_ranks_take():
    from snerf_amd import parallel
    for n, world in ((613, 8), (9, 8), (616, 8), (1001, 8), (1, 8)):
        assert R.frame_bounds(n, world) == [parallel.frame_shard(n, r, world) for r in range(world)]
    assert [hi - lo for lo, hi in R.ROWS[3][3]] == [77] * 7 + [74]
    assert [hi - lo for lo, hi in R.ROWS[4][3]] == [2, 2, 2, 2, 1, 0, 0, 0]
    for N, _, _, bounds in R.ROWS:
        assert bounds[0][0] == 0 and bounds[-1][1] == N and all(a[1] == b[0] for a, b in zip(bounds, bounds[1:]))


@pytest.mark.parametrize("row", range(len(R.ROWS)))
def test_doctored_counts(row):
    case = R.row_case(row)
    y, m, b = case["labels"][:, 0], case["mask"], case["bounds"]
    counts = R.shard_counts(case)
    lo, hi = b[0]
    assert bool((y[lo:hi] == R.CAR).all()) and bool(m[lo:hi].all()) and counts[0] == (0, hi - lo)    # all car: no CE-valid ray
    lo, hi = b[1]
    assert int(y[lo]) == R.CAR and bool(m[lo]) and counts[1][1] >= 1                                  # its first ray is a car ray
    if len(b) > 2:
        lo, hi = b[2]
        assert not bool(m[lo:hi].any()) and counts[2] == (0, 0)                                       # nothing valid, no car
    if len(b) > 5:
        lo, hi = b[5]
        assert not bool((y[lo:hi] == R.CAR).any()) and counts[5][1] == 0                              # no car ray
    assert sum(c[0] for c in counts) > 0                       # the union has rays that count for the CE ...
    assert sum(c[1] for c in counts[1:]) > 0                   # ... and car rays outside shard 0
    if row < 3:   # eight shards of equal size: every shard the list does not doctor away could have run alone
        assert all(c[0] > 0 for k, c in enumerate(counts) if k not in (0, 2))
        assert all(c[1] > 0 for k, c in enumerate(counts) if k not in (2, 5))


def _specs(row):
    return ("everything",) + (R.MODULE_SPECS if row < 3 else ())


@pytest.mark.parametrize("row", range(len(R.ROWS)))
def test_reference_is_finite_and_fp32_oracle_is_inside_the_bars(row):
    case = R.row_case(row)
    worst_v = worst_g = 0.0
    for name in _specs(row):
        pair = R.spec_for(name, case["C"])
        ld64, g64 = R.oracle_fp64(case, pair)
        ld32, g32 = R.oracle_fp64(case, pair, dtype=torch.float32)
        assert set(ld64) == set(ld32) and ld64
        for k, v in ld64.items():
            assert v == v and abs(v) != float("inf"), (name, k, v)
            assert abs(ld32[k] - v) <= R.TERM_BAR * max(1.0, abs(v)), (name, k, ld32[k], v)
            worst_v = max(worst_v, abs(ld32[k] - v) / max(abs(v), 1e-300))
        for k in R.RENDERED:
            assert bool(torch.isfinite(g64[k]).all()), (name, k)
            if float(g64[k].abs().max()) == 0.0:
                assert float(g32[k].abs().max()) == 0.0, (name, k)
                continue
            e = rel_err(g32[k], g64[k])
            assert e <= R.GRAD_BAR, (name, k, e)
            worst_g = max(worst_g, e)
    print(f"row {row}: fp32 oracle vs fp64: values {worst_v:.2e} relative, gradients {worst_g:.2e} relative L2")


@pytest.mark.parametrize("row", range(len(R.ROWS)))
def test_summed_numerators_and_denominators_equal_the_union(row):
    case = R.row_case(row)
    for name in _specs(row):
        pair = R.spec_for(name, case["C"])
        ld_u, g_u = R.oracle_fp64(case, pair)
        ld_s, g_s = R.oracle_sharded_fp64(case, pair)
        assert set(ld_u) == set(ld_s)
        for k, v in ld_u.items():
            assert abs(ld_s[k] - v) <= 1e-12 * max(1.0, abs(v)), (name, k, ld_s[k], v)
        for k in R.RENDERED:
            assert rel_err(g_s[k], g_u[k]) <= 1e-12, (name, k, rel_err(g_s[k], g_u[k]))


@pytest.mark.parametrize("row", range(3))
def test_a_shard_on_its_own_is_far_from_the_union(row):
    """what the GPU test's control relies on: with "everything", shard 0 alone has no CE mean (NaN) and shard 1 alone an L_t more than
    100 bars away from the union's"""
    case = R.row_case(row)
    pair = R.spec_for("everything", case["C"])
    union, _ = R.oracle_fp64(case, pair)
    alone = []
    for lo, hi in case["bounds"][:2]:
        one = dict(case, bounds=[(0, hi - lo)], N=hi - lo, results={k: v[lo:hi] for k, v in case["results"].items()},
                   **{k: case[k][lo:hi] for k in ("gt", "labels", "mask", "depth_gt", "depth_w")})
        alone.append(R.oracle_fp64(one, pair)[0])
    assert alone[0]["coarse_semantic"] != alone[0]["coarse_semantic"]
    v = union["coarse_car_reg_loss"]
    assert abs(alone[1]["coarse_car_reg_loss"] - v) > 100 * R.TERM_BAR * max(1.0, abs(v)), (alone[1]["coarse_car_reg_loss"], v)
