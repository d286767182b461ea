"""The block-scaled fp16-plane format (csrc/bsp.h) and the element-wise bars of tests/test_gpu_bsp_exact.py, restated in
plain numpy fp64.  Nothing here imports the library: the code was read and written down again, so that a test can tell the
kernels' own error (fp32 accumulation, one output rounding) from the operand rounding the format imposes.

Format, as the kernels apply it:
  * activations (bsp_aux.hip: to_planes_kernel; bsp.h: split8 / cvt8, exp_of_maxbits): one exponent e per 128 x 128 block,
    blocks anchored at row 0 / column 0 of the SOURCE matrix, e = clamp(13 - (biased exponent of the block's |max| - 127),
    -E_MAX, E_QUIET), e = 0 for an all-zero or non-finite maximum; hi = f16(x 2^e) and, with two planes, lo = f16(x 2^e - hi).
    x 2^e is exact in fp32 (and fp64), the mixed-precision FMA rounds once, x 2^e - hi is exact in fp32 as well: one
    rounding per plane, to nearest-even, fp16 subnormals kept -- what numpy's float64 -> float16 conversion does.
  * weights (wmax_kernel / wpack_kernel): ONE exponent per matrix from its |max|, the same hi / lo rule.
  * from_planes_kernel: the fp32 sum hi + lo, then ldexp by -e, in fp32.
  * a consumer contracts hi hi + hi lo + lo hi (the lo lo term is dropped: bsp.h), one plane: hi hi alone."""
import numpy as np

RB = CB = 128
E_MAX, E_QUIET = 100, 60           # bsp.h
U = 2.0 ** -23                     # unit of acc_bound: see there
DW_DROP = 64                       # bsp_gemm.hip (gemm_dw_kernel: chunk()): a chunk with e_new - e_cur > 64 is dropped


def exp_of_max(m):
    """exp_of_maxbits: the exponent of a block whose |max| is m (max 2^e in [2^13, 2^14) unless clamped)"""
    m = abs(float(m))
    if m == 0.0 or not np.isfinite(m):
        return 0
    e = 13 - (int(np.frexp(m)[1]) - 1)
    return int(max(-E_MAX, min(E_QUIET, e)))


def _f16(x):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(x, np.float64).astype(np.float16).astype(np.float64)


def split(xs, planes):
    """xs = x 2^e (exact) -> hi, lo as fp64 arrays holding fp16 values (lo = 0 with one plane)"""
    hi = _f16(xs)
    if planes == 1:
        return hi, np.zeros_like(hi)
    with np.errstate(invalid="ignore"):
        return hi, _f16(xs - hi)


def block_exps(x):
    x = np.abs(np.asarray(x, np.float64))
    R, Cn = x.shape
    e = np.zeros(((R + RB - 1) // RB, (Cn + CB - 1) // CB), np.int64)
    for rb in range(e.shape[0]):
        for cb in range(e.shape[1]):
            e[rb, cb] = exp_of_max(x[RB * rb: RB * rb + RB, CB * cb: CB * cb + CB].max())
    return e


def expand(e, R, Cn):
    """block table -> one exponent per element"""
    return np.repeat(np.repeat(np.asarray(e), RB, 0), CB, 1)[:R, :Cn]


def to_planes(x, planes):
    """activation planes of an fp32 matrix: hi, lo (fp64 arrays of fp16 values times 2^e) and the block table e"""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 2
    e = block_exps(x)
    hi, lo = split(np.ldexp(x.astype(np.float64), expand(e, *x.shape)), planes)
    return hi, lo, e


def weight_planes(w, planes):
    w = np.asarray(w)
    assert w.dtype == np.float32
    e = exp_of_max(np.abs(w.astype(np.float64)).max())
    hi, lo = split(np.ldexp(w.astype(np.float64), e), planes)
    return hi, lo, e


def from_planes(hi, lo, e):
    """fp32 (hi + lo), then ldexp by -e in fp32; e: one int, or one per element"""
    s = hi.astype(np.float32) + lo.astype(np.float32)
    return np.ldexp(s, -np.asarray(e)).astype(np.float32)


def deq(hi, lo, e):
    """the two planes as fp64 values (exact): hi 2^-e, lo 2^-e"""
    return np.ldexp(hi, -np.asarray(e)), np.ldexp(lo, -np.asarray(e))


def exact_product(ah, al, bh, bl, planes):
    """What the matrix cores are asked to sum: (ah, al) [M][K] and (bh, bl) [K][N], dequantised planes.  One plane: sum ah bh; two:
    sum (ah bh + ah bl + al bh).  Returns the sum and `mag`, the same sum over absolute values.  fp64 matmuls: their own error,
    K 2^-53 mag, is 2^-30 of the bars below."""
    ex, mag = ah @ bh, np.abs(ah) @ np.abs(bh)
    if planes == 2:
        ex = ex + ah @ bl + al @ bh
        mag = mag + np.abs(ah) @ np.abs(bl) + np.abs(al) @ np.abs(bh)
    return ex, mag


def acc_bound(n_terms, mag):
    """Worst case of an fp32 sum of n_terms products in any order: (n_terms + 2) u mag.  u = 2^-23, not 2^-24: how the matrix
    cores round their internal adds is not documented, and 2^-23 also covers an accumulator that chops.  (Rescaling the
    accumulators by a power of two where the block exponent changes is exact.)  n_terms counts contraction indices: with two
    planes each index carries three products, two of them 2^-11 of the first."""
    return (n_terms + 2) * U * mag


def dw_drop_bound(esum):
    """gemm_dw_kernel leaves out a 128-point chunk whose exponent sum (dZ block + X block) is more than DW_DROP above the
    frame its accumulators are in (the first chunk's sum, then every sum that was not dropped).  esum: the sums of ONE
    split-K slab for one (row block, column block) pair, in order.  A plane value is at most 2^14 (+ 2^3 of lo), a product
    below 2^29 2^-esum, a chunk has 128 of them: what the rule can remove."""
    e_cur, lost = int(esum[0]), 0.0
    for e_new in esum[1:]:
        e_new = int(e_new)
        if e_new - e_cur > DW_DROP:
            lost += 128.0 * 2.0 ** (29 - e_new)
        else:
            e_cur = e_new
    return lost


def ulp16(y):
    """spacing of fp16 at |y| (subnormals: 2^-24)"""
    y = np.abs(np.asarray(y, np.float64))
    ex = np.frexp(y)[1]
    return np.where(y < 2.0 ** -14, 2.0 ** -24, np.ldexp(1.0, ex - 11))


def grid_spacing(v, planes):
    """spacing of the plane grid at the scaled value v = x 2^e: one plane ulp16(v); two planes ulp16 of the largest
    residual hi leaves, ulp16(v) / 2"""
    return ulp16(v) if planes == 1 else ulp16(0.5 * ulp16(v))


def _on_grid(v, planes):
    hi = _f16(v)
    if planes == 1:
        return hi == v
    r = v - hi
    return _f16(r) == r


def on_grid_near(got, exact, delta, planes, e_fixed=None, skip=None):
    """The check for an output that is itself stored as planes (blocks anchored at row 0 / column 0 of `got`).
      * every got element is a point of its block's grid: got 2^e is a sum of `planes` fp16 values;
      * every got element lies within half a grid spacing plus delta of the exact value (either neighbour passes where the
        exact value is within delta of a rounding tie).
    e: the kernel takes it from the block's |max| BEFORE rounding, which is within max(delta) of the exact |max| -- so e is
    exp_of_max of a value in [max - delta, max + delta]: one exponent, or two where that interval holds a power of two.  (The
    |max| of got itself would name the wrong binade where the maximum rounds up to 2^14.)  e_fixed: the producer writes a
    constant exponent (the sine epilogue: 13).  skip: elements left out of the nearness check (not of the grid check).
    Returns a dict: ok, bad_grid, bad_near, ratio = worst |got - exact| / (half spacing + delta), where (block, row, col)."""
    got = np.asarray(got, np.float64)
    exact = np.asarray(exact, np.float64)
    delta = np.broadcast_to(np.asarray(delta, np.float64), got.shape)
    R, Cn = got.shape
    out = {"ok": True, "bad_grid": 0, "bad_near": 0, "ratio": 0.0, "where": None}
    for rb in range((R + RB - 1) // RB):
        for cb in range((Cn + CB - 1) // CB):
            sl = (slice(RB * rb, RB * rb + RB), slice(CB * cb, CB * cb + CB))
            g, x, d = got[sl], exact[sl], delta[sl]
            if e_fixed is not None:
                cand = [int(e_fixed)]
            else:
                m, dm = np.abs(x).max(), d.max()
                cand = sorted({exp_of_max(max(m - dm, 0.0)), exp_of_max(m + dm)})
            best = None
            for e in cand:
                grid = _on_grid(np.ldexp(g, e), planes)
                bar = np.ldexp(0.5 * grid_spacing(np.ldexp(np.abs(x) + d, e), planes), -e) + d
                ratio = np.abs(g - x) / bar
                if skip is not None:
                    ratio = np.where(skip[sl], 0.0, ratio)
                res = (int((~grid).sum()), int((ratio > 1.0).sum()), float(ratio.max()), np.unravel_index(int(ratio.argmax()), ratio.shape))
                if best is None or (res[0] + res[1], res[2]) < (best[0] + best[1], best[2]):
                    best = res
            out["bad_grid"] += best[0]
            out["bad_near"] += best[1]
            if best[2] > out["ratio"]:
                out["ratio"], out["where"] = best[2], (rb, cb, int(best[3][0]), int(best[3][1]))
    out["ok"] = out["bad_grid"] == 0 and out["bad_near"] == 0
    return out
