"""The summation order of csrc/reduce.h restated in numpy (tests only), vectorised over threads and workgroups: every fp64
addition the kernels make is one fp64 numpy addition here, in the same order, so the results are equal bit for bit.  The order
(DESIGN.md section 5k): per thread ascending, then the strided sum of the per-workgroup partials, then the tree, then the serial
sum over the workgroups where a kernel has one."""
import numpy as np


def blocks_for(n, threads, cap):
    """ceil(n / threads) in [1, cap]"""
    return max(1, min(cap, -(-n // threads)))


def tree(a):
    """block_tree with OpSum over the last axis (T threads, a power of two): levels o = T/2 ... 1, a[t] += a[t + o] for t < o"""
    a = np.array(a, np.float64)
    o = a.shape[-1] // 2
    while o:
        a[..., :o] = a[..., :o] + a[..., o:2 * o]
        o //= 2
    return a[..., 0]


def strided_sum(p, threads=256):
    """block_strided_sum: thread t adds p[t], p[t + T], ... in ascending order from 0.0, then the tree"""
    p = np.asarray(p, np.float64)
    steps = -(-p.shape[0] // threads)
    padded = np.zeros(steps * threads)
    padded[:p.shape[0]] = p
    ok = np.arange(steps * threads) < p.shape[0]
    a = np.zeros(threads)
    for s in range(steps):
        sl = slice(s * threads, (s + 1) * threads)
        a = np.where(ok[sl], a + padded[sl], a)
    return tree(a)


def grid_stride_sums(x, ok, grid, threads=256):
    """(grid, T) per-thread sums of a grid-stride loop over the items x: thread t of workgroup b adds x[p] at
    p = b * T + t, + grid * T, ... in ascending order from 0.0, where ok[p]"""
    x, ok = np.asarray(x, np.float64).reshape(-1), np.asarray(ok, bool).reshape(-1)
    span = grid * threads
    steps = -(-x.shape[0] // span)
    xp, okp = np.zeros(steps * span), np.zeros(steps * span, bool)
    xp[:x.shape[0]], okp[:x.shape[0]] = x, ok
    a = np.zeros((grid, threads))
    for s in range(steps):
        sl = slice(s * span, (s + 1) * span)
        a = np.where(okp[sl].reshape(grid, threads), a + xp[sl].reshape(grid, threads), a)
    return a


def serial_sum(p):
    """one thread, ascending, from 0.0"""
    s = np.float64(0.0)
    for v in np.asarray(p, np.float64):
        s = s + v
    return float(s)
