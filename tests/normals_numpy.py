"""The two kernels of csrc/normals.hip restated in numpy, operation for operation (include/snerf_normals.h states the order;
DESIGN.md section 5za).  tests/test_normals_cpu.py checks the restatement against torch.autograd in fp64; tests/test_gpu_normals.py
checks the kernels against the restatement bit for bit.

Every operation is an IEEE fp64 operation rounded on its own.  The product of two fp32 values is exact in fp64 (48 significant
bits), so `acc + d * w` below rounds once, as the kernel's fused multiply-add does."""
import numpy as np


def encoding_gradient(dz, w_enc, enc, n_freq):
    """One layer that reads the encoding.  dz (P, W) and w_enc (W, >= E), E = 6 n_freq or 3: the layer's d(pre-activation) and its
    weight columns on the encoding; enc (P, >= E): the encoding, column 6 k + c = sin(2^k x_c), 6 k + 3 + c = cos(2^k x_c) (unused
    for the identity encoding, n_freq = 0).  Returns q (P, 3) fp64:
        T[e] = sum over j = 0 .. W - 1 ascending of dz[p][j] * w[j][e], one accumulator from 0.0
        n_freq > 0: q[c] = 0.0; k ascending: q[c] = q[c] + ((T[6k+c] * enc[6k+3+c]) - (T[6k+3+c] * enc[6k+c])) * 2^k
        n_freq = 0: q[c] = T[c]"""
    dz = np.asarray(dz, dtype=np.float64)
    w = np.asarray(w_enc, dtype=np.float64)
    P, W = dz.shape
    E = 6 * n_freq if n_freq > 0 else 3
    T = np.zeros((P, E), dtype=np.float64)
    for j in range(W):                                   # one addition per j: the order of the kernel's accumulator
        T = T + dz[:, j:j + 1] * w[j:j + 1, :E]
    if n_freq == 0:
        return T[:, :3].copy()
    enc = np.asarray(enc, dtype=np.float64)
    q = np.zeros((P, 3), dtype=np.float64)
    for k in range(n_freq):
        ta = T[:, 6 * k:6 * k + 3] * enc[:, 6 * k + 3:6 * k + 6]
        tb = T[:, 6 * k + 3:6 * k + 6] * enc[:, 6 * k:6 * k + 3]
        q = q + (ta - tb) * float(2 ** k)
    return q


def point_gradient(dz_layers, w_layers, enc, n_freq):
    """G (P, 3): the layers that read the encoding in the pass's launch order (skip layers descending, then layer 0): the first
    stores, each later one adds: G = G + q."""
    G = None
    for dz, w in zip(dz_layers, w_layers):
        q = encoding_gradient(dz, w, enc, n_freq)
        G = q if G is None else G + q
    return G


def ray_fold(G, n_rays, n_samples):
    """grad_ray (N, 3) fp64 = 0.0 + G[n S] + G[n S + 1] + ... in that order; grad_sample (N, S, 3) = (float)G."""
    G = np.asarray(G, dtype=np.float64).reshape(n_rays, n_samples, 3)
    acc = np.zeros((n_rays, 3), dtype=np.float64)
    for s in range(n_samples):
        acc = acc + G[:, s, :]
    return acc, G.astype(np.float32)
