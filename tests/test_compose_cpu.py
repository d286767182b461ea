"""feats_from_xyz composed into the fused first head layer: the algebra, in torch fp64 against autograd.

The library replaces  pre1 = W_h1 [W_f h + b_f | extras] + b_h1  by  pre1 = W_c [h | extras] + b_c  with
W_c = [A W_f | W_h1[:, W:]], b_c = b_h1 + A b_f, A = W_h1[:, :W] (csrc/api.hip: snerf_pack_params), and turns the gradient of the composed
layer (G_c, g_c) back into those of the two Linear layers (csrc/bsp_pass.hip: the un-compose launch):

    dW_h1[:, :W] = G_c[:, :W] W_f^T + g_c (x) b_f      dW_h1[:, W:] = G_c[:, W:]      db_h1 = g_c
    dW_f = A^T G_c[:, :W]                              db_f = A^T g_c

Both are exact in real arithmetic; here they hold to fp64 round-off, for the whole layer and for a row block of it (the solar-correction
pass runs the sun-visibility block alone, while the main pass contributes the gradient of every block)."""
import pytest
import torch

DT = torch.float64


def _problem(seed, P, W, X, N1):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=DT)
    return dict(W_f=r(W, W) / W ** 0.5, b_f=r(W), W_h1=r(N1, W + X) / (W + X) ** 0.5, b_h1=r(N1), h=r(P, W), extras=r(P, X), dz1=r(P, N1))


def _two_linear_grads(q, rows):
    """autograd through the two Linear layers, the first head layer restricted to `rows`; dz1 is the gradient of its pre-activation"""
    leaves = {k: q[k].clone().requires_grad_(True) for k in ("W_f", "b_f", "W_h1", "b_h1", "h")}
    feats = leaves["h"] @ leaves["W_f"].T + leaves["b_f"]
    pre1 = torch.cat([feats, q["extras"]], 1) @ leaves["W_h1"][rows].T + leaves["b_h1"][rows]
    pre1.backward(q["dz1"][:, rows])
    return pre1.detach(), {k: v.grad for k, v in leaves.items()}


def _composed(q, rows):
    W = q["W_f"].shape[0]
    A = q["W_h1"][rows, :W]
    W_c = torch.cat([A @ q["W_f"], q["W_h1"][rows, W:]], 1)
    b_c = q["b_h1"][rows] + A @ q["b_f"]
    x = torch.cat([q["h"], q["extras"]], 1)
    pre1 = x @ W_c.T + b_c
    dz1 = q["dz1"][:, rows]
    G_c, g_c = dz1.T @ x, dz1.sum(0)                       # the composed layer's own gradients: one dW launch, one column sum
    grads = {
        "W_h1": torch.zeros_like(q["W_h1"]), "b_h1": torch.zeros_like(q["b_h1"]),
        "W_f": A.T @ G_c[:, :W], "b_f": A.T @ g_c,
        "h": dz1 @ W_c[:, :W],                             # what the merged dX launch contracts (before the activation derivative)
    }
    grads["W_h1"][rows] = torch.cat([G_c[:, :W] @ q["W_f"].T + torch.outer(g_c, q["b_f"]), G_c[:, W:]], 1)
    grads["b_h1"][rows] = g_c
    return pre1, grads


def _close(a, b, what):
    scale = float(b.abs().max()) + 1e-300
    err = float((a - b).abs().max()) / scale
    assert err < 1e-12, (what, err)


@pytest.mark.parametrize("P,W,X,N1,rows", [
    (257, 64, 16, 96, slice(0, 96)),          # every block (main pass)
    (257, 64, 16, 96, slice(64, 96)),         # the last block alone (solar-correction pass: the sun-visibility rows)
    (100, 32, 112, 160, slice(0, 160)),       # extras block wider than the layer (pad columns between feats and extras)
    (64, 128, 16, 48, slice(16, 48)),
])
def test_compose_uncompose_match_autograd(P, W, X, N1, rows):
    q = _problem(1234 + W + N1, P, W, X, N1)
    pre_ref, g_ref = _two_linear_grads(q, rows)
    pre_c, g_c = _composed(q, rows)
    _close(pre_c, pre_ref, "pre-activation")
    for k in ("W_h1", "b_h1", "W_f", "b_f", "h"):
        _close(g_c[k], g_ref[k], k)
    # rows outside the block get no gradient from this pass
    mask = torch.ones(N1, dtype=torch.bool); mask[rows] = False
    assert float(g_ref["W_h1"][mask].abs().max() if mask.any() else 0.0) == 0.0


def test_bias_outer_product_term_is_needed():
    """Dropping g_c (x) b_f from dW_h1[:, :W] is visible: the term is not round-off."""
    q = _problem(7, 128, 64, 16, 96)
    rows = slice(0, 96)
    _, g_ref = _two_linear_grads(q, rows)
    _, g_c = _composed(q, rows)
    W = 64
    g_c_vec = q["dz1"].sum(0)
    without = g_c["W_h1"].clone()
    without[:, :W] -= torch.outer(g_c_vec, q["b_f"])
    assert float((without - g_ref["W_h1"]).abs().max()) > 1e-3 * float(g_ref["W_h1"].abs().max())


def test_two_passes_accumulate():
    """Main pass (all rows) and sc pass (the last block, its own dz1) add into the same gradients: un-composing each pass with its own
    G_c, g_c and summing equals autograd of the summed losses."""
    q = _problem(99, 96, 64, 16, 96)
    q2 = dict(q); q2["dz1"] = torch.randn(96, 96, generator=torch.Generator().manual_seed(5), dtype=DT)
    ra, rb = slice(0, 96), slice(64, 96)
    _, ga = _two_linear_grads(q, ra)
    _, gb = _two_linear_grads(q2, rb)
    _, ca = _composed(q, ra)
    _, cb = _composed(q2, rb)
    for k in ("W_h1", "b_h1", "W_f", "b_f"):
        _close(ca[k] + cb[k], ga[k] + gb[k], k)
