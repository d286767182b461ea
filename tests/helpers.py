"""Shared helpers for the parity tests (fixtures -> oracle config / tensors)."""
import json
import os

import numpy as np
import torch

from oracle import snerf_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_fixture(name):
    z = np.load(os.path.join(GOLDEN, f"{name}.npz"), allow_pickle=False)
    meta = json.loads(str(z["meta_json"]))
    c = dict(meta["cfg"])
    c["fc_skips"] = tuple(c["fc_skips"])
    cfg = O.OracleCfg(**c)
    return z, meta, cfg


def fixture_params(z, meta, cfg):
    """Parameters regenerate from (cfg, seed); small fixtures also store them, which pins the generator."""
    params = O.init_params_numpy(cfg, meta["seed"])
    for k, v in meta.get("param_edit", {}).items():   # shifted biases (tools/gen_golden.py: edited_params)
        params[k] = (params[k] + np.asarray(v, dtype=np.float32)).astype(np.float32)
    stored = [k for k in z.files if k.startswith("param_")]
    for k in stored:
        assert np.array_equal(z[k], params[k[len("param_"):]]), k
    return params


def fixture_batch(z, prefix="in_"):
    """Main batch (prefix 'in_') or the depth-ray batch ('in_depth_': rays / extras / u only)."""
    depth_keys = {"in_depth_rays", "in_depth_extras", "in_depth_u"}
    b = {}
    for k in z.files:
        if prefix == "in_" and k.startswith("in_") and k not in depth_keys:
            b[k[3:]] = z[k]
        elif prefix == "in_depth_" and k in depth_keys:
            b[k[len(prefix):]] = z[k]
    return O.batch_to_torch(b)


def max_abs(a, b):
    a = torch.as_tensor(np.asarray(a)).double()
    b = torch.as_tensor(np.asarray(b)).double()
    return float((a - b).abs().max()) if a.numel() else 0.0


def rel_err(a, b):
    a = torch.as_tensor(np.asarray(a)).double().reshape(-1)
    b = torch.as_tensor(np.asarray(b)).double().reshape(-1)
    return float((a - b).norm() / (b.norm() + 1e-30))


def check_validation_metrics(device):
    """Device-side validation metrics (snerf_amd/semantic/components/metrics.py, snerf_amd/eval/utils/metrics.py) against
    plain numpy restatements of the reference definitions (semantic/components/metrics.py:11-87,
    eval/utils/metrics.py:8-18), with every tensor on `device`.  parity unpinned: torchmetrics / kornia are absent."""
    from snerf_amd.semantic.components import metrics as M
    from snerf_amd.eval.utils.metrics import mse, psnr, sum_squared_error
    dev = torch.device(device)
    rng = np.random.default_rng(5)
    N, S, Cn = 500, 8, 6                       # class 5 never occurs: NaN IoU -> skipped
    gt = rng.integers(0, 5, size=(N, 1)).astype(np.uint8)
    pred = np.where(rng.random(N) < 0.7, gt[:, 0], rng.integers(0, 5, size=N)).astype(np.int64)
    wn, bn = rng.random((N, S)).astype(np.float32), rng.random((N, S, 1)).astype(np.float32)
    res = {"semantic_label_coarse": torch.from_numpy(pred).to(dev), "rgb_coarse": torch.zeros(N, 3, device=dev),
           "weights_coarse": torch.from_numpy(wn).to(dev), "beta_coarse": torch.from_numpy(bn).to(dev)}
    tg = torch.from_numpy(gt).to(dev)
    err = (gt[:, 0] != pred).astype(np.float32)
    acc = M.semantic_accuracy(res, tg)
    assert acc.device.type == dev.type and abs(float(acc) - (1 - err.sum() / N)) < 1e-6
    err4 = np.where(gt[:, 0] == 4, 0.0, err)
    assert abs(float(M.semantic_accuracy(res, tg, filter_idx=4)) - (1 - err4.sum() / N)) < 1e-6
    assert M.semantic_error(res["semantic_label_coarse"], tg).shape == tg.shape
    counts = np.zeros((Cn, Cn))
    for g, p in zip(gt[:, 0], pred):
        counts[g, p] += 1
    cm_counts = M.confusion_matrix_values(res, tg, Cn, normalize=None)
    assert cm_counts.device.type == dev.type and np.array_equal(cm_counts.cpu().numpy(), counts)
    cm = M.confusion_matrix_values(res, tg, Cn).cpu().numpy()
    rows = counts.sum(1, keepdims=True)
    assert np.allclose(cm, np.divide(counts, rows, out=np.zeros_like(counts), where=rows > 0), atol=1e-6)
    ious = np.array([counts[c, c] / (counts[c].sum() + counts[:, c].sum() - counts[c, c]) if
                     (counts[c].sum() + counts[:, c].sum()) > 0 else np.nan for c in range(Cn)])
    assert abs(float(M.semantic_mIoU(cm_counts)) - np.nanmean(ious)) < 1e-9
    assert abs(float(M.semantic_mIoU(cm_counts.cpu().numpy())) - np.nanmean(ious)) < 1e-9   # the reference passes numpy
    comp = (wn[..., None] * bn).sum(-2)[:, 0]
    car = gt[:, 0] == 3
    assert abs(float(M.uncertainty_at_transient(res, tg, 3)) - comp[car].sum() / car.sum()) < 1e-5
    g = torch.Generator().manual_seed(1)
    a, c = torch.rand(40, 3, generator=g).to(dev), torch.rand(40, 3, generator=g).to(dev)
    mask = (torch.rand(40, generator=g) > 0.5).to(dev)
    want = float(-10 * torch.log10(((a - c) ** 2)[mask].mean()))
    got = psnr(a, c, mask)
    assert got.device.type == dev.type and abs(float(got) - want) < 1e-5
    assert abs(float(psnr(a, c)) - float(-10 * torch.log10(((a - c) ** 2).mean()))) < 1e-5
    sse, cnt = sum_squared_error(a, c, mask)
    assert float(cnt) == 3 * int(mask.sum()) and abs(float(sse / cnt) - float(mse(a, c, mask))) < 1e-7
    assert mse(a, c, reduction="none").shape == (40, 3) and mse(a, c, mask, reduction="none").shape == (int(mask.sum()), 3)
    img_mask = (torch.rand(5, 8, generator=g) > 0.3).to(dev)           # an (H, W) mask over an (H, W, 3) image
    ia, ic = torch.rand(5, 8, 3, generator=g).to(dev), torch.rand(5, 8, 3, generator=g).to(dev)
    assert abs(float(mse(ia, ic, img_mask)) - float(((ia - ic) ** 2)[img_mask].mean())) < 1e-6


# ----------------------------------------------------------------------------------------------------------------------
# CPU-oracle subsets that do not alias onto the 128-point row tiles
# ----------------------------------------------------------------------------------------------------------------------
TILE_ROWS = 128     # rows (points) of a row tile of every point-major launch
XCD_GROUPS = 8      # workgroups b and b + 8 share an XCD: the tile maps (csrc/tiles.h) group row tiles by index mod 8


def dealiased_subset(N, n_sub, S):
    """n_sub of N rays for the oracle: ray k * stride + ((k + k // 8) mod stride), stride = N // n_sub.  A plain power-of-two stride puts
    every live ray at the same position of its row tile (4096 x 64, stride 16: rays 0, 16, 32, ... = rows 0-63 of the tiles
    0, 8, 16, ... only): then only one tile residue mod 8 and one half of a tile carry gradient, and every other 128 x 128 block
    of dZ / dX is zero.  The per-ray offset walks every position inside the stride; the k // 8 term keeps it from locking to k
    mod 8 (the plain k mod stride reached four residues at 301 x 96, stride 4).  Returns the indices and the live points'
    coverage: the row-tile residues mod 8 and the tile halves (rows 0-63 / 64-127) they touch."""
    stride = N // n_sub
    k = torch.arange(n_sub)
    idx = k * stride + (k + k // XCD_GROUPS) % stride
    assert int(idx[-1]) < N and len(set(idx.tolist())) == n_sub
    pts = (idx[:, None] * S + torch.arange(S)[None, :]).reshape(-1)
    residues = set((pts // TILE_ROWS % XCD_GROUPS).tolist())
    halves = set((pts % TILE_ROWS // (TILE_ROWS // 2)).tolist())
    return idx, residues, halves


# ----------------------------------------------------------------------------------------------------------------------
# the oracle over a whole batch, in fp64, on any device
# ----------------------------------------------------------------------------------------------------------------------
class PerRayRows:
    """stands in for an embedding table where the oracle's render_rays looks rows up by image index: hands out the given
    per-ray rows (a slice of one leaf) whatever the index"""

    def __init__(self, rows):
        self.rows = rows

    def __getitem__(self, _):
        return self.rows


ORACLE_CHUNK_POINTS = 16384   # points per ray chunk: about 4 GB of fp64 autograd state at W = 512 (main + sc pass)


def chunked_oracle(cfg, params_np, emb_np, batch, epoch, device, emb_s_np=None, dtype=torch.float64,
                   chunk_points=ORACLE_CHUNK_POINTS, g_out=None):
    """Outputs, loss terms and gradients of O.render_rays + O.training_losses over a WHOLE batch, with the autograd state of
    one ray chunk at a time.  Phase 1 renders the chunks without grad, concatenates the outputs into leaves and evaluates the
    loss set on the whole batch (true means, CE ignore-index count and L_t car-ray count) to get d loss / d output of every ray;
    phase 2 re-renders each chunk with grad and back-propagates its slice of those output gradients, so the parameter
    gradients accumulate over the chunks.  Rays are independent, so this is the whole-batch backward up to summation order.
    The transient codes enter as ONE per-ray leaf (the table's rows of the batch): its gradient is d loss / d t per ray, and the
    table's gradient is its scatter-add by image index.  `batch`: CPU tensors as O.batch_to_torch makes them (floats are cast
    to `dtype`).  Returns a dict: out (detached), loss ({term: float}), grads ({name: tensor}), emb / emb_s (table gradients or
    None), t_rows (per-ray d loss / d t or None), g_out ({output: d loss / d output}), peak_bytes (CUDA: peak allocation above
    the starting level, else None).  `g_out` given ({output: tensor}): phase 2 back-propagates those output gradients (cast to
    `dtype`) instead of the loss's own, and `loss` is empty -- the backward alone, driven by another oracle's output gradients."""
    dev = torch.device(device)
    cuda = dev.type == "cuda"
    if cuda:
        torch.cuda.synchronize(dev)
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
    p = O.to_torch(params_np, dtype=dtype)
    p = {k: v.to(dev).requires_grad_(True) for k, v in p.items()}
    b = {k: (v.to(dev, dtype) if v.is_floating_point() else v.to(dev)) for k, v in batch.items()}
    ts = b["extras"][:, 3].long()
    tables = [torch.from_numpy(emb_np).to(dev, dtype)] + ([torch.from_numpy(emb_s_np).to(dev, dtype)] if emb_s_np is not None else [])
    rows = [t[ts].detach().requires_grad_(True) for t in tables]
    N, S = b["rays"].shape[0], cfg.n_samples
    R = max(1, chunk_points // S)
    chunks = [(i, min(N, i + R)) for i in range(0, N, R)]

    def render(i, j):
        return O.render_rays(p, PerRayRows(rows[0][i:j]), cfg, b["rays"][i:j], b["extras"][i:j], b["u"][i:j],
                             PerRayRows(rows[1][i:j]) if len(rows) > 1 else None)

    with torch.no_grad():                                                          # phase 1
        parts = [render(i, j) for i, j in chunks]
    out = {k: torch.cat([q[k] for q in parts], 0) for k in parts[0]}
    del parts
    if g_out is None:
        leaves = {k: v.requires_grad_(True) for k, v in out.items() if v.is_floating_point() and k != "_z_vals"}
        ld = O.training_losses({**out, **leaves}, b, cfg, epoch)
        O.total_loss(ld).backward()
        g_out = {k: v.grad for k, v in leaves.items() if v.grad is not None}
    else:
        ld = {}
        g_out = {k: v.to(dev, dtype) for k, v in g_out.items()}
    for i, j in chunks:                                                            # phase 2
        r = render(i, j)
        keys = list(g_out)
        torch.autograd.backward([r[k] for k in keys], [g_out[k][i:j] for k in keys])
        del r
    res = {"out": {k: v.detach() for k, v in out.items()}, "loss": {k: float(v.detach()) for k, v in ld.items()},
           "grads": {k: v.grad for k, v in p.items()}, "emb": None, "emb_s": None, "t_rows": rows[0].grad, "g_out": g_out,
           "peak_bytes": None}
    for name, t, r in zip(("emb", "emb_s"), tables, rows):
        if r.grad is not None:
            res[name] = torch.zeros_like(t).index_add_(0, ts, r.grad)
    if cuda:
        torch.cuda.synchronize(dev)
        res["peak_bytes"] = torch.cuda.max_memory_allocated(dev) - base
    return res
