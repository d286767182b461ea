"""Image-error metrics of the validation step as device-side reductions.

Same definitions as the reference's `mse` / `psnr` (eval/utils/metrics.py:8-18): squared error averaged over
the selected elements, PSNR = -10 log10(MSE) for images in [0, 1].  Written as ONE masked sum-of-squares
reduction: a `valid_mask` is applied as a 0/1 weight inside the reduction (no boolean-index gather, hence no
data-dependent shape and no host synchronisation), and the result stays a 0-d device tensor until it is logged.
The DSM altitude MAE is eval/utils/dsm.py.

SSIM (metrics.py:21-83) is one HIP kernel pair (csrc/ssim.hip): a tile kernel takes the five window sums over the ws x ws taps
in fp64 and forms the SSIM value in fp64, a reduce kernel sums each image's tile partials in a fixed order (no float atomics,
no host synchronisation; bit-reproducible, and an image's value does not depend on the rest of the batch).  Inputs are CUDA
fp32 (B, C, H, W) tensors; anything else raises (there is no CPU fallback).  Two forms, under the reference's names:
- `ssim(image_pred, image_gt)` = torch.mean(kornia.losses.ssim(pred, gt, 3)) of kornia 0.5.3: window x = arange(ws) - ws // 2,
  g = exp(-x^2 / (2 * 1.5^2)), g /= g.sum(), K = g g^T, all fp32; reflect padding of ws // 2 (the edge is not repeated);
  C1 = (0.01 max_val)^2, C2 = (0.03 max_val)^2 with max_val = 1; map = num / (den + 1e-12).  kornia is not installed here:
  this form is RESTATED from kornia 0.5.3, not run against it.  The reference's callers pass (H*W, 3) frames through
  `.view(1, 3, H, W)`, so its three "channels" are the three thirds of the interleaved buffer, not R, G and B (kept as is).
- `ssim_inria(img1, img2, window_size=11, size_average=True)`: `create_window`'s window (Python math.exp values in fp32,
  normalised and outer-multiplied in fp32), zero padding of ws // 2, no eps; size_average=False gives one mean per image, (B,).
  Pinned by fixtures the reference's own code made (tests/golden/ssim_*.npz).
Both return fp32 device tensors (the fp64 sums divided by the element count, rounded once)."""
import math

import torch


def _weights(mask, like):
    """`mask` selects leading-dimension entries of `like` (the reference indexes value[mask]); returns it as a
    float weight broadcast over the trailing dimensions, plus the number of selected ELEMENTS."""
    w = mask.to(device=like.device, dtype=like.dtype)
    per_entry = 1
    for d in like.shape[w.dim():]:
        per_entry *= int(d)
    count = w.sum() * per_entry
    return w.reshape(w.shape + (1,) * (like.dim() - w.dim())), count


def sum_squared_error(image_pred, image_gt, valid_mask=None):
    """(sum of squared differences, element count) over the valid elements -- the two numbers a sharded
    validation step all-reduces before forming the global PSNR."""
    diff = image_pred - image_gt
    if valid_mask is None:
        return torch.sum(diff * diff), torch.tensor(float(diff.numel()), device=diff.device)
    w, count = _weights(valid_mask, diff)
    # excluded elements contribute an exact zero even when they hold NaN / Inf (0 * NaN would poison the sum; the reference's
    # boolean gather never reads them)
    return torch.sum(torch.where(w > 0, w * diff * diff, torch.zeros_like(diff))), count


def mse(image_pred, image_gt, valid_mask=None, reduction="mean"):
    if reduction != "mean":
        # per-element form (only the visualisers ask for it): the reference's boolean gather
        err = torch.square(image_pred - image_gt)
        return err if valid_mask is None else err[valid_mask]
    sse, count = sum_squared_error(image_pred, image_gt, valid_mask)
    return sse / count


def psnr(image_pred, image_gt, valid_mask=None, reduction="mean"):
    return -10.0 * torch.log10(mse(image_pred, image_gt, valid_mask, reduction))


# ---- SSIM ---------------------------------------------------------------------------------------------------------------
KORNIA_SIGMA = 1.5
_windows = {}      # (form, ws, device) -> contiguous (ws, ws) fp32 table on the device


def gaussian(window_size, sigma):
    """ssim_inria's 1-D window: Python-float exponentials stored as fp32, normalised by their fp32 sum"""
    centre = window_size // 2
    g = torch.tensor([math.exp(-((k - centre) ** 2) / float(2 * sigma ** 2)) for k in range(window_size)],
                     dtype=torch.float32)
    return g / g.sum()


def create_window(window_size, channel):
    """ssim_inria's (channel, 1, ws, ws) fp32 window: the outer product of `gaussian(ws, 1.5)` with itself, in fp32"""
    g = gaussian(window_size, 1.5).unsqueeze(1)
    k2 = g.mm(g.t()).float()
    return k2.expand(channel, 1, window_size, window_size).contiguous()


def kornia_window(window_size, sigma=KORNIA_SIGMA):
    """kornia 0.5.3's get_gaussian_kernel2d((ws, ws), (sigma, sigma)) for an odd ws: fp32 throughout"""
    x = torch.arange(window_size, dtype=torch.float32) - window_size // 2
    g = torch.exp(-x.pow(2.0) / float(2 * sigma ** 2))
    g = g / g.sum()
    return torch.matmul(g.unsqueeze(-1), g.unsqueeze(-1).t())


def _window(form, window_size, device):
    key = (form, int(window_size), str(device))
    if key not in _windows:
        k2 = create_window(window_size, 1)[0, 0] if form == "inria" else kornia_window(window_size)
        _windows[key] = k2.contiguous().to(device)
    return _windows[key]


def _check_images(img1, img2):
    for t in (img1, img2):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise ValueError("SSIM runs on the device: pass CUDA tensors")
        if t.dtype != torch.float32:
            raise TypeError(f"SSIM takes float32 images, not {t.dtype}")
        if t.dim() != 4:
            raise ValueError(f"SSIM takes (B, C, H, W) images, not {tuple(t.shape)}")
    if img1.shape != img2.shape or img1.device != img2.device:
        raise ValueError(f"SSIM images differ: {tuple(img1.shape)} on {img1.device} vs {tuple(img2.shape)} on {img2.device}")


def ssim_sums(img1, img2, window, border, c1, c2, eps=0.0, return_map=False):
    """The kernel behind both forms: per-image fp64 sums of the SSIM map of two CUDA fp32 (B, C, H, W) images under the
    (ws, ws) fp32 `window` with `border` "reflect" or "zero"; with return_map also the fp32 map.  Returns (sums, map|None)."""
    from ... import _lib
    _check_images(img1, img2)
    if border not in ("reflect", "zero"):
        raise ValueError(f"border must be 'reflect' or 'zero', not {border!r}")
    x, y = img1.contiguous(), img2.contiguous()
    b, c, h, w = x.shape
    k = window.to(device=x.device, dtype=torch.float32).contiguous()
    ws = k.shape[-1]
    if k.dim() != 2 or k.shape[0] != ws:
        raise ValueError(f"the window must be (ws, ws), not {tuple(k.shape)}")
    nbytes = _lib.call_size("snerf_ssim_workspace_bytes", b, c, h, w, ws, exc=ValueError)
    work = torch.empty(nbytes // 8, dtype=torch.float64, device=x.device)
    sums = torch.empty(b, dtype=torch.float64, device=x.device)
    smap = torch.empty_like(x) if return_map else None
    mode = _lib.SSIM_REFLECT if border == "reflect" else _lib.SSIM_ZERO
    _lib.call("snerf_ssim", x, y, b, c, h, w, ws, mode, k, c1, c2, eps, smap, sums, work, nbytes, exc=ValueError)
    return sums, smap


def ssim(image_pred, image_gt):
    """torch.mean(kornia.losses.ssim(image_pred, image_gt, 3)) (kornia 0.5.3; restated, see the module docstring); 0-d fp32"""
    sums, _ = ssim_sums(image_pred, image_gt, _window("kornia", 3, image_pred.device), "reflect",
                        (0.01 * 1.0) ** 2, (0.03 * 1.0) ** 2, 1e-12)
    return (sums.sum() / image_pred.numel()).to(torch.float32)


def ssim_inria(img1, img2, window_size=11, size_average=True):
    """metrics.py:29-83: Gaussian window of `create_window`, zero padding, no eps; the mean over everything, or (B,) per-image
    means with size_average=False"""
    sums, _ = ssim_sums(img1, img2, _window("inria", window_size, img1.device), "zero", 0.01 ** 2, 0.03 ** 2, 0.0)
    per_image = img1[0].numel()
    if size_average:
        return (sums.sum() / (per_image * img1.shape[0])).to(torch.float32)
    return (sums / per_image).to(torch.float32)
