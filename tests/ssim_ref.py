"""Plain-torch fp64 restatement of the two SSIM forms of eval/utils/metrics.py (the yardstick of the SSIM kernel): pad with
F.pad (reflect, or zeros), filter each plane with F.conv2d (depthwise), and form the SSIM map from the five window sums.
Inputs of any float dtype are taken to fp64; the window is the fp32 table the kernel is handed, cast to fp64."""
import torch
import torch.nn.functional as F


def ssim_map(x, y, window, border, c1, c2, eps=0.0):
    """SSIM map, fp64 (B, C, H, W), of (B, C, H, W) images under the (ws, ws) `window`; border "reflect" or "zero"."""
    x, y = x.double().cpu(), y.double().cpu()
    ws = window.shape[-1]
    r = ws // 2
    c = x.shape[1]
    k = window.double().cpu().reshape(1, 1, ws, ws).expand(c, 1, ws, ws)

    def filt(t):
        if border == "reflect":
            return F.conv2d(F.pad(t, (r, r, r, r), mode="reflect"), k, groups=c)
        return F.conv2d(t, k, padding=r, groups=c)

    mu1, mu2 = filt(x), filt(y)
    mu11, mu22, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1, s2, s12 = filt(x * x) - mu11, filt(y * y) - mu22, filt(x * y) - mu12
    num = (2.0 * mu12 + c1) * (2.0 * s12 + c2)
    den = (mu11 + mu22 + c1) * (s1 + s2 + c2)
    return num / (den + eps)


def kornia_window(window_size, sigma=1.5):
    """kornia 0.5.3's gaussian + get_gaussian_kernel2d for an odd window, in fp32 (restated)"""
    x = torch.arange(window_size).float() - window_size // 2
    g = torch.exp(-x.pow(2.0) / float(2 * sigma ** 2))
    g = g / g.sum()
    return torch.matmul(g.unsqueeze(-1), g.unsqueeze(-1).t())


def kornia_map(x, y, window_size=3):
    """kornia 0.5.3's ssim map (restated): reflect padding, C1 = 0.01^2, C2 = 0.03^2, eps = 1e-12"""
    return ssim_map(x, y, kornia_window(window_size), "reflect", (0.01 * 1.0) ** 2, (0.03 * 1.0) ** 2, 1e-12)


def inria_map(x, y, window_size=11):
    """ssim_inria's map: create_window, zero padding, no eps"""
    from snerf_amd.eval.utils.metrics import create_window
    return ssim_map(x, y, create_window(window_size, 1)[0, 0], "zero", 0.01 ** 2, 0.03 ** 2)


def inria(x, y, window_size=11, size_average=True):
    m = inria_map(x, y, window_size)
    return m.mean() if size_average else m.mean(dim=(1, 2, 3))


def frame_view(frame, h, w):
    """the reference callers' (H*W, 3) -> (1, 3, H, W) reinterpretation (the three thirds of the flat buffer)"""
    return frame.reshape(1, 3, h, w)
