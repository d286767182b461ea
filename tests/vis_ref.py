"""Numpy restatement of the visualisation maps (csrc/vismaps.hip, include/snerf_hip.h): what the fold and the colormap compute,
with every rounding written out.  The weighted sums are formed as the kernel's spec says -- the fp32 product, summed in fp64,
rounded once -- so they are the fp64-accumulated value the GPU tests compare against under the derived bound."""
import numpy as np

F32 = np.float32
FLT_MAX = float(np.finfo(np.float32).max)


def products(w, f):
    """fl32(w_s * f_s): w (n, S), f (n, S, B) -> (n, S, B) fp32"""
    return (np.asarray(w, F32)[..., None] * np.asarray(f, F32).reshape(w.shape[0], w.shape[1], -1)).astype(F32)


def weighted_sum(w, f):
    """(B, n) fp32 planar (B = 1: (n,)): the fp64 sum of the fp32 products, rounded once"""
    p = products(w, f).astype(np.float64).sum(1).astype(F32)          # (n, B)
    return p[:, 0] if p.shape[1] == 1 else np.ascontiguousarray(p.T)


def sum_bound(w, f):
    """the tests' bound on |ours - reference| of a weighted sum, same layout as weighted_sum: S * 2^-23 * sum_s |fl32(w_s f_s)|
    (fp32 summation in any order errs by at most (S - 1) u sum |p|, u = 2^-24; one final rounding is added, the whole doubled)"""
    S = w.shape[1]
    b = S * 2.0 ** -23 * np.abs(products(w, f).astype(np.float64)).sum(1)
    return b[:, 0] if b.shape[1] == 1 else np.ascontiguousarray(b.T)


def rgb_diff(rgb, gt):
    """(3, n) fp32 |gt - rgb|"""
    return np.ascontiguousarray(np.abs(np.asarray(gt, F32) - np.asarray(rgb, F32)).T)


def rgb_diff_distance(rgb, gt):
    d = rgb_diff(rgb, gt)
    sq = (d * d).astype(F32)
    return np.sqrt(((sq[0] + sq[1]).astype(F32) + sq[2]).astype(F32)).astype(F32)


def to_u8(v):
    """float -> uint8 through int32: truncate, low eight bits (NaN -> 0)"""
    v = np.where(np.isnan(v), 0, v)
    return (np.clip(np.trunc(v), -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64) & 255).astype(np.uint8)


def sem_color(label, palette):
    """(3, n) uint8; a label outside the palette is (0, 0, 0).  Returns (planes, count of such labels)"""
    label = np.asarray(label, np.int64).reshape(-1)
    ok = (label >= 0) & (label < palette.shape[0])
    c = np.where(ok[:, None], palette[np.where(ok, label, 0)], 0).astype(np.uint8)
    return np.ascontiguousarray(c.T), int((~ok).sum())


def sem_shaded(label, palette, sun_map):
    c, _ = sem_color(label, palette)
    return to_u8((c.astype(F32) * np.asarray(sun_map, F32)[None, :]).astype(F32))


def sem_error(label, gt):
    d = np.asarray(gt).reshape(-1).astype(np.int64) - np.asarray(label, np.int64).reshape(-1)
    return np.clip(np.abs(d), 0, 1).astype(F32)


def nan_to_num(x):
    big = np.finfo(x.dtype).max
    return np.where(np.isnan(x), x.dtype.type(0), np.clip(x, -big, big)).astype(x.dtype)


def minmax(x):
    """exact (min, max) of the nan_to_num plane as Python floats, or None for an empty plane"""
    x = nan_to_num(np.asarray(x))
    return (float(x.min()), float(x.max())) if x.size else None


def colormap_index(x, bounds=None):
    """visualize_image_numpy up to the table: every step in x's own type T.  bounds None: mi, ma the plane's own, the
    denominator fl_T(fl_T(ma - mi) + fl_T(1e-8)) (numpy >= 2); else explicit Python floats: mi = fl_T(lo), denominator
    fl_T(hi - lo + 1e-8) with the sum in fp64."""
    x = nan_to_num(np.asarray(x))
    T = x.dtype.type
    if bounds is None:
        mi, ma = (x.min(), x.max()) if x.size else (T(0), T(0))
        den = T(T(ma - mi) + T(1e-8))
    else:
        mi, den = T(bounds[0]), T(float(bounds[1]) - float(bounds[0]) + 1e-8)
    with np.errstate(over="ignore", invalid="ignore"):
        q = ((x - mi).astype(x.dtype) / den).astype(x.dtype)
        return to_u8((T(255) * q).astype(x.dtype))


def to_uint8_image(img):
    """torchvision's save_image conversion, restated: x * 255 + 0.5, clamp, uint8"""
    img = np.asarray(img, F32)
    if img.size and img.max() > 1:
        img = img / F32(255)
    return np.clip(img * F32(255) + F32(0.5), 0, 255).astype(np.uint8)
