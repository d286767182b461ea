"""GeoTIFF readers of the scene loaders -- mirror of framework/util/img_utils.py:9-43.  The scenes' RGB and CLS rasters are
plain 8-bit TIFFs, read with PIL (the reference reads them with rasterio, which this build does not carry)."""
import numpy as np
import torch
from PIL import Image


def _read(img_path, what):
    try:
        with Image.open(img_path) as im:
            im.load()
            return np.array(im)
    except Exception as e:   # PIL raises several types for an unreadable or truncated file
        raise ValueError(f"cannot decode the {what} GeoTIFF {img_path!r}: {e}") from e


def load_tensor_from_rgb_geotiff(img_path):
    """(h*w, 3) fp32 = fp32(x_u8 / 255.0 in fp64), pixels in row-major order (ToTensor of the fp64 array, then .view / .permute)"""
    img = _read(img_path, "RGB")
    if img.ndim != 3 or img.shape[2] != 3 or img.dtype != np.uint8:
        raise ValueError(f"RGB GeoTIFF {img_path!r}: expected an 8-bit 3-band raster, got {img.dtype} {img.shape}")
    return torch.from_numpy((img.reshape(-1, 3) / 255.0).astype(np.float32))


def load_tensor_from_cls_geotiff(img_path):
    """(h*w, 1) uint8: the raw label values (no palette conversion)"""
    lab = _read(img_path, "CLS")
    if lab.ndim != 2 or lab.dtype != np.uint8:
        raise ValueError(f"CLS GeoTIFF {img_path!r}: expected an 8-bit single-band raster, got {lab.dtype} {lab.shape}")
    return torch.from_numpy(np.ascontiguousarray(lab.reshape(-1, 1)))
