"""Colour tables and the default label palette of the visualisers -- the project's own data.

JET and BONE are (256, 3) uint8 tables in the channel order the reference ends up with: it hands cv2.applyColorMap's BGR rows to
PIL as if they were RGB (framework/util/other.py visualize_image), so band 0 of the written image holds the map's BLUE, band 2
its RED.  OpenCV is not part of this build: the tables are restated from the maps' published definitions (MATLAB's jet and
bone, which OpenCV's tables sample at 256 points), and parity with cv2's own arrays is UNPINNED -- a value may
differ by a unit of the last place where OpenCV rounded its table differently.  The quantisation in front of the table (the
index) is pinned against the reference by tests/golden/vis_*.npz."""
import numpy as np

COLORMAP_BONE = 1       # cv2.COLORMAP_BONE
COLORMAP_JET = 2        # cv2.COLORMAP_JET


def _jet_rgb():
    x = np.arange(256, dtype=np.float64) / 255.0
    r = np.clip(1.5 - np.abs(4.0 * x - 3.0), 0.0, 1.0)
    g = np.clip(1.5 - np.abs(4.0 * x - 2.0), 0.0, 1.0)
    b = np.clip(1.5 - np.abs(4.0 * x - 1.0), 0.0, 1.0)
    return np.stack([r, g, b], 1)


def _bone_rgb():
    # bone = (7 * gray + fliplr(hot)) / 8, hot rising over thirds of the range
    x = np.arange(256, dtype=np.float64) / 255.0
    h0, h1, h2 = np.clip(3.0 * x, 0, 1), np.clip(3.0 * x - 1.0, 0, 1), np.clip(3.0 * x - 2.0, 0, 1)
    return np.stack([(7.0 * x + h2) / 8.0, (7.0 * x + h1) / 8.0, (7.0 * x + h0) / 8.0], 1)


def _as_written(rgb):
    return np.ascontiguousarray(np.rint(rgb[:, ::-1] * 255.0).astype(np.uint8))      # BGR rows, read as RGB


TABLES = {COLORMAP_JET: _as_written(_jet_rgb()), COLORMAP_BONE: _as_written(_bone_rgb())}
IDENTITY = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, 1)    # table[i] = (i, i, i): the index itself (tests)

# one colour per label of the scenes' class list (ground, water, vegetation, buildings, cars, and a spare)
DEFAULT_PALETTE = np.array([[222, 205, 150], [40, 120, 220], [30, 150, 70], [150, 150, 160], [210, 60, 50], [80, 80, 90]], np.uint8)

_dev = {}


def table(cmap, device):
    """the (256, 3) uint8 table of `cmap` (a COLORMAP_* id or an array) on `device`, cached"""
    import torch
    if not isinstance(cmap, int):
        return torch.as_tensor(np.asarray(cmap, np.uint8)).to(device)
    key = (cmap, str(device))
    if key not in _dev:
        if cmap not in TABLES:
            raise ValueError(f"colour map {cmap}: only COLORMAP_JET and COLORMAP_BONE are restated here")
        _dev[key] = torch.from_numpy(TABLES[cmap]).to(device)
    return _dev[key]
