"""GeoTIFF readers of the scene loaders -- mirror of framework/util/img_utils.py:9-43 -- and the writer of the ortho products.  The scenes' RGB and CLS rasters are
plain 8-bit TIFFs, read with PIL (the reference reads them with rasterio, which this build does not carry).

The DSM ground truth (framework/datasets.py:35-44, eval/utils/dsm.py:180-231): a float32 single-band raster whose georeference
is read from the GeoTIFF tags ModelPixelScale (33550) and ModelTiepoint (33922) (north-up, no rotation), the ROI text file
(xoff, yoff, size, resolution) and the water (class 9) or ignore mask.  Cropping to the ROI replaces the reference's
gdal.Translate(projWin=...): an integer-offset crop when the raster lies on the ROI's lattice; a raster without the tags must
already have the ROI's shape.  DIVERGENCE: anything else (another resolution, a corner off the lattice by more than 1e-6 cells,
an ROI reaching beyond the raster) raises ValueError where gdal would resample or pad -- unless `resample=` is given: the raster is
then warped onto the ROI's lattice on the device (eval/utils/warp.py), cells it does not cover NaN / 255.

save_geotiff writes a north-up raster on a DsmGrid with the same two tags and, given the scene's UTM zone, a GeoKeyDirectory
(34735) naming the projected CRS (EPSG 326zz north / 327zz south).  The reference writes its DSMs with rasterio; neither
rasterio nor GDAL is part of this build, so what their readers make of these files is UNPINNED (as `utm` and cv2 are, DESIGN.md
5h / 5i): the tests pin the round trip through PIL and load_dsm_geotiff."""
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


TAG_MODEL_PIXEL_SCALE = 33550
TAG_MODEL_TIEPOINT = 33922
TAG_GEO_KEY_DIRECTORY = 34735


def load_dsm_geotiff(fp):
    """(raster (h, w) ndarray in the file's dtype, geotransform (x0, y0, sx, sy) or None): x0 / y0 = the outer corner of the
    north-west pixel, sx / sy = the pixel size east / south; None when the file carries no ModelPixelScale / ModelTiepoint"""
    try:
        with Image.open(fp) as im:
            im.load()
            a = np.array(im)
            tags = getattr(im, "tag_v2", {})
            scale, tie = tags.get(TAG_MODEL_PIXEL_SCALE), tags.get(TAG_MODEL_TIEPOINT)
    except Exception as e:
        raise ValueError(f"cannot decode the DSM GeoTIFF {fp!r}: {e}") from e
    if a.ndim != 2:
        raise ValueError(f"DSM GeoTIFF {fp!r}: expected a single-band raster, got {a.dtype} {a.shape}")
    if scale is None or tie is None:
        return a, None
    scale, tie = [float(v) for v in scale], [float(v) for v in tie]
    if len(scale) < 2 or len(tie) < 6 or not (scale[0] > 0 and scale[1] > 0):
        raise ValueError(f"DSM GeoTIFF {fp!r}: malformed ModelPixelScale / ModelTiepoint tags")
    return a, (tie[3] - tie[0] * scale[0], tie[4] + tie[1] * scale[1], scale[0], scale[1])


def crop_to_roi(raster, geotransform, roi_meta, what="DSM", resample=None, device=None):
    """the (size, size) window of `raster` that the ROI (xoff, yoff, size, resolution; yoff = the SOUTH edge) covers.
    `resample` (default None: anything off the ROI's lattice raises, as before): True or a method name of eval/utils/warp.py -- a raster
    at another resolution, off the ROI's lattice or not containing the ROI is warped onto it on `device` (default "cuda") and comes
    back as a host array; True takes the default method (bilinear / nearest onto a lattice as fine or finer, average / mode
    otherwise), a uint8 raster always the label default.  ROI cells the raster does not cover are NaN (255 in a uint8 raster).  A raster
    on the ROI's lattice that contains the ROI is cropped as without `resample`: its bits are kept."""
    xoff, yoff, size, res = [float(v) for v in np.asarray(roi_meta, np.float64).reshape(-1)[:4]]
    n = int(size)
    if geotransform is None:
        if raster.shape != (n, n):
            raise ValueError(f"{what} raster of shape {raster.shape} carries no georeference and is not the ROI's {n} x {n}")
        return raster
    x0, y0, sx, sy = geotransform
    i = j = 0
    refusal = None
    if abs(sx - res) > 1e-9 * res or abs(sy - res) > 1e-9 * res:
        refusal = f"{what} raster resolution ({sx}, {sy}) != ROI resolution {res}: resampling is not supported"
    else:
        fi, fj = (xoff - x0) / res, (y0 - (yoff + n * res)) / res
        i, j = round(fi), round(fj)
        if abs(fi - i) > 1e-6 or abs(fj - j) > 1e-6:
            refusal = (f"{what} raster origin ({x0}, {y0}) is off the ROI lattice ({xoff} + k {res}, {yoff} + k {res}): "
                       "resampling is not supported")
        elif i < 0 or j < 0 or i + n > raster.shape[1] or j + n > raster.shape[0]:
            refusal = f"the ROI ({n} x {n} cells from column {i}, row {j}) reaches beyond the {what} raster {raster.shape}"
    if refusal is not None and resample:
        from ...eval.utils import warp as W
        method = None if resample is True or raster.dtype == np.uint8 else resample
        src = torch.from_numpy(np.ascontiguousarray(raster)).to(device or "cuda")
        return W.warp(src, W.lattice_of(geotransform, raster.shape), W.Lattice(xoff, yoff + n * res, res, res, n, n), method).cpu().numpy()
    if refusal is not None:
        raise ValueError(refusal)
    return raster[j:j + n, i:i + n]


def load_dsm_ground_truth(dsm_tif_fp, dsm_txt_fp, dsm_cls_fp=None, ignore_mask_fp=None, resample=None, device=None):
    """{"gt": (n, n) f32, "roi": (4,) f64, "water_mask" | "ignore_mask": (n, n) u8} as CPU tensors.  Exactly one mask is used, as
    eval/utils/dsm.py:124-129,199-219 of the reference: the ignore mask when the scene names one, else the water mask (the CLS
    raster; class 9 is water) when its file exists.  `resample`, `device`: as crop_to_roi takes them (the method name serves the DSM,
    a mask takes the label default); without them a raster off the ROI's lattice raises."""
    import os
    roi = np.loadtxt(dsm_txt_fp, dtype=np.float64).reshape(-1)
    if roi.size < 4:
        raise ValueError(f"ROI file {dsm_txt_fp!r}: expected xoff, yoff, size, resolution")
    gt, gtf = load_dsm_geotiff(dsm_tif_fp)
    if gt.dtype != np.float32:
        raise ValueError(f"DSM GeoTIFF {dsm_tif_fp!r}: expected a float32 raster, got {gt.dtype}")
    out = {"gt": torch.from_numpy(np.ascontiguousarray(crop_to_roi(gt, gtf, roi, resample=resample, device=device))),
           "roi": torch.from_numpy(roi[:4].copy())}
    key, fp = ("ignore_mask", ignore_mask_fp) if ignore_mask_fp else ("water_mask", dsm_cls_fp)
    if fp and os.path.isfile(fp):
        m, mtf = load_dsm_geotiff(fp)
        if resample:
            m = m.astype(np.uint8)
        out[key] = torch.from_numpy(np.ascontiguousarray(crop_to_roi(m, mtf, roi, what=key, resample=resample, device=device)).astype(np.uint8))
    return out


def utm_epsg(zone_string):
    """EPSG code of WGS 84 / UTM zone zz: 326zz on the northern hemisphere, 327zz on the southern"""
    from .conversions import split_zone_string, zone_is_south
    number = split_zone_string(zone_string)[0]
    if not 1 <= number <= 60:
        raise ValueError(f"UTM zone number {number} outside [1, 60]")
    return (32700 if zone_is_south(zone_string) else 32600) + number


def save_geotiff(fp, array, grid, zone_string=None):
    """Write `array` -- (h, w) float32 ("F"), (h, w) int32 ("I"), (h, w) uint8 ("L") or (h, w, 3) uint8 ("RGB"); a tensor or an ndarray -- as an
    uncompressed TIFF on `grid` (a DsmGrid: xoff / yoff = the outer corner of the north-west cell): ModelPixelScale =
    (res, res, 0), ModelTiepoint = (0, 0, 0, xoff, yoff, 0) and, with `zone_string`, a GeoKeyDirectory (projected model,
    pixel-is-area, ProjectedCSTypeGeoKey = utm_epsg(zone_string)).  No RPC tags."""
    from PIL import TiffImagePlugin
    a = array.detach().cpu().numpy() if torch.is_tensor(array) else np.asarray(array)
    if a.ndim == 2 and a.dtype == np.float32:
        mode = "F"
    elif a.ndim == 2 and a.dtype == np.int32:
        mode = "I"
    elif a.ndim == 2 and a.dtype == np.uint8:
        mode = "L"
    elif a.ndim == 3 and a.shape[2] == 3 and a.dtype == np.uint8:
        mode = "RGB"
    else:
        raise ValueError(f"save_geotiff: expected (h, w) float32, (h, w) int32, (h, w) uint8 or (h, w, 3) uint8, got {a.dtype} {a.shape}")
    if a.shape[:2] != (int(grid.ysize), int(grid.xsize)):
        raise ValueError(f"save_geotiff: the raster is {a.shape[0]} x {a.shape[1]}, the grid {grid.ysize} x {grid.xsize}")
    res = float(grid.resolution)
    ifd = TiffImagePlugin.ImageFileDirectory_v2()
    ifd[TAG_MODEL_PIXEL_SCALE] = (res, res, 0.0)
    ifd.tagtype[TAG_MODEL_PIXEL_SCALE] = 12          # DOUBLE
    ifd[TAG_MODEL_TIEPOINT] = (0.0, 0.0, 0.0, float(grid.xoff), float(grid.yoff), 0.0)
    ifd.tagtype[TAG_MODEL_TIEPOINT] = 12
    if zone_string is not None:
        # header (version 1, revision 1.0, 3 keys); GTModelTypeGeoKey = 1 (projected); GTRasterTypeGeoKey = 1 (pixel is area);
        # ProjectedCSTypeGeoKey = the EPSG code
        ifd[TAG_GEO_KEY_DIRECTORY] = (1, 1, 0, 3, 1024, 0, 1, 1, 1025, 0, 1, 1, 3072, 0, 1, utm_epsg(zone_string))
        ifd.tagtype[TAG_GEO_KEY_DIRECTORY] = 3       # SHORT
    Image.fromarray(np.ascontiguousarray(a), mode=mode).save(fp, format="TIFF", tiffinfo=ifd)
    return fp
