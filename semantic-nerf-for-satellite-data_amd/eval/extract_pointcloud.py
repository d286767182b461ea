"""Point clouds from a trained model -- the device side of eval/extract_pointcloud.py:66-114: full-frame inference of
one image's rays (lean: rgb + depth [+ label] only, written in place per chunk), then the ray end points
xyz = o + d * depth in double precision (baseline/dataset/satnerf_dataset.py:156-171).  DSM rasterisation and the altitude
MAE of the cloud are eval/utils/dsm.py (device side); with `geo` (a GeoFrame, framework/components/coordinate_systems.py) the
reference's un-normalised UTM cloud comes from one more launch (csrc/geo.hip).  The reference's exporter writes nx ny nz through a
pluggable normals_fn whose default is the sun direction; here `with_normals=True` gives every point the normal of the density field
(eval/utils/normals.py, csrc/normals.hip) and save_ply writes it."""
import numpy as np
import torch

from .utils.util import guided_lean_inference, lean_inference, sharded_lean_inference, with_depth_mode


def get_xyz_from_nerf_prediction(rays: torch.Tensor, depth: torch.Tensor) -> torch.Tensor:
    """baseline/dataset/satnerf_dataset.py:156-171 -- in double, as the reference does, on whatever device holds the rays."""
    rays = rays.double()
    depth = depth.double()
    return rays[:, 0:3] + rays[:, 3:6] * depth.view(-1, 1)


@torch.no_grad()
def extract_pointcloud(cfgs, renderer, models, rays, extras, render_options=None, with_labels=None, sharded=False, geo=None,
                       with_colors=True, depth_mode="mean", guide=None, with_normals=False):
    """One image -> {"xyz_n" (R,3) f64, "colors" (R,3) f32, "depth" (R) f32 [, "labels" (R) i64]}, all on the device.
    `with_colors=False` leaves "colors" out; without labels either, the walk asks for the depth alone and runs as geometry passes
    (eval/utils/util.py: relight_chunks) -- no head launch, the same depth bits, hence the same cloud.
    With `geo` also "xyz_utm" (R,3) f64: the un-normalised UTM (east, north, alt) cloud (GeoFrame.cloud of rays and depth).
    `sharded=False` (default) is the reference's single-device call: safe from one rank of a process group (the usual export
    inside a data-parallel run).  `sharded=True` is a COLLECTIVE: every rank of the group must call it with the same rays;
    the image is rendered in rank shards and the per-ray results gathered, so every rank returns the whole cloud
    (eval/utils/util.py: sharded_lean_inference).
    `depth_mode="median"` places every point at its ray's median depth (SNERF_FLAG_DEPTH_MEDIAN) instead of the expected depth.
    `guide` (eval/utils/raycast.py DsmGuide): render with guide.n_samples depths in a band round each ray's hit on the guide's DSM
    (eval/utils/util.py guided_lean_inference) and add "guide_state" (R) u8; not with `sharded` (ValueError).  None (default):
    every path above as it was.
    `with_normals=True` adds "normals_n" (R, 3) f32, the unit normals of the density field in normalised scene coordinates (NaN where
    the field has no gradient), and with `geo` "normals_enu" (R, 3) f32, east / north / up: a walk of its own over the rays
    (normals.ray_normals: training forwards and the xyz-only backward), single-device, on the stratified depths of `render_options`
    -- {"perturb": 0} or a pinned "perturb_rand" make it the walk of the cloud.  Every other entry keeps the bits it has without.
    False (default) launches nothing new."""
    if guide is not None and sharded:
        raise ValueError("extract_pointcloud: guide= is a single-device render; pass sharded=False")
    render_options = with_depth_mode(render_options, depth_mode, "extract_pointcloud")
    sem = models["coarse"].spec.n_classes > 0
    if with_labels is None:
        with_labels = sem
    keys = (["rgb_coarse"] if with_colors else []) + ["depth_coarse"] + (["semantic_label_coarse"] if with_labels and sem else [])
    infer = sharded_lean_inference if sharded else lean_inference
    if guide is not None:
        res = guided_lean_inference(cfgs, renderer, models, rays, extras, guide, keys=keys, render_options=render_options or {})
    else:
        res = infer(cfgs, renderer, models, rays, extras, keys=keys, render_options=render_options or {})
    out = {"xyz_n": get_xyz_from_nerf_prediction(rays, res["depth_coarse"]), "depth": res["depth_coarse"]}
    if with_colors:
        out["colors"] = res["rgb_coarse"]
    if "semantic_label_coarse" in res:
        out["labels"] = res["semantic_label_coarse"]
    if guide is not None:
        out["guide_state"] = res["guide_state"]
    if geo is not None:
        out["xyz_utm"] = geo.cloud(rays, res["depth_coarse"])[0]
    if with_normals:
        from .utils import normals as NM
        nopts = {k: v for k, v in (render_options or {}).items() if k != "depth_mode"}
        out["normals_n"] = NM.ray_normals(cfgs, renderer, models, rays, extras, nopts)["normal_n"]
        if geo is not None:
            out["normals_enu"] = NM.to_enu(geo, out["normals_n"])
    return out


def filtered_indices(n_points: int, keep: int = 30000, seed: int = 0) -> torch.Tensor:
    """the reference's reduced cloud: a seeded randperm prefix (eval/extract_pointcloud.py:96-100)"""
    g = torch.Generator().manual_seed(seed)
    return torch.randperm(n_points, generator=g)[:keep]


def save_ply(fp: str, xyz, colors=None, labels=None, normals=None):
    """binary little-endian PLY: double xyz, optional float nx ny nz (`normals` (R, 3), behind xyz as the reference's exporter
    orders them), uchar rgb (colors in [0,1]), optional uchar label.  Without `normals` the file is byte for byte what it was."""
    xyz = np.asarray(xyz.detach().cpu() if torch.is_tensor(xyz) else xyz, dtype="<f8")
    fields = [("x", "<f8"), ("y", "<f8"), ("z", "<f8")]
    props = ["property double x", "property double y", "property double z"]
    if normals is not None:
        normals = np.asarray(normals.detach().cpu() if torch.is_tensor(normals) else normals, dtype="<f4")
        if normals.shape != (xyz.shape[0], 3):
            raise ValueError(f"save_ply: normals must be {(xyz.shape[0], 3)}, got {normals.shape}")
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
        props += ["property float nx", "property float ny", "property float nz"]
    if colors is not None:
        colors = np.asarray(colors.detach().cpu() if torch.is_tensor(colors) else colors)
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        props += ["property uchar red", "property uchar green", "property uchar blue"]
    if labels is not None:
        labels = np.asarray(labels.detach().cpu() if torch.is_tensor(labels) else labels)
        fields += [("label", "u1")]
        props += ["property uchar label"]
    rec = np.empty(xyz.shape[0], dtype=fields)
    rec["x"], rec["y"], rec["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    if normals is not None:
        rec["nx"], rec["ny"], rec["nz"] = normals[:, 0], normals[:, 1], normals[:, 2]
    if colors is not None:
        c = np.clip(np.rint(colors * 255.0), 0, 255).astype("u1")
        rec["red"], rec["green"], rec["blue"] = c[:, 0], c[:, 1], c[:, 2]
    if labels is not None:
        rec["label"] = labels.astype("u1")
    with open(fp, "wb") as f:
        f.write(("ply\nformat binary_little_endian 1.0\nelement vertex %d\n%s\nend_header\n" % (xyz.shape[0], "\n".join(props))).encode())
        f.write(rec.tobytes())
    return fp
