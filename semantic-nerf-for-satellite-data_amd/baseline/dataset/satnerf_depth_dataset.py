"""Depth-supervision loader -- mirror of baseline/dataset/satnerf_depth_dataset.py: one ray per keypoint of every train image
(the meta's keypoints/2d_coordinates, fp64 (col, row)), built by the same ray kernel and normalised with the parameters shared
with the RGB banks; the bundle-adjusted tie points (points3d_fp, ECEF fp64) are rounded to fp32 and normalised the same way;
depths = |pts - o| in fp32 (torch's CPU norm, as the reference); weights = exp(-(e / mean e)^2) with e the summed reprojection error of each tie point over the
train images (fp32, numpy's order: the errors are computed on the device, read back once -- n_pts x n_images values -- and
reduced on the host).  Columns: rays (R, 8), depths (R, 1), weights (R, 1), extras (R, 4), as the depth step consumes them."""
import os

import numpy as np
import torch

from ...framework.datasets import GpuRayBank
from ..components.camera_models import construct_rpc_camera_model
from ..components.rays import construct_sun_dir, satnerf_construct
from .satnerf_dataset import read_json, refuse_unsupported, split_names


class SatNeRFDepthDataset:
    def __init__(self, cfgs, device=None):
        refuse_unsupported(cfgs)
        self.cfgs = cfgs
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.dataset_dp = cfgs.run.dataset_dp
        self.root = read_json(os.path.join(self.dataset_dp, "root.json"))
        if "points3d_fp" not in self.root:
            raise ValueError(f"scene {self.dataset_dp!r}: root.json has no 'points3d_fp' "
                             "(depth supervision needs the bundle-adjusted tie points)")
        self.points3d_fp = os.path.join(self.dataset_dp, self.root["points3d_fp"])
        self.meta_dp = os.path.join(self.dataset_dp, self.root["meta_dp"])
        self.data_names = split_names(self.root, "train", cfgs.run.dataset_limit_train_images)
        self.metas = [read_json(os.path.join(self.meta_dp, n)) for n in self.data_names]
        for n, d in zip(self.data_names, self.metas):
            if "keypoints" not in d:
                raise ValueError(f"meta {n} has no 'keypoints': depth supervision needs them for every train image")
        self.t = None

    def keypoint_weights(self, tie_points):
        """fp32 weight per tie point: exp(-(e / mean(e))^2), e = the point's summed reprojection error over the train images.
        The per-keypoint errors come from the device in fp64 and are stored as fp32 in a (points, images) table, zero where a
        point is not observed; the row sums, their mean and the weights follow numpy's fp32 reductions over that table."""
        idx = [np.asarray(d["keypoints"]["pts3d_indices"], np.int64) for d in self.metas]
        on_device = [construct_rpc_camera_model(d, self.device).reprojection_error(tie_points[i], d["keypoints"]["2d_coordinates"])
                     for d, i in zip(self.metas, idx)]
        table = np.zeros((tie_points.shape[0], len(self.metas)), dtype=np.float32)
        for col, (i, err) in enumerate(zip(idx, on_device)):
            table[i, col] = err.cpu().numpy()          # one read back per image (n keypoints values)
        per_point = table.sum(axis=1)
        return np.exp(-np.square(per_point / per_point.mean()))

    def load(self, normalization):
        tie_points = np.load(self.points3d_fp)
        kp_weights = self.keypoint_weights(tie_points)
        cams = [construct_rpc_camera_model(d, self.device) for d in self.metas]
        pix = [np.array(d["keypoints"]["2d_coordinates"], dtype=np.float64) for d in self.metas]
        rays = satnerf_construct(cams, [float(d["min_alt"]) for d in self.metas], [float(d["max_alt"]) for d in self.metas],
                                 pixels=pix, names=self.data_names, device=self.device)
        normalization.normalize_rays_(rays)
        idx = np.concatenate([np.asarray(d["keypoints"]["pts3d_indices"], np.int64) for d in self.metas])
        pts = torch.from_numpy(tie_points[idx, :]).type(torch.FloatTensor).to(self.device).contiguous()
        normalization.normalize_xyz(pts)
        # |pts - o| as the reference evaluates it: torch's fp32 CPU norm (its reduction rounds differently from a plain fp32 or
        # fp64 sum of squares, and from the device norm); one keypoint per row, a small host array
        depths = torch.linalg.norm((pts - rays[:, :3]).cpu(), axis=1).to(self.device)
        weights = torch.from_numpy(kp_weights[idx]).type(torch.FloatTensor)
        extras = []
        for t, (d, p) in enumerate(zip(self.metas, pix)):
            n = p.shape[0]
            extras.append(torch.hstack([construct_sun_dir(float(d["sun_elevation"]), float(d["sun_azimuth"]), n), t * torch.ones(n, 1)]))
        self.t = {"rays": rays, "depths": depths[:, None].contiguous(), "weights": weights[:, None].to(self.device),
                  "extras": torch.cat(extras, 0).to(self.device)}
        return self

    def bank(self, n_classes=5, car_cls_idx=4, seed=0):
        return GpuRayBank(self.t, n_classes=n_classes, car_cls_idx=car_cls_idx, seed=seed)
