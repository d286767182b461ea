"""Semantic scene loader -- mirror of semantic/dataset/semantic_dataset.py:8-90: the SatNeRF loader plus the CLS labels of
`semantic_dp_<semantic_dataset_type>` (raw 8-bit values, (h*w, 1) uint8), the sparsity mask (train only: images from index
`sparsity_n_images` on are masked out), and where root.json names them the labels without cars
(`semantic_dp_<type>_no_cars`) and, for a corrupted type, the non-corrupted labels (`semantic_dp_<type minus "_corrupted">`)."""
import os

import torch

from ...baseline.dataset.satnerf_dataset import SatNeRFDataset
from ...framework.util.img_utils import load_tensor_from_cls_geotiff


class SemanticDataset(SatNeRFDataset):
    def __init__(self, cfgs, split: str, device=None):
        super().__init__(cfgs, split, device)
        pc = cfgs.pipeline
        kind = pc.semantic_dataset_type
        key = f"semantic_dp_{kind}"
        missing = [k for k in (key, "semantic_cls_labels") if k not in self.root]
        if missing:
            raise ValueError(f"scene {self.dataset_dp!r}: root.json lacks {missing}: a semantic pipeline needs a dataset with "
                             "semantic labels")
        self.semantic_dataset_name = key
        self.semantic_dp = self._label_dir(key)
        # a corrupted label set ("<type>_corrupted") is evaluated against the clean set of <type>
        self.labels_are_corrupted = "corrupted" in kind
        self.semantic_non_corrupted_dp = self._label_dir("semantic_dp_" + kind.removesuffix("_corrupted")) \
            if self.labels_are_corrupted else None
        self.semantic_no_cars_dp = self._label_dir(key + "_no_cars") if self.root.get(key + "_no_cars") else None
        self.semantic_cls_labels = self.root["semantic_cls_labels"]          # {"<index>": "<name>"}
        self.semantic_n_classes = len(self.semantic_cls_labels)
        self.car_cls_idx = next((int(i) for i, name in self.semantic_cls_labels.items() if name == "cars"), None)
        self.sparsity_n_images = pc.sparsity_n_images

    def _label_dir(self, root_key):
        return os.path.join(self.dataset_dp, self.root[root_key])

    def _item_extra(self, k, d, n):
        cls_name = d["img"][:-7] + "CLS.tif"
        labels = load_tensor_from_cls_geotiff(os.path.join(self.semantic_dp, cls_name))
        if labels.shape[0] != n:
            raise ValueError(f"CLS labels of {self.data_names[k]}: {labels.shape[0]} pixels for {n} rays")
        index = self.ts[k]
        sparse = self.split == "train" and 0 < self.sparsity_n_images <= index
        out = {"semantic": labels, "semantic_sparsity_mask": torch.full((n,), not sparse, dtype=torch.bool)}
        if self.labels_are_corrupted:
            out["semantic_non_corrupted"] = load_tensor_from_cls_geotiff(os.path.join(self.semantic_non_corrupted_dp, cls_name))
        if self.semantic_no_cars_dp:
            out["semantic_no_cars"] = load_tensor_from_cls_geotiff(os.path.join(self.semantic_no_cars_dp, cls_name))
        return out

    def bank(self, n_classes=None, car_cls_idx=None, seed=0):
        return super().bank(n_classes=self.semantic_n_classes, car_cls_idx=self.car_cls_idx, seed=seed)
