"""The re-indexed dataset layer -- morefusion/datasets/rgbd_pose_estimation/{reindex,reindexed}.py.

``reindex`` walks frame datasets (``RGBDPoseEstimationDatasetBase``) and writes one compressed npz per example,
``<root>/<image_id>/<k:08d>.npz``, plus ``<root>/meta.json`` (instance id -> class_id, visibility): the
reference's layout.  It runs in the calling process; the reference's process pool would open the GPU from many
processes.  ``RGBDPoseEstimationDatasetReIndexedBase`` reads that tree back one example per index, and
``get_examples`` loads a minibatch and augments it in ONE ``augment_rgbd`` call on the device -- the path a
training loop should take.
"""
import collections
import json
import os

import numpy as np
import torch

from .augmentation import _random_state, augment_rgbd


def reindex(root_dir, datasets):
    """Write every example of every dataset under ``root_dir``; returns the id -> meta dict of ``meta.json``."""
    root_dir = str(root_dir)
    id_to_meta = {}
    for ds in datasets:
        for index in range(len(ds)):
            image_id = str(ds._ids[index])
            for k, example in enumerate(ds.get_example(index)):
                instance_id = f"{image_id}/{k:08d}"
                npz_file = os.path.join(root_dir, instance_id + ".npz")
                os.makedirs(os.path.dirname(npz_file), exist_ok=True)
                np.savez_compressed(npz_file, **example)
                id_to_meta[instance_id] = {"class_id": int(example["class_id"]),
                                           "visibility": float(example["visibility"])}
    os.makedirs(root_dir, exist_ok=True)
    with open(os.path.join(root_dir, "meta.json"), "w") as f:
        json.dump(id_to_meta, f, indent=4)
    return id_to_meta


class RGBDPoseEstimationDatasetReIndexedBase:
    """Examples of a ``reindex`` tree.  ``split``: kept for the reference's signature; a subclass that has splits
    overrides ``_get_image_ids`` (the reference asks the frame dataset of the split for its ids).  ``random_state``
    seeds the augmentation (an int or a ``numpy.random.RandomState``; default: NumPy's global generator)."""

    def __init__(self, root_dir, split=None, class_ids=None, augmentation=False, device="cuda", random_state=None):
        self.root_dir = str(root_dir)
        if not os.path.isdir(self.root_dir):
            raise IOError(f"{self.root_dir} does not exist. ")
        self._class_ids = None if class_ids is None else tuple(class_ids)
        self._split = split
        self._augmentation = augmentation
        self._device = torch.device(device)
        self._random_state = _random_state(random_state)
        self._ids = self._get_ids()

    def _get_image_ids(self, image_id_to_instance_ids):
        return list(image_id_to_instance_ids)  # meta.json order: the order reindex wrote the frames in

    def _get_ids(self):
        image_id_to_instance_ids = collections.defaultdict(list)
        with open(os.path.join(self.root_dir, "meta.json")) as f:
            instance_id_to_meta = json.load(f)
        for instance_id in instance_id_to_meta:
            image_id_to_instance_ids[os.path.dirname(instance_id)].append(instance_id)
        image_id_to_instance_ids = dict(image_id_to_instance_ids)
        ids = []
        for image_id in self._get_image_ids(image_id_to_instance_ids):
            for instance_id in image_id_to_instance_ids.get(image_id, ()):
                class_id = instance_id_to_meta[instance_id]["class_id"]
                if self._class_ids and class_id not in self._class_ids:
                    continue
                ids.append(instance_id)
        self._image_id_to_instance_ids = image_id_to_instance_ids
        return ids

    def __len__(self):
        return len(self._ids)

    def get_indices_from_image_id(self, image_id):
        indices = []
        for id in self._image_id_to_instance_ids[image_id]:
            try:
                indices.append(self._ids.index(id))
            except ValueError:
                pass
        return indices

    def _load(self, index):
        example = dict(np.load(os.path.join(self.root_dir, self._ids[index] + ".npz")))
        example.pop("visibility", None)
        return example

    def get_examples(self, indices):
        """The examples of ``indices``; with augmentation their rgb / pcd go through one ``augment_rgbd`` call."""
        examples = [self._load(i) for i in indices]
        if self._augmentation and examples:
            rgb = torch.from_numpy(np.stack([e["rgb"] for e in examples])).to(self._device)
            pcd = torch.from_numpy(np.stack([e["pcd"] for e in examples])).to(self._device)
            rgb, pcd, _ = augment_rgbd(rgb, pcd, self._random_state)
            rgb, pcd = rgb.cpu().numpy(), pcd.cpu().numpy()
            for k, e in enumerate(examples):
                e["rgb"], e["pcd"] = rgb[k], pcd[k]
        return examples

    def get_example(self, index):
        return self.get_examples([index])[0]

    def __getitem__(self, index):
        if isinstance(index, (list, tuple, np.ndarray)):
            return self.get_examples(list(index))
        return self.get_example(index)
