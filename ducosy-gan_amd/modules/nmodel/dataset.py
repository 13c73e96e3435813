"""Training data of the normal-map U-Net: the reference's modules/nmodel/dataset.py (CTDiffDataset,
get_dataloaders), restated without scikit-learn.

Layout: ``<data_dir>/vue_files/<id>_vue.npy`` (the input volume in HU, [D,H,W]) and
``<data_dir>/diff_map/<id>_diff.npy`` (the raw difference map, same shape); patients are the
``*_diff.npy`` files in directory-listing order.  A sample of the patch mode is slice
``index % patches_per_volume`` of patient ``index // patches_per_volume`` (clamped to the last slice),
cropped at a random in-plane position to ``patch_size`` and zero-padded when the volume is smaller.

The train / val split is sklearn's ``train_test_split(ids, test_size=val_size, random_state=42)``
written with numpy: ``n_test = ceil(val_size * n)``, the permutation of ``RandomState(42)``, its
first ``n_test`` entries the validation set and the rest the training set.
"""
import math
import os

import numpy as np
import torch
from torch.utils.data import DataLoader, Dataset

HU_RANGE = (-1024, 3071)
DIFF_RANGE = (0, 4000)


def split_ids(ids, val_size=0.15, random_state=42):
    """(train ids, val ids) as sklearn's ShuffleSplit draws them for a float ``val_size``."""
    n = len(ids)
    n_val = int(math.ceil(val_size * n))
    n_train = n - n_val
    if n_train < 1 or n_val < 1:
        raise ValueError(f"With n_samples={n} and test_size={val_size} a split would leave one side empty")
    perm = np.random.RandomState(random_state).permutation(n)
    return [ids[i] for i in perm[n_val:n_val + n_train]], [ids[i] for i in perm[:n_val]]


def _to_unit(v, lo, hi):
    v = np.clip(v, lo, hi)
    v = (v - lo) / (hi - lo)
    return v * 2 - 1


def _from_unit(v, lo, hi):
    v = (v + 1) / 2
    return v * (hi - lo) + lo


def _random_start(extent, size):
    room = max(0, extent - size)
    return np.random.randint(0, room + 1) if room > 0 else 0


def _pad_to(patch, size):
    if patch.shape == tuple(size):
        return patch
    out = np.zeros(tuple(size), dtype=patch.dtype)
    out[:patch.shape[0], :patch.shape[1], :patch.shape[2]] = patch
    return out


class CTDiffDataset(Dataset):
    def __init__(self, data_dir, mode='train', transform=None, val_size=0.15, random_state=42,
                 use_patches=True, patch_size=(64, 512, 512), patches_per_volume=8):
        self.data_dir, self.mode, self.transform = data_dir, mode, transform
        self.use_patches, self.patch_size, self.patches_per_volume = use_patches, tuple(patch_size), patches_per_volume
        files = [f for f in os.listdir(os.path.join(data_dir, 'diff_map')) if f.endswith('_diff.npy')]
        ids = [f.replace('_diff.npy', '') for f in files]
        train_ids, val_ids = split_ids(ids, val_size, random_state)
        if mode == 'train':
            self.patient_ids = train_ids
        elif mode == 'val':
            self.patient_ids = val_ids
        else:
            raise ValueError(f"Unknown mode: {mode}. Only 'train' and 'val' are supported.")
        print(f"[{mode.upper()}] Loaded {len(self.patient_ids)} patients")
        if use_patches:
            print(f"[{mode.upper()}] Using patch-based training: patch_size={self.patch_size}, "
                  f"patches_per_volume={patches_per_volume}")

    def __len__(self):
        return len(self.patient_ids) * (self.patches_per_volume if self.use_patches else 1)

    def extract_random_patch(self, volume, patch_size):
        d, h, w = volume.shape
        pd, ph, pw = patch_size
        z, y, x = _random_start(d, pd), _random_start(h, ph), _random_start(w, pw)
        return _pad_to(volume[z:z + pd, y:y + ph, x:x + pw], patch_size)

    def extract_slice_patch(self, volume, slice_idx, patch_size):
        d, h, w = volume.shape
        pd, ph, pw = patch_size
        slice_idx = min(slice_idx, d - 1)
        z = slice_idx if pd == 1 else min(slice_idx, max(0, d - pd))
        y, x = _random_start(h, ph), _random_start(w, pw)
        return _pad_to(volume[z:z + pd, y:y + ph, x:x + pw], patch_size)

    def __getitem__(self, idx):
        if self.use_patches:
            patient_id, slice_idx = self.patient_ids[idx // self.patches_per_volume], idx % self.patches_per_volume
        else:
            patient_id, slice_idx = self.patient_ids[idx], 0
        vue = np.load(os.path.join(self.data_dir, 'vue_files', f'{patient_id}_vue.npy'))
        diff = np.load(os.path.join(self.data_dir, 'diff_map', f'{patient_id}_diff.npy'))
        if self.use_patches:   # each volume draws its own crop position, as the reference does
            vue = self.extract_slice_patch(vue, slice_idx, self.patch_size)
            diff = self.extract_slice_patch(diff, slice_idx, self.patch_size)
        vue = torch.from_numpy(self.normalize_hu(vue)).float().unsqueeze(0)      # (1, D, H, W)
        diff = torch.from_numpy(self.normalize_diff(diff)).float().unsqueeze(0)
        if self.transform:
            vue, diff = self.transform(vue), self.transform(diff)
        return {'input': vue, 'target': diff, 'patient_id': patient_id}

    @staticmethod
    def normalize_hu(volume, min_hu=HU_RANGE[0], max_hu=HU_RANGE[1]):
        return _to_unit(volume, min_hu, max_hu)

    @staticmethod
    def normalize_diff(diff_map, min_diff=DIFF_RANGE[0], max_diff=DIFF_RANGE[1]):
        return _to_unit(diff_map, min_diff, max_diff)

    @staticmethod
    def denormalize_hu(volume, min_hu=HU_RANGE[0], max_hu=HU_RANGE[1]):
        return _from_unit(volume, min_hu, max_hu)

    @staticmethod
    def denormalize_diff(diff_map, min_diff=DIFF_RANGE[0], max_diff=DIFF_RANGE[1]):
        return _from_unit(diff_map, min_diff, max_diff)


def get_dataloaders(data_dir, batch_size=1, num_workers=4, val_size=0.15, use_patches=True,
                    patch_size=(64, 128, 128), patches_per_volume=8):
    """(train loader, shuffled; val loader, in order) over the two splits of ``data_dir``."""
    def loader(mode, shuffle, ppv):
        ds = CTDiffDataset(data_dir=data_dir, mode=mode, val_size=val_size, use_patches=use_patches,
                           patch_size=patch_size, patches_per_volume=ppv)
        return DataLoader(ds, batch_size=batch_size, shuffle=shuffle, num_workers=num_workers, pin_memory=False,
                          prefetch_factor=2 if num_workers > 0 else None, persistent_workers=False)

    return loader('train', True, patches_per_volume), loader('val', False, patches_per_volume if use_patches else 1)
