"""Host definitions of the heart-mask clean-up and the organ masking of the masked evaluation.

Reference: modify_heart_mask.py:87-198 (modify_heart_label) and masking.py:455-512 / :526-530
(organ_mask, apply_organ_mask).  The reference goes through cv2 and nibabel, which are not
installed here; the rules are restated in numpy / scipy.ndimage, these functions are the
definition, and the device path (modules/hip/organ_masks.py) equals them bit for bit.

The two line brushes are the discs OpenCV's thick-line code stamps for thickness 2 and 4, as read
from its drawing code; parity with cv2's rasteriser is unpinned.  They are kept as the two tables
below so that someone with cv2 can pin or correct them in one place (the device reads its brush
offsets from these tables too).
"""
from __future__ import annotations

import numpy as np
from scipy import ndimage

# masking.py:390 (TotalSegmentator classes: organs 1-9, 15, 18-24, heart 51, vessels 52-68 less 53)
MASK_TARGET_LABELS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 18, 19, 20, 21, 22, 23, 24, 51, 52, 54, 55, 56, 57, 58, 59, 60,
                      61, 62, 63, 64, 65, 66, 67, 68)
HEART_LABEL = 51
MASK_FILL = 9999

BRUSH_2 = np.array([[0, 1, 0],
                    [1, 1, 1],
                    [0, 1, 0]], dtype=np.uint8)            # drawContours(thickness=2)
BRUSH_4 = np.array([[0, 1, 1, 1, 0],
                    [1, 1, 1, 1, 1],
                    [1, 1, 1, 1, 1],
                    [1, 1, 1, 1, 1],
                    [0, 1, 1, 1, 0]], dtype=np.uint8)      # drawContours(thickness=4)


def brush_offsets(table: np.ndarray):
    """The (dy, dx) offsets of a brush table's set pixels from its centre, in raster order."""
    table = np.asarray(table)
    if table.ndim != 2 or table.shape[0] != table.shape[1] or table.shape[0] % 2 != 1:
        raise ValueError("brush table: odd square required")
    c = table.shape[0] // 2
    return [(int(i) - c, int(j) - c) for i, j in zip(*np.nonzero(table))]


# ---------------------------------------------------------------------------------------------
# heart clean-up
# ---------------------------------------------------------------------------------------------
def modify_heart_label(labels_xyz: np.ndarray, *, heart_label: int = HEART_LABEL, gap_threshold: int = 2,
                       offset: float = 1.15, offset_y_base: float = 1.4, offset_z: float = 2.65,
                       min_region: int = 1024) -> np.ndarray:
    """modify_heart_mask.py:87-198 on a label volume indexed [x, y, z]; returns the uint8 volume
    with the heart label cut back.  The constants are the reference's; they are arguments so that
    small volumes can be tested.

    Two deviations from the reference, which crashes or is ambiguous there: a volume without the
    heart label is returned unchanged (the reference raises on np.min of an empty array), and among
    components whose centres tie in z the first in ndimage.label's numbering wins (the
    lexicographic order of the first voxel in [x, y, z]; it is what the stable sort gives)."""
    if gap_threshold < 1:
        raise ValueError("gap_threshold must be >= 1")
    mask_volume = np.array(labels_xyz).astype(np.uint8)
    if mask_volume.ndim != 3:
        raise ValueError("modify_heart_label: a three-dimensional label volume is required")
    heart_mask = (mask_volume == heart_label).astype(np.uint8)
    if not heart_mask.any():
        return mask_volume
    labeled, num = ndimage.label(heart_mask)
    centers = ndimage.center_of_mass(heart_mask, labeled, range(1, num + 1))
    centers.sort(key=lambda c: c[2])
    x, y, z = centers[0]
    nz = heart_mask.shape[2]

    # column gap cut: scanning z upward from start_z, at the first run of gap_threshold zeros
    # the column is cleared from the run's first voxel on
    start_z = int(z)
    zero = heart_mask[:, :, start_z:] == 0
    nwin = zero.shape[2] - gap_threshold + 1
    if nwin > 0:
        run = np.ones(zero.shape[:2] + (nwin,), dtype=bool)
        for g in range(gap_threshold):
            run &= zero[:, :, g:g + nwin]
        cut = np.where(run.any(axis=2), start_z + run.argmax(axis=2), nz)
        heart_mask[np.arange(nz)[None, None, :] >= cut[:, :, None]] = 0

    # anisotropic distance test around the lowest component's centre
    nonzero_i, nonzero_j = np.nonzero(heart_mask[:, :, int(z)])
    if len(nonzero_i) > 0:
        distances_slice = np.sqrt((nonzero_i - x) ** 2 + (nonzero_j - y) ** 2)
        max_distance = np.max(distances_slice) * offset
        i_idx, j_idx, k_idx = np.nonzero(heart_mask)
        x_distances = i_idx - x
        y_distances = j_idx - y
        z_distances = k_idx - z
        offset_y_variable = 1 + (offset_y_base - 1) * np.abs(x_distances) / (np.max(np.abs(x_distances)) + 1e-5)
        distances = np.sqrt((i_idx - x) ** 2 +
                            np.where((y_distances > 0) & (z_distances > 0), (y_distances * offset_y_variable) ** 2,
                                     y_distances ** 2) +
                            np.where(z_distances > 0, (z_distances * offset_z) ** 2, z_distances ** 2))
        remove = distances >= max_distance
        heart_mask[i_idx[remove], j_idx[remove], k_idx[remove]] = 0

    # small regions
    labeled, num = ndimage.label(heart_mask)
    if num:
        sizes = np.bincount(labeled.ravel(), minlength=num + 1)
        small = sizes < min_region
        small[0] = False
        heart_mask[small[labeled]] = 0

    mask_volume[mask_volume == heart_label] = 0
    mask_volume[heart_mask == 1] = heart_label
    return mask_volume


# ---------------------------------------------------------------------------------------------
# organ mask
# ---------------------------------------------------------------------------------------------
def outside_background(s: np.ndarray) -> np.ndarray:
    """The background of the set ``s`` [H, W] that a 4-connected path joins to the padded border."""
    pad = np.pad(~np.asarray(s, dtype=bool), 1, constant_values=True)
    lab, _ = ndimage.label(pad)
    return lab == lab[0, 0]                                  # [H + 2, W + 2], the border ring included


def outer_boundary(s: np.ndarray, outside_padded: np.ndarray) -> np.ndarray:
    """Pixels of ``s`` with a 4-neighbour (or the image edge) in the outside background."""
    o = outside_padded
    return np.asarray(s, dtype=bool) & (o[:-2, 1:-1] | o[2:, 1:-1] | o[1:-1, :-2] | o[1:-1, 2:])


def stamp(points: np.ndarray, brush: np.ndarray) -> np.ndarray:
    """The brush stamped at every set pixel of ``points``, clipped to the image."""
    h, w = points.shape
    out = np.zeros((h, w), dtype=bool)
    for dy, dx in brush_offsets(brush):
        ys, yd = (slice(0, h - dy), slice(dy, h)) if dy >= 0 else (slice(-dy, h), slice(0, h + dy))
        xs, xd = (slice(0, w - dx), slice(dx, w)) if dx >= 0 else (slice(-dx, w), slice(0, w + dx))
        out[yd, xd] |= points[ys, xs]
    return out


def organ_mask_slice(labels_yx: np.ndarray, target_labels=MASK_TARGET_LABELS) -> np.ndarray:
    labels_yx = np.asarray(labels_yx)
    union = np.zeros(labels_yx.shape, dtype=bool)
    present = set(np.unique(labels_yx).tolist())
    for label in target_labels:
        if label not in present:
            continue
        filled = ndimage.binary_fill_holes(labels_yx == label)      # external contour, thickness=-1
        edge = outer_boundary(filled, outside_background(filled))
        union |= filled | stamp(edge, BRUSH_2)                       # the same contour, thickness=2
    edge = outer_boundary(union, outside_background(union))          # external contour of the union
    return union | stamp(edge, BRUSH_4)                              # drawn as a line only, thickness=4


def organ_mask(labels_zyx: np.ndarray, target_labels=MASK_TARGET_LABELS) -> np.ndarray:
    """masking.py:455-512 on a label volume indexed [z, y, x]: per slice, every target label's
    external contours filled and drawn with thickness 2, then the external contours of the union
    drawn with thickness 4.  Returns the uint8 0/1 mask [z, y, x]."""
    labels_zyx = np.asarray(labels_zyx)
    if labels_zyx.ndim != 3:
        raise ValueError("organ_mask: a [z, y, x] label volume is required")
    out = np.zeros(labels_zyx.shape, dtype=np.uint8)
    for z in range(labels_zyx.shape[0]):
        out[z] = organ_mask_slice(labels_zyx[z], target_labels)
    return out


def apply_organ_mask(series_int16: np.ndarray, mask: np.ndarray, fill: int = MASK_FILL) -> np.ndarray:
    """masking.py:526-541: a copy of the stored series with the masked pixels set to ``fill``."""
    series_int16 = np.asarray(series_int16)
    if series_int16.dtype != np.int16:
        raise ValueError("apply_organ_mask: an int16 series is required")
    if series_int16.shape != np.asarray(mask).shape:
        raise ValueError(f"apply_organ_mask: series {series_int16.shape} and mask {np.asarray(mask).shape} differ")
    out = series_int16.copy()
    out[np.asarray(mask) != 0] = np.int16(fill)
    return out
