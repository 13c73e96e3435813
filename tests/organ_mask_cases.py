"""Phantoms and independent restatements shared by test_cpu_organ_masks.py and
test_gpu_organ_masks.py (plain Python loops and float64 scalars; no scipy, no package code)."""
import math
from collections import deque

import numpy as np

BRUSH_CROSS = [(0, 0), (-1, 0), (1, 0), (0, -1), (0, 1)]
BRUSH_ROUND5 = [(dy, dx) for dy in range(-2, 3) for dx in range(-2, 3) if abs(dy) + abs(dx) < 4]
TARGETS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 18, 19, 20, 21, 22, 23, 24, 51, 52, 54, 55, 56, 57, 58, 59, 60, 61, 62, 63,
           64, 65, 66, 67, 68)


# ---------------------------------------------------------------------------------------------
# heart phantoms, indexed [x, y, z]
# ---------------------------------------------------------------------------------------------
def heart_phantom():
    """40x36x24: an ellipsoid of label 51, a stalk rising in +z with a two-voxel gap, a detached
    crumb below min_region, and two other labels that must come through untouched."""
    v = np.zeros((40, 36, 24), dtype=np.uint8)
    v[2:8, 2:9, 1:20] = 3
    v[30:38, 25:34, 3:9] = 52
    x, y, z = np.mgrid[0:40, 0:36, 0:24]
    v[((x - 20) / 9.0) ** 2 + ((y - 18) / 8.0) ** 2 + ((z - 9) / 6.0) ** 2 <= 1.0] = 51
    v[19:22, 17:20, 15:24] = 51          # the stalk ...
    v[19:22, 17:20, 18:20] = 0           # ... with its two-voxel gap
    v[20:22, 8:9, 10:11] = 51            # the crumb: beside the body, two voxels
    return v


HEART_PHANTOM_ARGS = dict(min_region=16)


def heart_tie():
    """Two equal blobs whose centres tie in z: the one that starts first in [x, y, z] raster order
    is the reference point, so it is the far top of the other one that the distance test removes."""
    v = np.zeros((30, 20, 12), dtype=np.uint8)
    v[16:22, 4:10, 1:10] = 51
    v[4:10, 11:17, 1:10] = 51
    v[0:3, 0:3, 0:3] = 7
    return v


HEART_TIE_ARGS = dict(min_region=8)


def heart_none():
    v = np.zeros((9, 8, 7), dtype=np.uint8)
    v[2:5, 2:6, 1:4] = 52
    v[6:8, 1:3, 4:6] = 3
    return v


def heart_soup(seed, shape=(37, 29, 21), p=0.35):
    rng = np.random.default_rng(seed)
    v = np.where(rng.random(shape) < p, 51, 0).astype(np.uint8)
    v[rng.random(shape) < 0.05] = 3
    return v


def _label6(mask):
    """Flood-fill labelling, 6-connectivity, numbered by the first voxel in [x, y, z] raster order."""
    nx, ny, nz = mask.shape
    lab = np.zeros(mask.shape, dtype=np.int64)
    comps = []
    for x in range(nx):
        for y in range(ny):
            for z in range(nz):
                if not mask[x, y, z] or lab[x, y, z]:
                    continue
                comps.append([])
                n = len(comps)
                lab[x, y, z] = n
                q = deque([(x, y, z)])
                while q:
                    a, b, c = q.popleft()
                    comps[-1].append((a, b, c))
                    for da, db, dc in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)):
                        u, w, t = a + da, b + db, c + dc
                        if 0 <= u < nx and 0 <= w < ny and 0 <= t < nz and mask[u, w, t] and not lab[u, w, t]:
                            lab[u, w, t] = n
                            q.append((u, w, t))
    return comps


def modify_heart_loops(vol, heart_label=51, gap_threshold=2, offset=1.15, offset_y_base=1.4, offset_z=2.65,
                       min_region=1024):
    """modify_heart_mask.py:87-198 voxel by voxel.  Returns (volume, voxels removed by the gap cut,
    by the distance test, by the size filter)."""
    vol = vol.astype(np.uint8).copy()
    nx, ny, nz = vol.shape
    heart = [[[1 if vol[x, y, z] == heart_label else 0 for z in range(nz)] for y in range(ny)] for x in range(nx)]
    comps = _label6(vol == heart_label)
    if not comps:
        return vol, 0, 0, 0
    centers = []
    for comp in comps:
        n = float(len(comp))
        centers.append((float(sum(c[0] for c in comp)) / n, float(sum(c[1] for c in comp)) / n,
                        float(sum(c[2] for c in comp)) / n))
    best = 0
    for k in range(1, len(centers)):
        if centers[k][2] < centers[best][2]:      # strict: the earlier one keeps a tie
            best = k
    cx, cy, cz = centers[best]
    start_z = int(cz)
    cut = 0
    for x in range(nx):
        for y in range(ny):
            gap = 0
            for z in range(start_z, nz):
                gap = gap + 1 if heart[x][y][z] == 0 else 0
                if gap >= gap_threshold:
                    for zz in range(z - gap + 1, nz):
                        cut += heart[x][y][zz]
                        heart[x][y][zz] = 0
                    break
    far = 0
    zc = int(cz)
    plane = [math.sqrt((x - cx) ** 2 + (y - cy) ** 2) for x in range(nx) for y in range(ny) if heart[x][y][zc]]
    if plane:
        max_distance = max(plane) * offset
        voxels = [(x, y, z) for x in range(nx) for y in range(ny) for z in range(nz) if heart[x][y][z]]
        max_adx = max(abs(x - cx) for x, _, _ in voxels)
        for x, y, z in voxels:
            dx, dy, dz = x - cx, y - cy, z - cz
            oyv = 1 + (offset_y_base - 1) * abs(dx) / (max_adx + 1e-5)
            ty = (dy * oyv) ** 2 if (dy > 0 and dz > 0) else dy ** 2
            tz = (dz * offset_z) ** 2 if dz > 0 else dz ** 2
            if math.sqrt(dx ** 2 + ty + tz) >= max_distance:
                heart[x][y][z] = 0
                far += 1
    small = 0
    for comp in _label6(np.array(heart, dtype=np.uint8) != 0):
        if len(comp) < min_region:
            for x, y, z in comp:
                heart[x][y][z] = 0
                small += 1
    for x in range(nx):
        for y in range(ny):
            for z in range(nz):
                if vol[x, y, z] == heart_label:
                    vol[x, y, z] = 0
                if heart[x][y][z]:
                    vol[x, y, z] = heart_label
    return vol, cut, far, small


# ---------------------------------------------------------------------------------------------
# organ-mask cases, slices indexed [y, x]
# ---------------------------------------------------------------------------------------------
CASE_NAMES = ("ring", "two_label_hole", "edge_pocket", "diagonal", "foreign_label", "far_corner")


def organ_cases(h, w):
    """uint8 [6, h, w] (h, w >= 40): one case per slice, in CASE_NAMES order."""
    assert h >= 40 and w >= 40
    v = np.zeros((len(CASE_NAMES), h, w), dtype=np.uint8)
    # a ring: its hole is filled in stage 1
    v[0, 8:28, 10:30] = 5
    v[0, 12:24, 14:26] = 0
    # a hole of the union between two labels: neither label encloses it
    v[1, 6:30, 6:18] = 1
    v[1, 6:30, 18:30] = 2
    v[1, 11:25, 11:25] = 0
    # a blob on the image edge whose pocket opens onto the edge: not a hole
    v[2, 0:14, 8:26] = 3
    v[2, 0:8, 13:21] = 0
    v[2, 18:34, 0:12] = 6
    v[2, 21:31, 0:8] = 0
    # diagonal-only contact: a diamond outline encloses its inside (8-connected foreground,
    # 4-connected background); two squares that touch at a corner
    for dy in range(-7, 8):
        for dx in range(-7, 8):
            if abs(dy) + abs(dx) == 7:
                v[3, 12 + dy, 14 + dx] = 4
    v[3, 26:30, 26:30] = 8
    v[3, 30:34, 30:34] = 8
    # labels outside the target list are ignored, next to one that is not
    v[4, 5:15, 5:15] = 10
    v[4, 20:30, 20:30] = 53
    v[4, 30:36, 4:10] = 200
    v[4, 18:22, 6:10] = 9
    # a ring against the far corner (rows / columns that depend on h, w)
    v[5, h - 12:h, w - 14:w] = 15
    v[5, h - 8:h - 3, w - 10:w - 4] = 0
    v[5, h // 2, :] = 68
    return v


def _outside(member, h, w):
    """The complement of ``member`` that a 4-connected path joins to the border of the image padded
    by one pixel, as a set of padded coordinates."""
    seen = {(-1, -1)}
    q = deque([(-1, -1)])
    while q:
        y, x = q.popleft()
        for dy, dx in ((1, 0), (-1, 0), (0, 1), (0, -1)):
            u, t = y + dy, x + dx
            if -1 <= u <= h and -1 <= t <= w and (u, t) not in seen:
                if 0 <= u < h and 0 <= t < w and member[u][t]:
                    continue
                seen.add((u, t))
                q.append((u, t))
    return seen


def _line(member, outside, brush, h, w):
    out = set()
    for y in range(h):
        for x in range(w):
            if member[y][x] and any((y + dy, x + dx) in outside for dy, dx in ((1, 0), (-1, 0), (0, 1), (0, -1))):
                for dy, dx in brush:
                    if 0 <= y + dy < h and 0 <= x + dx < w:
                        out.add((y + dy, x + dx))
    return out


def organ_mask_loops(slice_yx, targets=TARGETS):
    h, w = slice_yx.shape
    union = [[False] * w for _ in range(h)]
    for label in targets:
        member = [[bool(slice_yx[y, x] == label) for x in range(w)] for y in range(h)]
        if not any(any(r) for r in member):
            continue
        outside = _outside(member, h, w)
        filled = [[(y, x) not in outside for x in range(w)] for y in range(h)]
        line = _line(filled, outside, BRUSH_CROSS, h, w)
        for y in range(h):
            for x in range(w):
                if filled[y][x] or (y, x) in line:
                    union[y][x] = True
    outside = _outside(union, h, w)
    line = _line(union, outside, BRUSH_ROUND5, h, w)
    return np.array([[1 if union[y][x] or (y, x) in line else 0 for x in range(w)] for y in range(h)], dtype=np.uint8)


# ---------------------------------------------------------------------------------------------
# a tmp tree for masking.py: IN/DS/P*/{POST VUE, POST STD}, OUT/DS/P*, OUT/modified_mask/DS/P*.nii
# ---------------------------------------------------------------------------------------------
def masking_labels():
    """Label volume [z=6, y=32, x=32] of the masking tree."""
    lab = np.zeros((6, 32, 32), dtype=np.uint8)
    lab[:, 6:20, 8:22] = 5
    lab[1:5, 10:16, 12:18] = 0          # a hole in the middle slices
    lab[2:, 22:28, 3:9] = 51
    lab[3, 2:5, 25:30] = 53             # not a target
    return lab


def write_series(folder, vol, order, dicom):
    """Slices of ``vol`` as files whose name order differs from their InstanceNumber order."""
    folder.mkdir(parents=True, exist_ok=True)
    for fi, zi in enumerate(order):
        ds = dicom.new_ct_slice(vol[zi], instance=zi + 1, uid_suffix=f"{zi}")
        ds.ImagePositionPatient = [0.0, 0.0, 2.5 * zi]
        ds.save_as(str(folder / f"{fi:03d}.dcm"))


def masking_series(seed=5):
    rng = np.random.default_rng(seed)
    base = rng.integers(-200, 1500, (6, 32, 32)).astype(np.int16)
    base[0, 0, :4] = [9999, -32768, 32767, -1]
    return {"POST VUE": base, "POST STD": (base + rng.integers(0, 80, base.shape)).astype(np.int16),
            "generated": (base + rng.integers(0, 80, base.shape)).astype(np.int16)}


def build_masking_tree(root, dicom, nifti, patients=("P1",), order=(3, 0, 5, 1, 4, 2)):
    series = masking_series()
    lab = masking_labels()
    for p in patients:
        write_series(root / "in" / "DS" / p / "POST VUE", series["POST VUE"], order, dicom)
        write_series(root / "in" / "DS" / p / "POST STD", series["POST STD"], order, dicom)
        write_series(root / "out" / "DS" / p, series["generated"], order, dicom)
        (root / "out" / "modified_mask" / "DS").mkdir(parents=True, exist_ok=True)
        nifti.write_volume(str(root / "out" / "modified_mask" / "DS" / f"{p}.nii"), np.ascontiguousarray(lab.T))
    return series, lab, order
