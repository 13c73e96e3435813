"""csrc/organ_masks.hip against the host definitions (modules/organ_masks.py) and scipy, bit for bit."""
import numpy as np
import pytest
import torch
from scipy import ndimage

import organ_mask_cases as cases
from modules import dicom, nifti
from modules import organ_masks as OM

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def G():
    from modules.hip import organ_masks
    return organ_masks


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---------------------------------------------------------------------------------------------
# 3-D labelling
# ---------------------------------------------------------------------------------------------
def check_labelling(G, vol_zyx):
    """The device partition equals ndimage.label's (6-connectivity) up to renumbering, with equal
    sizes, centres of mass (float64 equality) and first voxels in [x, y, z] raster order."""
    D, H, W = vol_zyx.shape
    labels, count, sums, keys = (t.cpu().numpy() for t in G.label3d(dev(vol_zyx)))
    want, n = ndimage.label(vol_zyx)
    flat, wflat = labels.ravel(), want.ravel()
    assert np.array_equal(flat >= 0, wflat > 0)
    roots = np.flatnonzero(flat == np.arange(flat.size))
    assert len(roots) == n
    if n == 0:
        return 0
    fg = flat >= 0
    assert (flat[flat[fg]] == flat[fg]).all()                       # every label is a root
    pairs = np.unique(np.stack([flat[fg], wflat[fg]]), axis=1)
    assert pairs.shape[1] == n and len(set(pairs[0])) == n and len(set(pairs[1])) == n
    to_root = np.zeros(n + 1, dtype=np.int64)
    to_root[pairs[1]] = pairs[0]
    r = to_root[1:]
    u, first_index = np.unique(wflat, return_index=True)
    assert np.array_equal(r, first_index[u > 0])                    # a root is its component's first voxel
    assert np.array_equal(count[r], np.bincount(wflat, minlength=n + 1)[1:])
    com = np.array(ndimage.center_of_mass(vol_zyx, want, range(1, n + 1)))       # (z, y, x)
    cnt = count[r].astype(np.float64)
    for axis, plane in ((2, 0), (1, 1), (0, 2)):
        assert np.array_equal(sums[plane][r].astype(np.float64) / cnt, com[:, axis])
    z, y, x = np.nonzero(vol_zyx)
    key = (x.astype(np.int64) * H + y) * D + z
    first = np.full(n + 1, np.iinfo(np.int64).max)
    np.minimum.at(first, want[z, y, x], key)
    assert np.array_equal(keys[r], first[1:])
    return n


@pytest.mark.parametrize("p", [0.25, 0.31, 0.40])
def test_label3d_random_occupancy_around_percolation(G, p):
    rng = np.random.default_rng(int(p * 100))
    vol = (rng.random((33, 66, 70)) < p).astype(np.uint8)           # [x, y, z] = 70 x 66 x 33
    assert check_labelling(G, vol) > 1


def test_label3d_serpentine_through_every_brick(G):
    D, H, W = 21, 35, 37
    vol = np.zeros((D, H, W), dtype=np.uint8)
    ys = list(range(0, H, 2))
    for z in range(0, D, 2):                                         # a boustrophedon in every other plane ...
        for yi, y in enumerate(ys):
            vol[z, y, :] = 1
            if yi + 1 < len(ys):
                vol[z, y + 1, W - 1 if yi % 2 == 0 else 0] = 1
        if z + 2 < D:
            vol[z + 1, 0, 0] = 1                                     # ... joined to the next by one voxel
    assert check_labelling(G, vol) == 1
    snake = np.zeros((40, 40, 40), dtype=np.uint8)                   # one path: along x, turn in y, climb in z
    snake[5, 5, 2:38] = 1
    snake[5, 5:38, 37] = 1
    snake[5:38, 37, 37] = 1
    snake[37, 37, 2:38] = 1
    assert check_labelling(G, snake) == 1


def test_label3d_component_across_brick_faces_in_all_axes(G):
    vol = np.zeros((40, 41, 42), dtype=np.uint8)
    vol[20, 20, :] = 1
    vol[20, :, 20] = 1
    vol[:, 20, 20] = 1
    vol[15:18, 15:18, 15:18] = 1                                     # straddles the 16-voxel faces, separate
    vol[31:33, 0:2, 31:33] = 1
    vol[0, 0, 0] = 1
    vol[39, 40, 41] = 1
    assert check_labelling(G, vol) == 5


def test_label3d_full_empty_and_columns(G):
    assert check_labelling(G, np.ones((17, 18, 19), dtype=np.uint8)) == 1
    assert check_labelling(G, np.zeros((17, 18, 19), dtype=np.uint8)) == 0
    col = np.ones(100, dtype=np.uint8)
    col[[16, 47, 48, 95]] = 0
    assert check_labelling(G, col.reshape(100, 1, 1)) == 4            # 1 x 1 x N: z is the long axis
    assert check_labelling(G, col.reshape(1, 1, 100)) == 4
    assert check_labelling(G, col.reshape(1, 100, 1)) == 4
    # another value than 1 is matched exactly
    vol = np.zeros((5, 6, 7), dtype=np.uint8)
    vol[1:3, 1:3, 1:3], vol[3:, 3:, 3:] = 51, 52
    labels = G.label3d(dev(vol), match=51)[0].cpu().numpy()
    assert np.array_equal(labels >= 0, vol == 51)


# ---------------------------------------------------------------------------------------------
# heart clean-up
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,vol,kwargs", [
    ("phantom", cases.heart_phantom(), cases.HEART_PHANTOM_ARGS),
    ("tie", cases.heart_tie(), cases.HEART_TIE_ARGS),
    ("no heart", cases.heart_none(), {}),
    ("soup 1", cases.heart_soup(1), dict(min_region=8)),
    ("soup 2", cases.heart_soup(2, p=0.28), dict(min_region=8)),
    ("other constants", cases.heart_phantom(), dict(min_region=3, gap_threshold=3, offset=1.0, offset_y_base=2.0,
                                                    offset_z=1.5)),
])
def test_modify_heart_label_equals_the_host(G, name, vol, kwargs):
    want = OM.modify_heart_label(vol, **kwargs)                       # [x, y, z]
    got = G.modify_heart_label(dev(vol.T), **kwargs).cpu().numpy().T
    assert got.dtype == np.uint8 and np.array_equal(got, want), name
    if name in ("phantom", "tie"):
        assert 0 < (want == 51).sum() < (vol == 51).sum()


# ---------------------------------------------------------------------------------------------
# organ mask
# ---------------------------------------------------------------------------------------------
def organ_soup(seed, shape=(5, 64, 64)):
    """Blobs of all 34 labels (and a few foreign ones) with holes, from a smoothed random field."""
    rng = np.random.default_rng(seed)
    field = ndimage.uniform_filter(rng.random(shape), size=(1, 5, 5))
    which = np.kron(rng.integers(0, 40, (shape[0], shape[1] // 8, shape[2] // 8)), np.ones((1, 8, 8), dtype=np.int64))
    labels = np.array(list(OM.MASK_TARGET_LABELS) + [10, 53, 200, 0, 0, 0], dtype=np.uint8)[which]
    vol = np.where(field > 0.5, labels, 0).astype(np.uint8)
    vol[rng.random(shape) < 0.03] = 0                                # pin holes
    for i, label in enumerate(OM.MASK_TARGET_LABELS):                # every label at least once
        vol[-1, 3 * (i // 16):3 * (i // 16) + 2, 4 * (i % 16):4 * (i % 16) + 2] = label
    return vol


@pytest.mark.parametrize("h,w", [(96, 100), (130, 77)])
def test_organ_mask_cases_equal_the_host(G, h, w):
    vol = cases.organ_cases(h, w)
    want = OM.organ_mask(vol)
    assert np.array_equal(G.organ_mask(dev(vol)).cpu().numpy(), want)
    assert np.array_equal(G.organ_mask(dev(vol), chunk=1).cpu().numpy(), want)


def test_organ_mask_soup_and_chunks(G):
    vol = organ_soup(3)
    assert len(set(np.unique(vol)) & set(OM.MASK_TARGET_LABELS)) == 34
    want = OM.organ_mask(vol)
    assert 0 < want.sum() < want.size
    for chunk in (None, 1, 2, 5):
        assert np.array_equal(G.organ_mask(dev(vol), chunk=chunk).cpu().numpy(), want), chunk
    few = (1, 51, 68)
    assert np.array_equal(G.organ_mask(dev(vol), target_labels=few).cpu().numpy(), OM.organ_mask(vol, few))


def test_organ_mask_mostly_absent_pairs(G):
    vol = np.zeros((7, 70, 90), dtype=np.uint8)
    vol[2, 10:40, 10:50] = 51
    vol[2, 20:30, 20:40] = 0
    vol[5, 60:70, 80:90] = 3
    vol[6, 0:3, 0:3] = 10                                            # a foreign label alone in its slice
    want = OM.organ_mask(vol)
    got = G.organ_mask(dev(vol)).cpu().numpy()
    assert np.array_equal(got, want) and not got[[0, 1, 3, 4, 6]].any() and got[2].any() and got[5].any()
    assert not G.organ_mask(dev(np.zeros((2, 33, 35), dtype=np.uint8))).any()


def test_apply_equals_the_host(G):
    rng = np.random.default_rng(9)
    shape = (3, 37, 41)
    series = [rng.integers(-32768, 32767, shape, endpoint=True).astype(np.int16) for _ in range(3)]
    series[0][0, 0, :4] = [9999, -9999, -32768, 32767]
    mask = (rng.random(shape) < 0.3).astype(np.uint8)
    mask[0, 0, :4] = [1, 1, 0, 1]
    mask[1, 1, 1] = 255                                               # any non-zero value masks
    got = G.apply_organ_mask(*(dev(s) for s in series), dev(mask))
    for g, s in zip(got, series):
        assert g.dtype == torch.int16 and np.array_equal(g.cpu().numpy(), OM.apply_organ_mask(s, mask))
    got = G.apply_organ_mask(*(dev(s) for s in series), dev(mask), fill=-5)
    assert np.array_equal(got[2].cpu().numpy(), OM.apply_organ_mask(series[2], mask, fill=-5))


# ---------------------------------------------------------------------------------------------
# entry points
# ---------------------------------------------------------------------------------------------
def _tree_bytes(root):
    return {str(p.relative_to(root)): p.read_bytes() for p in sorted(root.rglob("*")) if p.is_file()}


def test_masking_and_modify_heart_mask_write_the_same_bytes_on_both_devices(tmp_path, monkeypatch):
    import masking
    import modify_heart_mask
    monkeypatch.chdir(tmp_path)                                          # the common arguments create ./data
    trees = {}
    for device in ("cpu", "cuda"):
        root = tmp_path / device
        cases.build_masking_tree(root, dicom, nifti, patients=("P1", "P2"))
        src = root / "out" / "mask" / "DS"
        src.mkdir(parents=True)
        nifti.write_volume(str(src / "P1.nii"), cases.heart_phantom(), pixdim=(0.7, 0.7, 2.5))
        argv = ["--input_dir_root", str(root / "in"), "--output_dir_root", str(root / "out"), "--dataset_names", "DS",
                "--device", device]
        masking.main(argv)
        (root / "out" / "modified_mask" / "DS" / "P1.nii").unlink()
        modify_heart_mask.main(argv)
        trees[device] = {**_tree_bytes(root / "out" / "masked"),
                         "heart": (root / "out" / "modified_mask" / "DS" / "P1.nii").read_bytes()}
    assert len(trees["cpu"]) == 2 * 3 * 6 + 1 and trees["cpu"].keys() == trees["cuda"].keys()
    for name, data in trees["cpu"].items():
        assert data == trees["cuda"][name], name


# ---------------------------------------------------------------------------------------------
# bad arguments
# ---------------------------------------------------------------------------------------------
def test_bad_arguments_raise(G):
    from modules.hip import lib
    vol = np.zeros((4, 8, 8), dtype=np.uint8)
    series = torch.zeros((4, 8, 8), dtype=torch.int16, device=DEV)
    for fn in (G.label3d, G.modify_heart_label, G.organ_mask):
        with pytest.raises(RuntimeError, match="device tensor"):
            fn(torch.from_numpy(vol))                                 # host tensor
        with pytest.raises(RuntimeError, match="< 256"):
            fn(dev(vol.astype(np.int16)))                             # a dtype that can hold labels >= 256
        with pytest.raises(ValueError):
            fn(dev(vol)[0])
    with pytest.raises(RuntimeError, match="device tensor"):
        G.apply_organ_mask(series.cpu(), series, series, dev(vol))
    with pytest.raises(RuntimeError, match="device tensor"):
        G.apply_organ_mask(series, series, series, torch.from_numpy(vol))
    with pytest.raises(RuntimeError, match="int16"):
        G.apply_organ_mask(series.int(), series, series, dev(vol))
    with pytest.raises(ValueError):
        G.apply_organ_mask(series, series, series[:2], dev(vol))
    with pytest.raises(ValueError, match="< 256"):
        G.organ_mask(dev(vol), target_labels=(1, 256))
    with pytest.raises(ValueError, match="< 256"):
        G.modify_heart_label(dev(vol), heart_label=300)
    with pytest.raises(ValueError, match="< 256"):
        G.label3d(dev(vol), match=-1)
    # oversize: refused from the shape alone, by the wrapper's query and by the entry points themselves
    assert G.heart_workspace_size((2048, 1024, 1024)) == 0
    assert G.organ_mask_workspace_size((2048, 1024, 1024), 34, 1) == 0
    assert G.organ_mask_workspace_size((64, 512, 512), 34, 300) == 0           # chunk * labels * H * W >= 2^31
    assert G.organ_mask_workspace_size((4, 8, 8), 34, 2000) == 0               # more images than the grid takes
    v, out = dev(vol), torch.empty(4 * 8 * 8, dtype=torch.uint8, device=DEV)
    ws = torch.empty(1 << 16, dtype=torch.int64, device=DEV)
    P, nbytes = lib.ptr, ws.numel() * 8
    with pytest.raises(lib.HipLibraryError, match="too large"):
        lib.call("dcs_heart_modify", P(v), 2048, 1024, 1024, 51, 2, 1.15, 0.4, 2.65, 1024, P(out), P(ws), nbytes,
                 lib.stream())
    with pytest.raises(lib.HipLibraryError, match="too large"):
        lib.call("dcs_cc3_label", P(v), 1, 2048, 1024, 1024, P(ws), P(ws), None, None, lib.stream())
    import ctypes
    tl, b = (ctypes.c_int32 * 1)(5), (ctypes.c_int8 * 2)(0, 0)
    with pytest.raises(lib.HipLibraryError, match="dimensions"):
        lib.call("dcs_organ_mask", P(v), 2048, 1024, 1024, tl, 1, b, 1, b, 1, 1, P(out), P(ws), nbytes, lib.stream())
    with pytest.raises(lib.HipLibraryError, match="< 256"):
        lib.call("dcs_organ_mask", P(v), 4, 8, 8, (ctypes.c_int32 * 1)(256), 1, b, 1, b, 1, 1, P(out), P(ws), nbytes,
                 lib.stream())
    with pytest.raises(lib.HipLibraryError, match="brush"):
        lib.call("dcs_organ_mask", P(v), 4, 8, 8, tl, 1, (ctypes.c_int8 * 2)(0, 3), 1, b, 1, 1, P(out), P(ws), nbytes,
                 lib.stream())
    # short workspace
    small = torch.empty(8, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match="workspace too small"):
        G.modify_heart_label(v, workspace=small)
    with pytest.raises(ValueError, match="workspace too small"):
        G.organ_mask(v, workspace=small)
    with pytest.raises(lib.HipLibraryError, match="workspace too small"):
        lib.call("dcs_heart_modify", P(v), 4, 8, 8, 51, 2, 1.15, 0.4, 2.65, 1024, P(out), P(small), 64, lib.stream())
    with pytest.raises(lib.HipLibraryError, match="workspace too small"):
        lib.call("dcs_organ_mask", P(v), 4, 8, 8, tl, 1, b, 1, b, 1, 1, P(out), P(small), 64, lib.stream())
    # and a supplied workspace of the right size is used
    big = torch.empty(G.heart_workspace_size(vol.shape) // 8 + 1, dtype=torch.int64, device=DEV)
    assert np.array_equal(G.modify_heart_label(v, workspace=big).cpu().numpy(), vol)
