"""Host definitions of the heart-mask clean-up and the organ mask (modules/organ_masks.py) against
independent restatements, and masking.py / calculate.py --mask end to end (no GPU)."""
import csv
import math

import numpy as np
import pytest

import organ_mask_cases as cases
from modules import dicom, nifti
from modules import organ_masks as OM


# ---------------------------------------------------------------------------------------------
# heart clean-up
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def phantom_loops():
    return cases.modify_heart_loops(cases.heart_phantom(), **cases.HEART_PHANTOM_ARGS)


def test_tables_are_the_reference_lists():
    assert tuple(OM.MASK_TARGET_LABELS) == cases.TARGETS and len(OM.MASK_TARGET_LABELS) == 34
    assert sorted(OM.brush_offsets(OM.BRUSH_2)) == sorted(cases.BRUSH_CROSS)
    assert sorted(OM.brush_offsets(OM.BRUSH_4)) == sorted(cases.BRUSH_ROUND5) and len(cases.BRUSH_ROUND5) == 21


def test_modify_heart_label_equals_the_voxel_loops_on_the_phantom(phantom_loops):
    want, cut, far, small = phantom_loops
    assert cut >= 1 and far >= 1 and small >= 1, (cut, far, small)      # no stage passes vacuously
    vol = cases.heart_phantom()
    got = OM.modify_heart_label(vol, **cases.HEART_PHANTOM_ARGS)
    assert got.dtype == np.uint8 and got.shape == vol.shape
    assert np.array_equal(got, want)
    assert np.array_equal(got[vol != 51], vol[vol != 51])                # other labels untouched
    assert 0 < (got == 51).sum() == (vol == 51).sum() - cut - far - small
    assert not got[19:22, 17:20, 20:].any()                              # the stalk above its gap
    assert not got[20:22, 8, 10].any()                                   # the crumb


def test_ties_in_z_go_to_the_first_component_in_xyz_order():
    vol = cases.heart_tie()
    want, cut, far, small = cases.modify_heart_loops(vol, **cases.HEART_TIE_ARGS)
    got = OM.modify_heart_label(vol, **cases.HEART_TIE_ARGS)
    assert np.array_equal(got, want)
    # ndimage.label numbers the blob at x = 4 first, so it is the reference point and stays whole; the
    # other one loses its far top (taking it as the reference would do the opposite)
    assert (got[4:10, 11:17, 1:10] == 51).all() and 0 < (got[16:22, 4:10, 1:10] == 51).sum() < 6 * 6 * 9
    assert far >= 1 and cut == 0


def test_a_volume_without_the_heart_label_is_returned_unchanged():
    vol = cases.heart_none()
    got = OM.modify_heart_label(vol)
    assert got.dtype == np.uint8 and np.array_equal(got, vol) and got is not vol
    assert np.array_equal(OM.modify_heart_label(np.zeros((3, 4, 5), dtype=np.uint8)), np.zeros((3, 4, 5)))


def test_soup_volumes_equal_the_voxel_loops():
    for seed in (1, 2):
        vol = cases.heart_soup(seed, shape=(19, 17, 13))
        want = cases.modify_heart_loops(vol, min_region=8)[0]
        assert np.array_equal(OM.modify_heart_label(vol, min_region=8), want)


def test_distance_test_is_greater_or_equal_by_hand():
    """A plus-shaped slab of one voxel thickness at z = 2, arms of length 5 along x and 3 along y,
    centre (10, 10, 2) exactly.  The farthest planar voxel is at distance 5, so max_distance = 5 * offset.
    With offset 0.8 the bound is 4.0: the voxels at |dx| = 4 sit exactly on it and go (>=), |dx| = 3
    stay; along y (dz = 0, so no y scaling) |dy| = 3 < 4 stays."""
    vol = np.zeros((21, 21, 5), dtype=np.uint8)
    vol[5:16, 10, 2] = 51
    vol[10, 7:14, 2] = 51
    got = OM.modify_heart_label(vol, offset=0.8, min_region=1)
    assert 5 * 0.8 == 4.0 and math.sqrt(16.0) == 4.0
    kept_x = [x for x in range(21) if got[x, 10, 2] == 51]
    assert kept_x == [7, 8, 9, 10, 11, 12, 13]                # |dx| <= 3 kept, |dx| = 4 (== bound) and 5 removed
    assert [y for y in range(21) if got[10, y, 2] == 51] == [7, 8, 9, 10, 11, 12, 13]
    # with the reference's offset nothing of the slab is at or beyond 5 * 1.15
    assert np.array_equal(OM.modify_heart_label(vol, min_region=1), vol)
    # the z term is scaled only upward: a voxel two slices up counts 2 * 2.65 = 5.3 < 5.75 and stays, three
    # slices up 7.95 goes; three slices down counts 3 and stays
    tall = np.zeros((21, 21, 9), dtype=np.uint8)
    tall[5:16, 10, 4] = 51
    tall[10, 10, 1:8] = 51
    cz = (11 * 4 + sum(z for z in range(1, 8) if z != 4)) / 17.0
    assert cz == 4.0
    got = OM.modify_heart_label(tall, min_region=1)
    assert [z for z in range(9) if got[10, 10, z] == 51] == [1, 2, 3, 4, 5, 6]


# ---------------------------------------------------------------------------------------------
# organ mask
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case_volume():
    return cases.organ_cases(44, 41)


def test_organ_mask_equals_the_flood_fill_restatement(case_volume):
    got = OM.organ_mask(case_volume)
    assert got.dtype == np.uint8 and got.shape == case_volume.shape and set(np.unique(got)) <= {0, 1}
    for k, name in enumerate(cases.CASE_NAMES):
        assert np.array_equal(got[k], cases.organ_mask_loops(case_volume[k])), name


def test_organ_mask_case_properties(case_volume):
    got = dict(zip(cases.CASE_NAMES, OM.organ_mask(case_volume)))
    ring = got["ring"]
    assert ring[18, 20] == 1 and ring[12:24, 14:26].all()                  # the hole is filled in stage 1
    assert ring[5, 20] == 1 and ring[4, 20] == 0                           # 1 (thickness 2) + 2 (thickness 4)
    two = got["two_label_hole"]
    assert two[18, 18] == 0 and not two[13:23, 13:23].any()                # the union's hole survives ...
    assert two[11, 18] == 1 and two[12, 18] == 0                           # ... less stage 1's line inside it
    assert two[3, 18] == 1 and two[2, 18] == 0
    pocket = got["edge_pocket"]
    assert pocket[0, 17] == 0 and pocket[3, 17] == 0 and pocket[3, 13:21].sum() < 8     # open to the edge
    assert pocket[25, 0] == 0 and pocket[26, 0] == 0 and pocket[22, 0] == 1    # the lines reach 3 pixels in
    dia = got["diagonal"]
    assert dia[12, 14] == 1 and dia[7:18, 12:17].all()                     # the diamond's inside is a hole
    assert dia[30, 29] == 1                                                # beside the corner contact: brushed
    foreign = got["foreign_label"]
    assert not foreign[5:15, 5:15].any() and not foreign[24:30, 24:30].any() and not foreign[30:36, 4:10][2:, :].any()
    assert foreign[18:22, 6:10].all()
    corner = got["far_corner"]
    assert corner[-1, -1] == 1 and corner[-6, -7] == 1 and corner[22, 0] == 1
    # a label argument: only the listed labels count
    only = OM.organ_mask(case_volume, target_labels=(10,))
    assert only[4, 5:15, 5:15].all() and not only[0].any()


def test_apply_organ_mask():
    rng = np.random.default_rng(0)
    s = rng.integers(-32768, 32767, (3, 5, 7)).astype(np.int16)
    s[0, 0, :3] = [9999, -1, 0]
    m = (rng.random(s.shape) < 0.4).astype(np.uint8)
    m[0, 0, :3] = [1, 0, 1]
    got = OM.apply_organ_mask(s, m)
    assert got.dtype == np.int16 and got is not s
    assert (got[m != 0] == 9999).all() and np.array_equal(got[m == 0], s[m == 0])
    assert (OM.apply_organ_mask(s, m, fill=-7)[m != 0] == -7).all()
    with pytest.raises(ValueError):
        OM.apply_organ_mask(s.astype(np.int32), m)
    with pytest.raises(ValueError):
        OM.apply_organ_mask(s, m[:2])


# ---------------------------------------------------------------------------------------------
# entry points
# ---------------------------------------------------------------------------------------------
def _argv(root, *extra):
    return ["--input_dir_root", str(root / "in"), "--output_dir_root", str(root / "out"), "--dataset_names", "DS",
            *extra]


def test_masking_end_to_end_then_calculate_mask(tmp_path, capsys, monkeypatch):
    import calculate
    import masking
    monkeypatch.chdir(tmp_path)                                          # the common arguments create ./data
    series, lab, order = cases.build_masking_tree(tmp_path, dicom, nifti)
    masking.main(_argv(tmp_path))
    mask = OM.organ_mask(lab)
    assert mask.any() and not mask.all()
    masked = tmp_path / "out" / "masked" / "DS" / "P1"
    assert sorted(p.name for p in masked.iterdir()) == ["POST STD", "POST VUE", "generated"]
    for sub, vol in series.items():
        assert sorted(p.name for p in (masked / sub).iterdir()) == [f"{i:03d}.dcm" for i in range(6)]
        for fi, zi in enumerate(order):                                   # file fi holds instance zi + 1
            ds = dicom.dcmread(str(masked / sub / f"{fi:03d}.dcm"))
            assert ds.file_meta.TransferSyntaxUID == dicom.EXPLICIT_VR_LE and int(ds.InstanceNumber) == zi + 1
            px = ds.pixel_array
            assert px.dtype == np.int16
            assert (px[mask[zi] != 0] == 9999).all() and np.array_equal(px[mask[zi] == 0], vol[zi][mask[zi] == 0])
    capsys.readouterr()
    # the masked evaluation now has its input
    calculate.main(_argv(tmp_path, "--mask"))
    calc = tmp_path / "out" / "calculated_mask"
    got = np.load(calc / "data" / "DS_P1_std.npy")
    want = np.where(mask != 0, 9999, series["POST STD"]).astype(np.float32) - 1024
    assert np.array_equal(got, want)
    stats = list(csv.DictReader(open(calc / "summary_statistics_masked.csv")))
    assert stats and {"Metric", "Mean"} <= set(stats[0])


def test_masking_skip_reasons(tmp_path, capsys, monkeypatch):
    import masking
    monkeypatch.chdir(tmp_path)
    pats = ("P1", "P2", "P3", "P4", "P5", "P6")
    cases.build_masking_tree(tmp_path, dicom, nifti, patients=pats)
    for f in (tmp_path / "in" / "DS" / "P2" / "POST VUE").iterdir():
        f.unlink()
    for f in (tmp_path / "in" / "DS" / "P3" / "POST STD").iterdir():
        f.unlink()
    for f in (tmp_path / "out" / "DS" / "P4").iterdir():
        f.unlink()
    (tmp_path / "out" / "modified_mask" / "DS" / "P5.nii").unlink()
    nifti.write_volume(str(tmp_path / "out" / "modified_mask" / "DS" / "P6.nii"),
                       np.ascontiguousarray(cases.masking_labels()[:5].T))
    # a dataset whose patient lists differ in length, and one whose names do not match
    (tmp_path / "in" / "DS2" / "Q1" / "POST VUE").mkdir(parents=True)
    (tmp_path / "out" / "DS2").mkdir(parents=True)
    (tmp_path / "in" / "DS3" / "A1" / "POST VUE").mkdir(parents=True)
    (tmp_path / "out" / "DS3" / "B1").mkdir(parents=True)
    argv = _argv(tmp_path)
    masking.main(argv[:-1] + ["DS", "DS2", "DS3"])
    out = capsys.readouterr().out
    assert "No NCCT DICOM files found for patient P2, skipping." in out
    assert "No CECT DICOM files found for patient P3, skipping." in out
    assert "No SCECT DICOM files found for patient P4, skipping." in out
    assert "Mask file not found for patient P5, skipping masking." in out
    assert "Slice count mismatch for patient P6, skipping." in out
    assert "Mismatch in number of patient directories among NCCT, CECT, and SCECT for dataset DS2. Skipping." in out
    assert "Patient ID mismatch between CECT and SCECT directories" in out and "B1" in out
    masked = tmp_path / "out" / "masked" / "DS"
    assert len(list((masked / "P1" / "generated").iterdir())) == 6
    for p in pats[1:]:
        assert not any((masked / p).rglob("*.dcm")), p


def test_generate_names_the_file_it_expects(tmp_path, monkeypatch):
    import masking
    monkeypatch.chdir(tmp_path)
    args = masking.get_args(_argv(tmp_path))
    assert args.device == "cpu"
    with pytest.raises(RuntimeError, match="TotalSegmentator") as e:
        masking.generate(args)
    assert "{patient}.nii" in str(e.value) and "mask" in str(e.value)
    with pytest.raises(SystemExit):
        masking.get_args(_argv(tmp_path, "--device", "tpu"))


def test_modify_heart_mask_script_on_the_host(tmp_path, monkeypatch):
    import modify_heart_mask
    monkeypatch.chdir(tmp_path)
    vol = cases.heart_tie()
    src = tmp_path / "out" / "mask" / "DS"
    src.mkdir(parents=True)
    nifti.write_volume(str(src / "P1.nii"), vol, pixdim=(0.7, 0.7, 2.5))
    modify_heart_mask.main(_argv(tmp_path))
    raw_in, raw_out = (src / "P1.nii").read_bytes(), (tmp_path / "out" / "modified_mask" / "DS" / "P1.nii").read_bytes()
    for a, b in nifti.GEOMETRY_SPANS:
        assert raw_in[a:b] == raw_out[a:b]
    got = nifti.read(str(tmp_path / "out" / "modified_mask" / "DS" / "P1.nii")).get_fdata()
    # the script runs the reference's constants (min_region 1024 drops both small blobs)
    assert np.array_equal(got, OM.modify_heart_label(vol)) and not (got == 51).any() and (got == 7).sum() == 27
