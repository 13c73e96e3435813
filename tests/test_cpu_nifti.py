"""modules/nifti.py: the NIfTI-1 subset the masking stage reads and writes (no GPU)."""
import gzip
import struct

import numpy as np
import pytest

from modules import nifti

DTYPES = [np.uint8, np.int16, np.int32, np.float32, np.float64, np.uint16]


def _volume(dtype, shape=(5, 4, 3), seed=0):
    rng = np.random.default_rng(seed)
    if np.issubdtype(dtype, np.floating):
        return rng.normal(0, 100, shape).astype(dtype)
    info = np.iinfo(dtype)
    return rng.integers(info.min, info.max, shape, endpoint=True).astype(dtype)


def _hand_header(order, dims, code, bitpix, vox_offset=352.0, slope=0.0, inter=0.0, magic=b"n+1\x00", sizeof=348):
    """A header packed field by field from the NIfTI-1 offsets (independent of the module's table)."""
    h = bytearray(348)
    struct.pack_into(order + "i", h, 0, sizeof)                     # sizeof_hdr
    struct.pack_into(order + "8h", h, 40, *dims)                    # dim[8]
    struct.pack_into(order + "h", h, 70, code)                      # datatype
    struct.pack_into(order + "h", h, 72, bitpix)                    # bitpix
    struct.pack_into(order + "8f", h, 76, -1.0, 0.7, 0.8, 2.5, 0, 0, 0, 0)   # pixdim
    struct.pack_into(order + "f", h, 108, vox_offset)               # vox_offset
    struct.pack_into(order + "f", h, 112, slope)                    # scl_slope
    struct.pack_into(order + "f", h, 116, inter)                    # scl_inter
    struct.pack_into(order + "hh", h, 252, 1, 2)                    # qform_code, sform_code
    struct.pack_into(order + "6f", h, 256, 0.1, 0.2, 0.3, -10.0, -20.0, 30.0)   # quatern_b..d, qoffset_x..z
    struct.pack_into(order + "12f", h, 280, *np.arange(12, dtype=np.float32) * 1.5)   # srow_x, srow_y, srow_z
    h[344:348] = magic
    return bytes(h)


@pytest.mark.parametrize("order", ["<", ">"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_round_trip_of_every_datatype_and_byte_order(tmp_path, dtype, order):
    vol = _volume(dtype)
    path = str(tmp_path / "v.nii")
    nifti.write_volume(path, vol, order=order)
    got = nifti.read(path)
    assert got.order == order and got.shape == vol.shape and got.raw_zyx.dtype == np.dtype(dtype)
    assert got.raw_zyx.dtype.isnative and np.array_equal(got.raw_zyx, vol.T)
    fd = got.get_fdata()
    assert fd.dtype == np.float64 and fd.shape == vol.shape and np.array_equal(fd, vol.astype(np.float64))


@pytest.mark.parametrize("order", ["<", ">"])
def test_hand_built_header_and_the_two_views(tmp_path, order):
    """x is the fastest axis of the file: voxel (x, y, z) sits at offset x + nx * (y + ny * z)."""
    nx, ny, nz = 4, 3, 2
    stored = np.arange(nx * ny * nz, dtype=np.int16) * 3 - 7
    pad = b"\xab" * 12                                              # vox_offset past the extension flag
    buf = _hand_header(order, (3, nx, ny, nz, 1, 1, 1, 1), 4, 16, vox_offset=364.0) + b"\0\0\0\0" + pad + \
        stored.astype(np.dtype(np.int16).newbyteorder(order)).tobytes()
    path = tmp_path / "hand.nii"
    path.write_bytes(buf)
    vol = nifti.read(str(path))
    xyz, zyx = vol.get_fdata(), vol.get_fdata_zyx()
    assert xyz.shape == (nx, ny, nz) and zyx.shape == (nz, ny, nx) and zyx.flags.c_contiguous
    for x in range(nx):
        for y in range(ny):
            for z in range(nz):
                want = float(stored[x + nx * (y + ny * z)])
                assert xyz[x, y, z] == want and zyx[z, y, x] == want
    assert np.array_equal(vol.raw_zyx.ravel(), stored)
    # dim[0] < 3 and trailing unit dimensions are fine
    path.write_bytes(_hand_header(order, (5, 6, 1, 1, 1, 1, 0, 0), 2, 8) + b"\0\0\0\0" + bytes(range(6)))
    assert np.array_equal(nifti.read(str(path)).get_fdata()[:, 0, 0], np.arange(6.0))


def test_scaling_as_get_fdata_applies_it(tmp_path):
    vol = _volume(np.int16, seed=3)
    path = str(tmp_path / "s.nii")
    nifti.write_volume(path, vol, slope=0.5, inter=-1024.0)
    got = nifti.read(path)
    assert np.array_equal(got.get_fdata(), vol.astype(np.float64) * np.float64(np.float32(0.5)) + -1024.0)
    assert np.array_equal(got.raw_zyx, vol.T)                       # the stored values stay available
    for slope in (0.0, float("nan"), float("inf")):                 # "no scaling"
        nifti.write_volume(path, vol, slope=slope, inter=5.0)
        assert np.array_equal(nifti.read(path).get_fdata(), vol.astype(np.float64))
    labels = np.array([[[0, 51, 255]]], dtype=np.uint8)
    nifti.write_volume(path, labels)
    assert nifti.read(path).labels_zyx().tolist() == [[[0]], [[51]], [[255]]]


@pytest.mark.parametrize("order", ["<", ">"])
def test_write_labels_keeps_the_geometry_bytes(tmp_path, order):
    src = tmp_path / "src.nii"
    stored = _volume(np.float32, (4, 3, 2))
    header = _hand_header(order, (3, 4, 3, 2, 1, 1, 1, 1), 16, 32, slope=2.0, inter=1.0)
    src.write_bytes(header + b"\0\0\0\0" + stored.T.astype(np.dtype(np.float32).newbyteorder(order)).tobytes())
    vol = nifti.read(str(src))
    labels = (np.arange(24).reshape(4, 3, 2) * 9 % 256).astype(np.uint8)
    dst = tmp_path / "dst.nii"
    nifti.write_labels(str(dst), labels, vol)
    raw = dst.read_bytes()
    for a, b in nifti.GEOMETRY_SPANS:
        assert raw[a:b] == header[a:b]
    assert raw[76:108] == header[76:108] and raw[252:328] == header[252:328]    # pixdim; qform + sform
    assert raw[40:56] == header[40:56]                                          # dim
    back = nifti.read(str(dst))
    assert back.order == order and back.raw_zyx.dtype == np.uint8
    assert np.array_equal(back.get_fdata(), labels.astype(np.float64))
    with pytest.raises(ValueError, match="dim"):
        nifti.write_labels(str(dst), labels[:3], vol)
    with pytest.raises(ValueError, match="datatype"):
        nifti.write_labels(str(dst), labels.astype(np.int16), vol)


def test_gzip(tmp_path):
    vol = _volume(np.uint8, (6, 5, 4))
    path = str(tmp_path / "v.nii.gz")
    nifti.write_volume(path, vol)
    assert open(path, "rb").read(2) == b"\x1f\x8b"
    got = nifti.read(path)
    assert np.array_equal(got.raw_zyx, vol.T)
    out = str(tmp_path / "l.nii.gz")
    nifti.write_labels(out, vol, got)
    assert np.array_equal(nifti.read(out).raw_zyx, vol.T)
    plain = tmp_path / "plain.nii"
    plain.write_bytes(gzip.open(path, "rb").read())
    assert np.array_equal(nifti.read(str(plain)).raw_zyx, vol.T)


@pytest.mark.parametrize("field,kwargs,dims", [
    ("sizeof_hdr", dict(sizeof=540), (3, 2, 2, 2, 1, 1, 1, 1)),                 # NIfTI-2
    ("sizeof_hdr", dict(sizeof=100), (3, 2, 2, 2, 1, 1, 1, 1)),
    ("magic", dict(magic=b"ni1\x00"), (3, 2, 2, 2, 1, 1, 1, 1)),                # header/image pair
    ("magic", dict(magic=b"xyz\x00"), (3, 2, 2, 2, 1, 1, 1, 1)),
    ("dim", dict(), (4, 2, 2, 2, 3, 1, 1, 1)),                                  # four non-unit dimensions
    ("dim", dict(), (0, 2, 2, 2, 1, 1, 1, 1)),
    ("dim", dict(), (3, 2, 0, 2, 1, 1, 1, 1)),
    ("datatype", dict(code=128, bitpix=24), (3, 2, 2, 2, 1, 1, 1, 1)),          # RGB24
    ("bitpix", dict(code=4, bitpix=8), (3, 2, 2, 2, 1, 1, 1, 1)),
    ("vox_offset", dict(vox_offset=100.0), (3, 2, 2, 2, 1, 1, 1, 1)),
    ("dim", dict(vox_offset=4000.0), (3, 2, 2, 2, 1, 1, 1, 1)),                 # data past the end of the file
])
def test_refusals_name_the_field(tmp_path, field, kwargs, dims):
    kw = dict(code=2, bitpix=8)
    kw.update(kwargs)
    path = tmp_path / "bad.nii"
    path.write_bytes(_hand_header("<", dims, kw.pop("code"), kw.pop("bitpix"), **kw) + b"\0" * 4 + b"\0" * 64)
    with pytest.raises(ValueError, match=field):
        nifti.read(str(path))


def test_refusals_of_the_writer(tmp_path):
    with pytest.raises(ValueError, match="datatype"):
        nifti.write_volume(str(tmp_path / "x.nii"), np.zeros((2, 2, 2), dtype=np.int64))
    with pytest.raises(ValueError, match="dim"):
        nifti.write_volume(str(tmp_path / "x.nii"), np.zeros((2, 2), dtype=np.uint8))
    (tmp_path / "short.nii").write_bytes(b"\x5c\x01")
    with pytest.raises(ValueError, match="sizeof_hdr"):
        nifti.read(str(tmp_path / "short.nii"))
