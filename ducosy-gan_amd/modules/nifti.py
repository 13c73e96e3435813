"""Minimal NIfTI-1 reader/writer for the label volumes the masking stage consumes.

The reference reads TotalSegmentator's multi-label output through nibabel
(modify_heart_mask.py:90-91, masking.py:449), which is not installed in this image.  This module
covers what those call sites use:

  * read(path) -> NiftiVolume for a single-file ``.nii`` (``.nii.gz`` through gzip): the 348-byte
    header in either byte order, ``vox_offset``, datatypes uint8 / int16 / int32 / float32 /
    float64 / uint16, ``scl_slope`` / ``scl_inter`` applied the way nibabel's ``get_fdata()``
    applies them (float64; a slope of 0 or a non-finite slope means "no scaling");
  * NiftiVolume.get_fdata() -> float64 array indexed [x, y, z] like nibabel's.  A NIfTI file stores
    x fastest, which is exactly a C array [z, y, x]; ``get_fdata_zyx()`` / ``raw_zyx`` expose that
    view (the one the device kernels take) and ``get_fdata()`` is its transpose, no copy;
  * write_labels(path, labels_xyz, like) writes a uint8 volume that keeps the source header's
    geometry fields (pixdim, qform, sform and their codes) byte for byte.

Anything else raises ValueError naming the header field: NIfTI-2, header/image pairs, more than
three non-unit dimensions, other datatypes.  It is host-side file I/O, outside the compute path;
parity with nibabel is unpinned (nibabel cannot be installed here).
"""
from __future__ import annotations

import gzip
import struct

import numpy as np

HEADER_SIZE = 348
# field -> (offset, struct format without the byte-order mark)
FIELDS = {
    "sizeof_hdr": (0, "i"), "dim": (40, "8h"), "datatype": (70, "h"), "bitpix": (72, "h"),
    "pixdim": (76, "8f"), "vox_offset": (108, "f"), "scl_slope": (112, "f"), "scl_inter": (116, "f"),
    "qform_code": (252, "h"), "sform_code": (254, "h"), "quatern": (256, "6f"), "srow": (280, "12f"),
    "magic": (344, "4s"),
}
# the bytes write_labels never touches: pixdim, qform/sform codes, quaternion + offsets, srow_x/y/z
GEOMETRY_SPANS = ((76, 108), (252, 328))
DATATYPES = {2: np.uint8, 4: np.int16, 8: np.int32, 16: np.float32, 64: np.float64, 512: np.uint16}


def _field(header: bytes, order: str, name: str):
    off, fmt = FIELDS[name]
    v = struct.unpack_from(order + fmt, header, off)
    return v[0] if len(v) == 1 else v


class NiftiVolume:
    """A loaded volume: ``header`` (the 348 bytes), ``order`` ('<' or '>'), ``shape`` (x, y, z),
    ``raw_zyx`` (stored values, native byte order, C array [z, y, x]), ``slope`` / ``inter``
    (None when the file asks for no scaling)."""

    def __init__(self, header: bytes, order: str, raw_zyx: np.ndarray, slope, inter):
        self.header, self.order, self.raw_zyx, self.slope, self.inter = header, order, raw_zyx, slope, inter

    @property
    def shape(self):
        return self.raw_zyx.shape[::-1]

    def get_fdata_zyx(self) -> np.ndarray:
        data = self.raw_zyx.astype(np.float64)
        if self.slope is not None:
            data = data * self.slope + self.inter
        return data

    def get_fdata(self) -> np.ndarray:
        return self.get_fdata_zyx().T

    def labels_zyx(self) -> np.ndarray:
        """``get_fdata().astype(np.uint8)`` of the reference, in the [z, y, x] view."""
        return np.ascontiguousarray(self.get_fdata_zyx().astype(np.uint8))


def _open(path: str, mode: str):
    return gzip.open(path, mode) if str(path).endswith(".gz") else open(path, mode)


def read(path: str) -> NiftiVolume:
    with _open(path, "rb") as f:
        buf = f.read()
    if len(buf) < 4:
        raise ValueError(f"{path}: sizeof_hdr: file too short for a NIfTI header")
    order = None
    for o in "<>":
        size = struct.unpack_from(o + "i", buf, 0)[0]
        if size == 540:
            raise ValueError(f"{path}: sizeof_hdr = 540: NIfTI-2 is not supported")
        if size == HEADER_SIZE:
            order = o
    if order is None:
        raise ValueError(f"{path}: sizeof_hdr = {struct.unpack_from('<i', buf, 0)[0]}: not a NIfTI-1 header")
    if len(buf) < HEADER_SIZE:
        raise ValueError(f"{path}: sizeof_hdr: file shorter than the 348-byte header")
    header = bytes(buf[:HEADER_SIZE])
    magic = _field(header, order, "magic")
    if magic[:3] == b"ni1":
        raise ValueError(f"{path}: magic = 'ni1': header/image pairs (.hdr/.img) are not supported")
    if magic != b"n+1\x00":
        raise ValueError(f"{path}: magic = {magic!r}: not a single-file NIfTI-1")
    dim = _field(header, order, "dim")
    if not 1 <= dim[0] <= 7:
        raise ValueError(f"{path}: dim[0] = {dim[0]}: out of range")
    sizes = [int(d) for d in dim[1:1 + dim[0]]]
    if any(d < 1 for d in sizes):
        raise ValueError(f"{path}: dim = {list(dim)}: non-positive extent")
    if any(d != 1 for d in sizes[3:]):
        raise ValueError(f"{path}: dim = {list(dim)}: more than three non-unit dimensions")
    nx, ny, nz = (sizes[:3] + [1, 1, 1])[:3]
    code = _field(header, order, "datatype")
    if code not in DATATYPES:
        raise ValueError(f"{path}: datatype = {code}: unsupported (uint8, int16, int32, float32, float64, uint16)")
    dt = np.dtype(DATATYPES[code])
    if _field(header, order, "bitpix") != dt.itemsize * 8:
        raise ValueError(f"{path}: bitpix = {_field(header, order, 'bitpix')}: does not match datatype {code}")
    vox = _field(header, order, "vox_offset")
    if not np.isfinite(vox) or vox != int(vox) or (vox != 0 and vox < HEADER_SIZE + 4):
        raise ValueError(f"{path}: vox_offset = {vox}: invalid")
    off = max(int(vox), HEADER_SIZE + 4)
    n = nx * ny * nz
    if len(buf) < off + n * dt.itemsize:
        raise ValueError(f"{path}: dim = {list(dim)}: the file holds fewer than {n} voxels after vox_offset {off}")
    raw = np.frombuffer(buf, dtype=dt.newbyteorder(order), count=n, offset=off).astype(dt).reshape(nz, ny, nx)
    slope, inter = float(_field(header, order, "scl_slope")), float(_field(header, order, "scl_inter"))
    if slope == 0.0 or not np.isfinite(slope):
        slope = inter = None
    elif not np.isfinite(inter):
        raise ValueError(f"{path}: scl_inter = {inter}: not finite")
    return NiftiVolume(header, order, raw, slope, inter)


def write_volume(path: str, data_xyz: np.ndarray, *, order: str = "<", slope: float = 1.0, inter: float = 0.0,
                 pixdim=(1.0, 1.0, 1.0)) -> None:
    """Write a three-dimensional array indexed [x, y, z] of a supported datatype with a fresh header
    (sform along the axes with ``pixdim`` spacings): phantoms, tests and the benchmark."""
    data_xyz = np.asarray(data_xyz)
    codes = {np.dtype(v): k for k, v in DATATYPES.items()}
    if data_xyz.dtype not in codes:
        raise ValueError(f"write_volume: datatype: unsupported dtype {data_xyz.dtype}")
    if data_xyz.ndim != 3:
        raise ValueError(f"write_volume: dim: a three-dimensional array is required, got {data_xyz.ndim}")
    h = bytearray(HEADER_SIZE)
    struct.pack_into(order + "i", h, 0, HEADER_SIZE)
    struct.pack_into(order + "8h", h, 40, 3, *data_xyz.shape, 1, 1, 1, 1)
    struct.pack_into(order + "hh", h, 70, codes[data_xyz.dtype], data_xyz.dtype.itemsize * 8)
    struct.pack_into(order + "8f", h, 76, 1.0, *[float(p) for p in pixdim], 0.0, 0.0, 0.0, 0.0)
    struct.pack_into(order + "fff", h, 108, float(HEADER_SIZE + 4), float(slope), float(inter))
    struct.pack_into(order + "hh", h, 252, 0, 1)
    struct.pack_into(order + "12f", h, 280, float(pixdim[0]), 0, 0, 0, 0, float(pixdim[1]), 0, 0, 0, 0,
                     float(pixdim[2]), 0)
    h[344:348] = b"n+1\x00"
    body = np.ascontiguousarray(data_xyz.T).astype(data_xyz.dtype.newbyteorder(order)).tobytes()
    with _open(path, "wb") as f:
        f.write(bytes(h) + b"\x00\x00\x00\x00" + body)


def write_labels(path: str, labels_xyz: np.ndarray, like: NiftiVolume) -> None:
    """Write a uint8 label volume indexed [x, y, z] with ``like``'s header: every byte of it is
    kept (the geometry fields in particular) except datatype, bitpix, vox_offset, the scaling
    (set to the identity) and the magic."""
    labels_xyz = np.asarray(labels_xyz)
    if labels_xyz.dtype != np.uint8:
        raise ValueError("write_labels: datatype: a uint8 volume is required")
    if tuple(labels_xyz.shape) != tuple(like.shape):
        raise ValueError(f"write_labels: dim: volume {labels_xyz.shape} differs from the source header's {like.shape}")
    h, o = bytearray(like.header), like.order
    struct.pack_into(o + "h", h, 70, 2)
    struct.pack_into(o + "h", h, 72, 8)
    struct.pack_into(o + "f", h, 108, float(HEADER_SIZE + 4))
    struct.pack_into(o + "f", h, 112, 1.0)
    struct.pack_into(o + "f", h, 116, 0.0)
    h[344:348] = b"n+1\x00"
    with _open(path, "wb") as f:
        f.write(bytes(h) + b"\x00\x00\x00\x00" + np.ascontiguousarray(labels_xyz.T).tobytes())
