"""Baseline JPEG, split where it stops being serial.

``probe`` and ``entropy_decode`` bind the host half of the library (``rn_jpeg_probe``, ``rn_jpeg_entropy_decode``: marker walk and
Huffman pass, pure C++ that needs no device; ctypes releases the GIL around both).  ``pixels_from_coeffs`` is the NumPy restatement of
the pixel stage -- dequantisation, ``jpeg_idct_islow``, "fancy" chroma upsampling, fixed-point YCbCr -> BGR, all integer -- which the
GPU kernels of ``csrc/rn_jpeg.hip`` are compared against byte for byte, and which itself equals libjpeg's default decode path
(what Pillow returns) byte for byte: the host half of the parity argument, as ``imageops.py`` is for the resize.
``decode_bgr`` composes them: the bytes of a supported file -> what ``imageio.imread`` returns for it.
``scan_probe_rc``, ``huffman_model_rc`` and ``load_file_bytes`` belong to the second opt-in, the Huffman pass on the GPU (DESIGN.md
section 18): the scan's byte range and lookup tables, the host model of the parallel decode, and the loader that leaves the pass out.
``probe_oriented``, ``oriented_shape``, ``turn`` and the ``orient=`` arguments belong to the third, files with an EXIF orientation
(DESIGN.md section 20): the probe that reads the orientation into ``info.supported`` instead of refusing the file, and the NumPy
statement of the turn the pixel stage's store applies.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Tuple

import numpy as np

from . import _capi
from ._capi import rn_jpeg_info

COEF_LIMIT = 1096          # RN_JPEG_COEF_LIMIT (include/roomnet_hip.h derives it)

# FIX(x) = round(x * 2^13) of jidctint.c
_F0298, _F0390, _F0541, _F0765, _F0899, _F1175 = 2446, 3196, 4433, 6270, 7373, 9633
_F1501, _F1847, _F1961, _F2053, _F2562, _F3072 = 12299, 15137, 16069, 16819, 20995, 25172


class JpegUnsupported(ValueError):
    """A JPEG file the split decoder leaves to the general one (``.reason`` says why)."""

    def __init__(self, reason: str):
        super().__init__("unsupported JPEG: %s" % reason)
        self.reason = reason


def _as_buffer(data) -> Tuple[object, int]:
    b = bytes(data) if not isinstance(data, bytes) else data
    return b, len(b)


def probe_rc(data, lib_path: Optional[str] = None) -> Tuple[int, rn_jpeg_info]:
    """``rn_jpeg_probe`` as it returns: ``(code, info)``; no exception (the robustness tests walk damaged files with it)."""
    lib = _capi.load_library(lib_path)
    b, n = _as_buffer(data)
    info = rn_jpeg_info()
    return int(lib.rn_jpeg_probe(b, n, C.byref(info))), info


def probe(data, lib_path: Optional[str] = None) -> rn_jpeg_info:
    """The file's ``rn_jpeg_info`` (``supported`` = 0 with a ``reason`` for a JPEG of another kind); ``ValueError`` for bytes that
    are no JPEG file or whose headers are truncated."""
    rc, info = probe_rc(data, lib_path)
    _capi._check(_capi.load_library(lib_path), rc, "rn_jpeg_probe")
    return info


def probe_oriented_rc(data, lib_path: Optional[str] = None) -> Tuple[int, rn_jpeg_info]:
    """``rn_jpeg_probe_oriented`` as it returns: ``(code, info)``; ``info.supported`` is 0, 1 or the EXIF orientation 2..8."""
    lib = _capi.load_library(lib_path)
    b, n = _as_buffer(data)
    info = rn_jpeg_info()
    return int(lib.rn_jpeg_probe_oriented(b, n, C.byref(info))), info


def probe_oriented(data, lib_path: Optional[str] = None) -> rn_jpeg_info:
    """``probe`` for files with an EXIF orientation: ``supported`` is 1 for an upright file and k in 2..8 for one whose decoded
    pixels are to be turned by orientation k; ``width`` and ``height`` stay the stored ones (``oriented_shape`` gives the turned)."""
    rc, info = probe_oriented_rc(data, lib_path)
    _capi._check(_capi.load_library(lib_path), rc, "rn_jpeg_probe_oriented")
    return info


def scan_probe_oriented_rc(data, lib_path: Optional[str] = None) -> Tuple[int, _capi.rn_jpeg_scan]:
    """``rn_jpeg_scan_probe_oriented`` as it returns: ``(code, scan)``."""
    lib = _capi.load_library(lib_path)
    b, n = _as_buffer(data)
    scan = _capi.rn_jpeg_scan()
    return int(lib.rn_jpeg_scan_probe_oriented(b, n, C.byref(scan))), scan


def oriented_shape(info: rn_jpeg_info) -> Tuple[int, int]:
    """``(height, width)`` of a supported file's image after the turn (``rn_jpeg_oriented_size``): swapped for orientations 5..8."""
    return _capi.jpeg_oriented_shape(info)


def turn(im: np.ndarray, k: int) -> np.ndarray:
    """The stored image ``im`` ``[H, W, ...]`` turned by EXIF orientation ``k`` (1..8), as ``ImageOps.exif_transpose`` turns it:
    2: ``O[y][x] = I[y][W-1-x]``, 3: ``I[H-1-y][W-1-x]``, 4: ``I[H-1-y][x]`` (``O`` is ``H x W``); 5: ``I[x][y]``, 6: ``I[H-1-x][y]``,
    7: ``I[H-1-x][W-1-y]``, 8: ``I[x][W-1-y]`` (``O`` is ``W x H``)."""
    k = int(k)
    if not 1 <= k <= 8:
        raise ValueError("turn: orientation %d (1..8)" % k)
    t = np.swapaxes(im, 0, 1)                    # t[y][x] = I[x][y]
    out = (im, im[:, ::-1], im[::-1, ::-1], im[::-1], t, t[:, ::-1], t[::-1, ::-1], t[::-1])[k - 1]
    return np.ascontiguousarray(out)


def coeff_count(info: rn_jpeg_info) -> int:
    """int16 elements of the file's coefficient buffer ``[component][block_y][block_x][64]``."""
    return sum(int(info.blocks_w[c]) * int(info.blocks_h[c]) * 64 for c in range(info.ncomp))


def entropy_decode_rc(data, info: rn_jpeg_info, out: np.ndarray, cap: Optional[int] = None, lib_path: Optional[str] = None) -> int:
    """``rn_jpeg_entropy_decode`` into the int16 array ``out`` with ``cap`` elements announced (default: all of it); the code."""
    lib = _capi.load_library(lib_path)
    b, n = _as_buffer(data)
    assert out.dtype == np.int16 and out.flags["C_CONTIGUOUS"]
    return int(lib.rn_jpeg_entropy_decode(b, n, C.byref(info), out.ctypes.data, out.size if cap is None else int(cap)))


def entropy_decode(data, info: Optional[rn_jpeg_info] = None, lib_path: Optional[str] = None) -> Tuple[rn_jpeg_info, np.ndarray]:
    """``(info, coeffs)``: the quantised coefficients of a supported file, int16, flat, ``[component][block_y][block_x][64]`` in
    natural order.  ``JpegUnsupported`` for a JPEG of another kind, ``ValueError`` for damaged bytes."""
    if info is None:
        info = probe(data, lib_path)
    if not info.supported:
        raise JpegUnsupported(info.reason.decode("ascii", "replace"))
    out = np.empty(coeff_count(info), np.int16)
    _capi._check(_capi.load_library(lib_path), entropy_decode_rc(data, info, out, lib_path=lib_path), "rn_jpeg_entropy_decode")
    return info, out


def scan_probe_rc(data, lib_path: Optional[str] = None) -> Tuple[int, _capi.rn_jpeg_scan]:
    """``rn_jpeg_scan_probe`` as it returns: ``(code, scan)`` -- the scan's byte range and the components' Huffman lookup tables."""
    lib = _capi.load_library(lib_path)
    b, n = _as_buffer(data)
    scan = _capi.rn_jpeg_scan()
    return int(lib.rn_jpeg_scan_probe(b, n, C.byref(scan))), scan


def huffman_model_rc(data, info: rn_jpeg_info, out: np.ndarray, subseq_bytes: int = _capi.RN_JPEG_SUBSEQ_BYTES,
                     cap: Optional[int] = None, lib_path: Optional[str] = None) -> Tuple[int, int]:
    """``rn_jpeg_huffman_model`` -- the GPU's parallel Huffman decode run lane by lane on the host -- into
    the int16 array ``out``: ``(code, status)``; the status is -1 when the call was refused."""
    lib = _capi.load_library(lib_path)
    b, n = _as_buffer(data)
    assert out.dtype == np.int16 and out.flags["C_CONTIGUOUS"]
    status = C.c_int32(-1)
    rc = lib.rn_jpeg_huffman_model(b, n, C.byref(info), out.ctypes.data, out.size if cap is None else int(cap), int(subseq_bytes),
                                   C.byref(status))
    return int(rc), int(status.value)


def _idct_pass(x, axis, itype):
    """One 1-D pass of ``jpeg_idct_islow`` along ``axis`` (length 8) before its descale, in integer type ``itype``."""
    x = np.moveaxis(x, axis, 0).astype(itype)
    z2, z3 = x[2], x[6]
    z1 = (z2 + z3) * itype(_F0541)
    tmp2 = z1 + z3 * itype(-_F1847)
    tmp3 = z1 + z2 * itype(_F0765)
    tmp0 = (x[0] + x[4]) * itype(8192)
    tmp1 = (x[0] - x[4]) * itype(8192)
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = x[7], x[5], x[3], x[1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * itype(_F1175)
    tmp0 = tmp0 * itype(_F0298)
    tmp1 = tmp1 * itype(_F2053)
    tmp2 = tmp2 * itype(_F3072)
    tmp3 = tmp3 * itype(_F1501)
    z1 = z1 * itype(-_F0899)
    z2 = z2 * itype(-_F2562)
    z3 = z3 * itype(-_F1961) + z5
    z4 = z4 * itype(-_F0390) + z5
    tmp0 = tmp0 + z1 + z3
    tmp1 = tmp1 + z2 + z4
    tmp2 = tmp2 + z2 + z3
    tmp3 = tmp3 + z1 + z4
    out = np.stack([tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2,
                    tmp10 - tmp3], 0)
    return np.moveaxis(out, 0, axis)


def idct_islow(dq: np.ndarray, itype=np.int64) -> np.ndarray:
    """``jpeg_idct_islow`` of dequantised blocks ``[..., 8, 8]`` (rows, columns) -> uint8 samples of the same shape.  ``itype``:
    the width of the intermediates (the C code's are 64-bit; ``np.int32`` is what the GPU kernel keeps, exact while
    ``|dq| <= COEF_LIMIT``)."""
    with np.errstate(over="ignore"):
        ws = (_idct_pass(dq, -2, itype) + itype(1 << 10)) >> itype(11)          # pass 1: columns, descale 11
        v = (_idct_pass(ws, -1, itype) + itype(1 << 17)) >> itype(18)           # pass 2: rows, descale 18
    m = (v & itype(1023)).astype(np.int64)
    return np.where(m < 128, m + 128, np.where(m < 512, 255, np.where(m < 896, 0, m - 896))).astype(np.uint8)


def _plane(info: rn_jpeg_info, coeffs: np.ndarray, c: int, off: int) -> np.ndarray:
    bh, bw = int(info.blocks_h[c]), int(info.blocks_w[c])
    blocks = coeffs[off:off + bh * bw * 64].reshape(bh, bw, 8, 8).astype(np.int64)
    q = np.ctypeslib.as_array(info.qt[c]).astype(np.int64).reshape(8, 8)
    px = idct_islow(blocks * q)
    return px.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)


def _h2v1_fancy(s: np.ndarray) -> np.ndarray:
    """Rows of downsampled samples ``[h, cw]`` (cw > 2) -> ``[h, 2 cw]``; edge columns replicated."""
    s = s.astype(np.int64)
    left = np.concatenate([s[:, :1], s[:, :-1]], 1)
    right = np.concatenate([s[:, 1:], s[:, -1:]], 1)
    out = np.empty((s.shape[0], 2 * s.shape[1]), np.int64)
    out[:, 0::2] = (3 * s + left + 1) >> 2
    out[:, 1::2] = (3 * s + right + 2) >> 2
    return out


def _h2v2_fancy(s: np.ndarray) -> np.ndarray:
    """Downsampled samples ``[ch, cw]`` (cw > 2) -> ``[2 ch, 2 cw]``; the row above the first is the first, below the last the last."""
    s = s.astype(np.int64)
    above = np.concatenate([s[:1], s[:-1]], 0)
    below = np.concatenate([s[1:], s[-1:]], 0)
    out = np.empty((2 * s.shape[0], 2 * s.shape[1]), np.int64)
    for par, other in ((0, above), (1, below)):
        t = 3 * s + other
        left = np.concatenate([t[:, :1], t[:, :-1]], 1)
        right = np.concatenate([t[:, 1:], t[:, -1:]], 1)
        out[par::2, 0::2] = (3 * t + left + 8) >> 4
        out[par::2, 1::2] = (3 * t + right + 7) >> 4
    return out


def _upsample(plane: np.ndarray, info: rn_jpeg_info) -> np.ndarray:
    """A chroma plane (padded to whole blocks) to at least ``height x width`` full-resolution samples."""
    h, w = int(info.height), int(info.width)
    if info.hsamp == 1:
        return plane.astype(np.int64)
    cw = (w + 1) // 2
    ch = (h + 1) // 2 if info.vsamp == 2 else h
    s = plane[:ch, :cw]                      # the component's downsampled extent, not the padded blocks
    if cw <= 2:                              # libjpeg picks plain replication here, vertically too
        return np.repeat(np.repeat(s, info.vsamp, 0), 2, 1).astype(np.int64)
    return _h2v2_fancy(s) if info.vsamp == 2 else _h2v1_fancy(s)


def pixels_from_coeffs(info: rn_jpeg_info, coeffs: np.ndarray) -> np.ndarray:
    """The pixel stage on the host: ``entropy_decode``'s output -> BGR uint8 ``[height, width, 3]``."""
    h, w = int(info.height), int(info.width)
    coeffs = np.asarray(coeffs, np.int16).reshape(-1)
    planes, off = [], 0
    for c in range(info.ncomp):
        planes.append(_plane(info, coeffs, c, off))
        off += int(info.blocks_h[c]) * int(info.blocks_w[c]) * 64
    y = planes[0][:h, :w].astype(np.int64)
    if info.ncomp == 1:
        return np.ascontiguousarray(np.repeat(y[:, :, None], 3, 2).astype(np.uint8))
    cb = _upsample(planes[1], info)[:h, :w] - 128
    cr = _upsample(planes[2], info)[:h, :w] - 128
    r = y + ((91881 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    return np.ascontiguousarray(np.clip(np.stack([b, g, r], 2), 0, 255).astype(np.uint8))


def decode_bgr(data, lib_path: Optional[str] = None, orient: bool = False) -> np.ndarray:
    """The bytes of a supported baseline JPEG file -> BGR uint8 HWC, byte for byte ``imageio.imread`` of that file.  ``orient``:
    files with an EXIF orientation are supported too: ``probe_oriented``, the stored image, ``turn``."""
    if not orient:
        info, coeffs = entropy_decode(data, lib_path=lib_path)
        return pixels_from_coeffs(info, coeffs)
    info, coeffs = entropy_decode(data, probe_oriented(data, lib_path), lib_path=lib_path)
    return turn(pixels_from_coeffs(info, coeffs), int(info.supported))


# ---- files -> coefficients on a thread pool (RoomNet.infer_files) ------------------------------------------------------------
MAX_COEFFS = 1 << 28       # int16 elements of one file this path takes (a 512 MB buffer); larger files go to the general decoder


class CoeffRing:
    """``slots`` page-locked int16 buffers (``rn_host_alloc``) for the coefficients of files in flight: a slot's buffer is kept
    and reused from file to file, and replaced by a larger one only when a file needs more than it holds."""

    def __init__(self, slots: int):
        self._bufs = [None] * int(slots)

    def __len__(self):
        return len(self._bufs)

    def buffer(self, slot: int, count: int) -> np.ndarray:
        b = self._bufs[slot]
        if b is None or b.array.size < count:
            if b is not None:
                b.close()
            b = self._bufs[slot] = _capi.PinnedArray((count + count // 8,), np.int16)
        return b.array

    def close(self) -> None:
        for b in self._bufs:
            if b is not None:
                b.close()
        self._bufs = [None] * len(self._bufs)


class ByteRing:
    """``slots`` page-locked byte buffers for the FILES in flight when the Huffman pass runs on the GPU (``load_file_bytes``): kept
    and reused from file to file like ``CoeffRing``'s."""

    def __init__(self, slots: int):
        self._bufs = [None] * int(slots)

    def __len__(self):
        return len(self._bufs)

    def buffer(self, slot: int, count: int) -> np.ndarray:
        b = self._bufs[slot]
        if b is None or b.array.size < count:
            if b is not None:
                b.close()
            b = self._bufs[slot] = _capi.PinnedArray((count + count // 8 + 64,), np.uint8)
        return b.array

    def close(self) -> None:
        for b in self._bufs:
            if b is not None:
                b.close()
        self._bufs = [None] * len(self._bufs)


def load_file_bytes(path: str, ring: ByteRing, slot: int, orient: bool = False):
    """One file for the classifier when the GPU runs the Huffman pass too: ``("file", info, scan, bytes)``
    -- a supported baseline JPEG, read into the ring's slot and only its markers walked (``rn_jpeg_probe``,
    ``rn_jpeg_scan_probe``); ``bytes`` is the view of the scan's bytes inside the slot; ``("image", bgr)`` -- anything else
    ``imageio.imread`` reads; ``None`` -- not a readable image.  Runs on a pool thread; the file read and both probes release the GIL.
    ``orient``: the oriented probes: a file with an EXIF orientation is a ``"file"`` as well, its
    ``info.supported`` the orientation."""
    from .imageio import imread
    lib = _capi.load_library()
    probe_fn, scan_fn = (lib.rn_jpeg_probe_oriented, lib.rn_jpeg_scan_probe_oriented) if orient else (lib.rn_jpeg_probe, lib.rn_jpeg_scan_probe)
    try:
        with open(path, "rb") as f:
            size = os.fstat(f.fileno()).st_size
            buf = ring.buffer(slot, max(size, 1))
            got = f.readinto(memoryview(buf)[:size]) if size else 0
    except OSError:
        return None
    if got == size and size:
        info = rn_jpeg_info()
        if probe_fn(C.cast(buf.ctypes.data, C.c_char_p), size, C.byref(info)) == 0 and info.supported and \
                coeff_count(info) <= MAX_COEFFS:
            scan = _capi.rn_jpeg_scan()
            if scan_fn(buf.ctypes.data, size, C.byref(scan)) == 0 and scan.scan_len:
                return ("file", info, scan, buf[int(scan.scan_begin):int(scan.scan_begin) + int(scan.scan_len)])
    im = imread(path)
    return None if im is None else ("image", im)


def load_file(path: str, ring: CoeffRing, slot: int, orient: bool = False):
    """One file for the classifier: ``("jpeg", info, coeffs)`` -- a supported baseline JPEG, Huffman-decoded into the ring's slot;
    ``("image", bgr)`` -- anything else ``imageio.imread`` reads (other JPEG kinds, damaged JPEG data, PNG, ...); ``None`` -- not
    a readable image.  Runs on a pool thread: file read, ``rn_jpeg_probe`` and ``rn_jpeg_entropy_decode`` all release the GIL.
    ``orient``: ``rn_jpeg_probe_oriented``: a file with an EXIF orientation is a ``"jpeg"`` as well, its
    coefficients those of the stored image and ``info.supported`` the orientation the GPU's store turns the pixels by."""
    from .imageio import imread
    try:
        with open(path, "rb") as f:
            data = f.read()
    except OSError:
        return None
    rc, info = probe_oriented_rc(data) if orient else probe_rc(data)
    if rc == 0 and info.supported:
        count = coeff_count(info)
        if count <= MAX_COEFFS:
            buf = ring.buffer(slot, count)
            if entropy_decode_rc(data, info, buf) == 0:
                return ("jpeg", info, buf)
    im = imread(path)
    return None if im is None else ("image", im)
