"""Baseline JPEG written where it stops being parallel: ``jpegdec`` mirrored.

``encode_info`` and ``entropy_encode`` bind the host half of the library (``rn_jpeg_encode_info``, ``rn_jpeg_entropy_encode``: the
output file's description and its Huffman pass, pure C++ that needs no device; ctypes releases the GIL around both).
``coeffs_from_pixels`` is the NumPy restatement of the pixel stage -- fixed-point BGR -> YCbCr, edge padding, h2v2 downsampling,
``jpeg_fdct_islow``, quantisation, all integer -- which the GPU kernels of ``csrc/rn_jpeg_enc.hip`` are compared against exactly, and
which itself equals libjpeg's default compress path (the coefficients in Pillow's files) exactly.  ``encode_bgr`` composes them:
a BGR image -> the bytes ``imageio.imwrite`` writes for a ``.jpg`` name.
"""
from __future__ import annotations

import ctypes as C
import threading
from typing import Optional, Tuple

import numpy as np

from . import _capi
from ._capi import rn_jpeg_info
from .jpegdec import coeff_count

QUALITY = 95               # imageio.imwrite's (OpenCV's default)
JPEG_EXTENSIONS = (".jpg", ".jpeg", ".jpe")

# JPEG Annex K.1, natural (row-major) order
_STD_LUMA = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80,
             62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98,
             112, 100, 103, 99)
_STD_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99) + (99,) * 36

# FIX(x) = round(x * 2^13) of jfdctint.c
_F0298, _F0390, _F0541, _F0765, _F0899, _F1175 = 2446, 3196, 4433, 6270, 7373, 9633
_F1501, _F1847, _F1961, _F2053, _F2562, _F3072 = 12299, 15137, 16069, 16819, 20995, 25172


def quality_tables(quality: int) -> Tuple[np.ndarray, np.ndarray]:
    """libjpeg's ``jpeg_set_quality``: the two standard tables (luma, chroma; natural order, uint16[64]) scaled by ``5000 / q``
    below 50, else ``200 - 2 q``; each entry ``(std * scale + 50) / 100`` clamped to 1..255."""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError("quality_tables: quality must be 1..100, got %r" % (quality,))
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((np.asarray(t, np.int64) * scale + 50) // 100, 1, 255).astype(np.uint16) for t in (_STD_LUMA, _STD_CHROMA))


def encode_info(h: int, w: int, quality: int = QUALITY, lib_path: Optional[str] = None) -> rn_jpeg_info:
    """The ``rn_jpeg_info`` of the ``h x w`` file the encoder writes (``rn_jpeg_encode_info``): what ``jpegdec.probe`` fills for
    that file -- 3 components, luma 2x2, whole-MCU block grids, ``quality_tables`` in ``qt``, ``supported`` = 1."""
    lib = _capi.load_library(lib_path)
    info = rn_jpeg_info()
    _capi._check(lib, lib.rn_jpeg_encode_info(int(w), int(h), int(quality), C.byref(info)), "rn_jpeg_encode_info")
    return info


def _fdct_pass(d):
    """One 1-D pass of ``jpeg_fdct_islow`` along the last axis (length 8) before its descales: outputs 0 and 4 are plain sums,
    the others carry 13 more fraction bits."""
    t0, t7, t1, t6 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7], d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5, t3, t4 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5], d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    z1 = (t12 + t13) * _F0541
    o2, o6 = z1 + t13 * _F0765, z1 - t12 * _F1847
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * _F1175
    t4, t5, t6, t7 = t4 * _F0298, t5 * _F2053, t6 * _F3072, t7 * _F1501
    z1, z2, z3, z4 = -z1 * _F0899, -z2 * _F2562, z5 - z3 * _F1961, z5 - z4 * _F0390
    return [t10 + t11, t7 + z1 + z4, o2, t6 + z2 + z3, t10 - t11, t5 + z2 + z4, o6, t4 + z1 + z3]


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def fdct_islow(blocks: np.ndarray) -> np.ndarray:
    """``jpeg_fdct_islow`` of ``sample - 128`` blocks ``[..., 8, 8]`` (rows, columns) -> coefficients scaled by 8, int64, same
    shape (CONST_BITS 13, PASS1_BITS 2: rows first, then columns)."""
    o = _fdct_pass(blocks.astype(np.int64))
    rows = np.stack([o[k] << 2 if k in (0, 4) else _descale(o[k], 11) for k in range(8)], -1)
    o = _fdct_pass(np.swapaxes(rows, -1, -2))
    cols = np.stack([_descale(o[k], 2) if k in (0, 4) else _descale(o[k], 15) for k in range(8)], -1)
    return np.swapaxes(cols, -1, -2)


def quantise(coef: np.ndarray, q: np.ndarray) -> np.ndarray:
    """``sign(c) * ((|c| + 4 q) / (8 q))``, integer division (jcdctmgr.c; libjpeg-turbo's reciprocal form equals it)."""
    q8 = q.astype(np.int64) * 8
    v = (np.abs(coef) + (q8 >> 1)) // q8
    return np.where(coef < 0, -v, v)


def quantise_mulhi(coef: np.ndarray, q: np.ndarray) -> np.ndarray:
    """The form the GPU kernel evaluates: ``(|c| + 4 q) * ceil(2^32 / (8 q)) >> 32``.  Equal to ``quantise`` for ``|c| < 2^21``
    (the reciprocal's excess ``e = m * 8 q - 2^32 < 8 q`` contributes ``n e / (8 q 2^32) < 1 / (8 q)`` while ``n e < 2^32``), and
    tests/test_jpegenc_host.py checks every ``q`` in 1..255 against every ``|c|`` in 0..65535."""
    q8 = q.astype(np.uint64) * np.uint64(8)
    m = ((np.uint64(1) << np.uint64(32)) + q8 - np.uint64(1)) // q8
    v = (((np.abs(coef).astype(np.uint64) + (q8 >> np.uint64(1))) * m) >> np.uint64(32)).astype(np.int64)
    return np.where(coef < 0, -v, v)


def _ycc(im_bgr: np.ndarray):
    b, g, r = (im_bgr[..., i].astype(np.int64) for i in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def _pad(p: np.ndarray, h: int, w: int) -> np.ndarray:
    return np.pad(p, ((0, h - p.shape[0]), (0, w - p.shape[1])), mode="edge")


def _h2v2(p: np.ndarray) -> np.ndarray:
    s = p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2]
    bias = np.where(np.arange(s.shape[1]) % 2 == 0, 1, 2)[None, :]          # 1 for even output columns, 2 for odd ones
    return (s + bias) >> 2


def planes_from_pixels(info: rn_jpeg_info, im_bgr: np.ndarray):
    """Colour conversion, padding and downsampling: the Y, Cb, Cr planes on their block grids (int64).  Rows are extended to the
    luma block grid by their last column BEFORE downsampling; one row is added below only when the height is odd; each
    downsampled component is then extended to its block grid by its own last row."""
    h, w = im_bgr.shape[:2]
    y, cb, cr = _ycc(im_bgr)
    h0, w0 = int(info.blocks_h[0]) * 8, int(info.blocks_w[0]) * 8
    return [_pad(y, h0, w0)] + [_pad(_h2v2(_pad(c, h + (h & 1), w0)), h0 // 2, w0 // 2) for c in (cb, cr)]


def coeffs_from_pixels(info: rn_jpeg_info, im_bgr: np.ndarray, mulhi: bool = True) -> np.ndarray:
    """The pixel stage on the host: a BGR uint8 ``[height, width, 3]`` image -> the file's quantised coefficients, int16, flat,
    ``[component][block_y][block_x][64]`` in natural order (what ``jpegdec.entropy_decode`` reads back from the file)."""
    im_bgr = np.asarray(im_bgr)
    h, w = im_bgr.shape[:2]
    if im_bgr.ndim != 3 or im_bgr.shape[2] != 3 or im_bgr.dtype != np.uint8 or (h, w) != (int(info.height), int(info.width)):
        raise ValueError("coeffs_from_pixels: expected a uint8 [%d, %d, 3] image, got %s %s"
                         % (info.height, info.width, im_bgr.dtype, im_bgr.shape))
    out = []
    for c, p in enumerate(planes_from_pixels(info, im_bgr)):
        q = np.ctypeslib.as_array(info.qt[c]).reshape(8, 8)
        bh, bw = p.shape[0] // 8, p.shape[1] // 8
        blocks = p.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3) - 128
        cq = (quantise_mulhi if mulhi else quantise)(fdct_islow(blocks), q)
        if c == 0:
            # luma blocks beyond the image's own are not transformed: AC 0, and the DC of the block before them in MCU order
            vb_h, vb_w = -(-h // 8), -(-w // 8)
            by, bx = np.mgrid[0:bh, 0:bw]
            src_y, src_x = np.minimum(by, vb_h - 1), np.minimum(np.where(by < vb_h, bx, bx | 1), vb_w - 1)
            dummy = (by >= vb_h) | (bx >= vb_w)
            dc = cq[src_y, src_x, 0, 0]
            cq = np.where(dummy[:, :, None, None], 0, cq)
            cq[:, :, 0, 0] = dc
        out.append(cq.reshape(-1))
    return np.concatenate(out).astype(np.int16)


def encoded_bound(info: rn_jpeg_info, lib_path: Optional[str] = None) -> int:
    """Bytes that always suffice for the file of ``info`` (``rn_jpeg_encoded_bound``)."""
    return int(_capi.load_library(lib_path).rn_jpeg_encoded_bound(C.byref(info)))


def entropy_encode_rc(info: rn_jpeg_info, coeffs, out: np.ndarray, cap: Optional[int] = None, lib_path: Optional[str] = None) -> Tuple[int, int]:
    """``rn_jpeg_entropy_encode`` into the uint8 array ``out`` with ``cap`` bytes announced (default: all of it): ``(code, len)``.
    ``coeffs``: an int16 array or the address of one."""
    lib = _capi.load_library(lib_path)
    assert out.dtype == np.uint8 and out.flags["C_CONTIGUOUS"]
    if isinstance(coeffs, np.ndarray):
        assert coeffs.dtype == np.int16 and coeffs.flags["C_CONTIGUOUS"] and coeffs.size >= coeff_count(info)
        coeffs = coeffs.ctypes.data
    n = C.c_size_t(0)
    rc = lib.rn_jpeg_entropy_encode(C.byref(info), C.c_void_p(int(coeffs)), out.ctypes.data, out.size if cap is None else int(cap), C.byref(n))
    return int(rc), int(n.value)


_scratch = threading.local()


def entropy_encode(info: rn_jpeg_info, coeffs, lib_path: Optional[str] = None) -> bytes:
    """The whole file for quantised coefficients in ``jpegdec.entropy_decode``'s layout.  The Huffman pass runs into a buffer the
    calling thread keeps (``rn_jpeg_encoded_bound`` bytes: untouched pages cost nothing)."""
    need = encoded_bound(info, lib_path)
    if not need:
        raise ValueError("entropy_encode: the info is not one encode_info fills")
    buf = getattr(_scratch, "buf", None)
    if buf is None or buf.size < need:
        buf = _scratch.buf = np.empty(need, np.uint8)
    rc, n = entropy_encode_rc(info, coeffs, buf, lib_path=lib_path)
    _capi._check(_capi.load_library(lib_path), rc, "rn_jpeg_entropy_encode")
    return buf[:n].tobytes()


# the status of an image after the GPU's Huffman pass (include/roomnet_hip.h: RN_JPEG_ENC_ST_*)
ST_OK, ST_CATEGORY, ST_CAP, ST_TOO_LARGE = 0, 1, 2, 3
HUFFENC_MAX_BLOCKS = 0xFFFFFFFF // 1658


def encode_headers(info: rn_jpeg_info, lib_path: Optional[str] = None) -> bytes:
    """SOI .. SOS of the file of ``info`` (``rn_jpeg_encode_headers``): the first bytes ``entropy_encode`` writes."""
    lib = _capi.load_library(lib_path)
    buf = np.empty(1024, np.uint8)
    n = C.c_size_t(0)
    _capi._check(lib, lib.rn_jpeg_encode_headers(C.byref(info), buf.ctypes.data, buf.size, C.byref(n)), "rn_jpeg_encode_headers")
    return buf[:n.value].tobytes()


def huffenc_model_rc(info: rn_jpeg_info, coeffs, out: np.ndarray, cap: Optional[int] = None, lib_path: Optional[str] = None) -> Tuple[int, int, int]:
    """``rn_jpeg_huffenc_model`` into the uint8 array ``out`` with ``cap`` bytes announced (default: all of it):
    ``(code, len, status)``.  ``coeffs``: an int16 array or the address of one."""
    lib = _capi.load_library(lib_path)
    assert out.dtype == np.uint8 and out.flags["C_CONTIGUOUS"]
    if isinstance(coeffs, np.ndarray):
        assert coeffs.dtype == np.int16 and coeffs.flags["C_CONTIGUOUS"]
        coeffs = coeffs.ctypes.data
    n, status = C.c_size_t(0), C.c_int32(0)
    rc = lib.rn_jpeg_huffenc_model(C.byref(info), C.c_void_p(int(coeffs)), out.ctypes.data, out.size if cap is None else int(cap),
                                   C.byref(n), C.byref(status))
    return int(rc), int(n.value), int(status.value)


def huffenc_model(info: rn_jpeg_info, coeffs, lib_path: Optional[str] = None) -> Tuple[Optional[bytes], int]:
    """The host model of the GPU's Huffman encode: ``(file, status)``; ``file`` is what
    ``entropy_encode`` writes where ``status`` is ``ST_OK``, else None."""
    need = encoded_bound(info, lib_path)
    if not need:
        raise ValueError("huffenc_model: the info is not one encode_info fills")
    blocks = coeff_count(info) // 64
    buf = np.empty(need if blocks <= HUFFENC_MAX_BLOCKS else 1024, np.uint8)
    rc, n, status = huffenc_model_rc(info, coeffs, buf, lib_path=lib_path)
    _capi._check(_capi.load_library(lib_path), rc, "rn_jpeg_huffenc_model")
    return (buf[:n].tobytes() if status == ST_OK else None), status


def encode_bgr(im_bgr: np.ndarray, quality: int = QUALITY, lib_path: Optional[str] = None) -> bytes:
    """A BGR uint8 HWC image -> the bytes of the file ``imageio.imwrite`` writes for a ``.jpg`` name, byte for byte."""
    im_bgr = np.ascontiguousarray(im_bgr, dtype=np.uint8)
    info = encode_info(im_bgr.shape[0], im_bgr.shape[1], quality, lib_path)
    return entropy_encode(info, coeffs_from_pixels(info, im_bgr), lib_path)
