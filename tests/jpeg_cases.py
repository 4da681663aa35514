"""JPEG files for the split-decoder tests, made at test time with Pillow's encoder; the reference for every comparison is
Pillow's decode of the same bytes through ``roomnet_amd.imageio.imread``."""
import io
import os
import struct

import numpy as np

SIZES = [(1, 1), (16, 16), (8, 24), (17, 33), (37, 53), (31, 1), (31, 2), (9, 4), (20, 5), (1, 40), (3, 17), (50, 49), (72, 96),
         (240, 320)]           # h x w
SAMPLINGS = [0, 1, 2, "grey"]    # Pillow's subsampling: 4:4:4, 4:2:2, 4:2:0
VARIANTS = [dict(quality=30), dict(quality=90), dict(quality=100), dict(quality=90, optimize=True),
            dict(quality=90, restart_marker_blocks=3), dict(quality=90, restart_marker_rows=1)]


def content(h, w, kind, seed=0):
    """RGB uint8 [h, w, 3]: seeded noise, or a smooth two-axis ramp."""
    if kind == "noise":
        return np.random.default_rng(seed * 1000003 + h * 1009 + w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack([xx * 255 // max(w - 1, 1), yy * 255 // max(h - 1, 1), (xx + yy) * 7 % 256], 2).astype(np.uint8)


def encode(path, rgb, sampling, **kw):
    """Write ``rgb`` as a JPEG file at ``path``; returns the file's bytes.  (With ``optimize`` Pillow's encoder needs the whole file
    in one buffer of ``max(ImageFile.MAXBLOCK, w * h)`` bytes, which noise at a high quality outgrows: the block size is raised
    for the call.)"""
    from PIL import Image, ImageFile
    im = Image.fromarray(rgb)
    if sampling == "grey":
        im = im.convert("L")
    else:
        kw = dict(kw, subsampling=sampling)
    keep = ImageFile.MAXBLOCK
    ImageFile.MAXBLOCK = max(keep, 4 * rgb.shape[0] * rgb.shape[1] + 4096)
    try:
        im.save(path, "JPEG", **kw)
    finally:
        ImageFile.MAXBLOCK = keep
    with open(path, "rb") as f:
        return f.read()


def splice_after_soi(data, segment):
    assert data[:2] == b"\xff\xd8"
    return data[:2] + segment + data[2:]


ADOBE_APP14 = b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x01"


def exif_app1(orientation, little_endian=True):
    """An APP1 segment whose IFD0 holds only the orientation tag."""
    e = "<" if little_endian else ">"
    tiff = (b"II" if little_endian else b"MM") + struct.pack(e + "HI", 42, 8)
    tiff += struct.pack(e + "H", 1) + struct.pack(e + "HHIHH", 0x0112, 3, 1, orientation, 0) + struct.pack(e + "I", 0)
    body = b"Exif\x00\x00" + tiff
    return b"\xff\xe1" + struct.pack(">H", len(body) + 2) + body


def hand_built_grey_8x8(q, dc, ac1):
    """A one-block grey baseline file from hand-written tables: quantisation table all ``q`` (8-bit), DC coefficient ``dc`` and
    the first AC coefficient ``ac1`` (0: none), each 512 <= |value| < 2048, coded with two three-symbol Huffman tables (2-bit
    codes): DC 00 -> category 11, 01 -> category 0, 10 -> category 10; AC 00 -> EOB, 01 -> run 0 / size 11, 10 -> run 0 / size 10."""
    def coded(v):              # the code of the value's category, then its magnitude field
        s = abs(v).bit_length()
        assert s in (10, 11)
        return ("00" if s == 11 else "10") + format(v if v > 0 else v + (1 << s) - 1, "0%db" % s)
    bits = coded(dc) if dc else "01"
    if ac1:
        code = coded(ac1)
        bits += ("01" if code[:2] == "00" else "10") + code[2:]
    bits += "00"                                           # EOB
    bits += "1" * (-len(bits) % 8)
    scan = bytes(int(bits[i:i + 8], 2) for i in range(0, len(bits), 8)).replace(b"\xff", b"\xff\x00")

    def seg(marker, body):
        return b"\xff" + bytes([marker]) + struct.pack(">H", len(body) + 2) + body
    dht_dc = bytes([0x00]) + bytes([0, 3] + [0] * 14) + bytes([11, 0, 10])
    dht_ac = bytes([0x10]) + bytes([0, 3] + [0] * 14) + bytes([0x00, 0x0B, 0x0A])
    return (b"\xff\xd8" + seg(0xDB, bytes([0]) + bytes([q] * 64)) + seg(0xC0, struct.pack(">BHHB", 8, 8, 8, 1) + bytes([1, 0x11, 0]))
            + seg(0xC4, dht_dc) + seg(0xC4, dht_ac) + seg(0xDA, bytes([1, 1, 0x00, 0, 63, 0])) + scan + b"\xff\xd9")
