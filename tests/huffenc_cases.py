"""Coefficient sets for the Huffman-encode tests (test_jpeg_huffenc_host.py on the host model, test_hip_jpeg_huffenc.py on the
kernels): hand-built blocks on a 16x16 info (one MCU: blocks 0..3 luma, 4 Cb, 5 Cr, each 64 values in natural order), the
stuffing and padding cases, the flat grey image.  Every case is ``(name, info, coeffs)``; nothing here needs a GPU."""
import numpy as np

from roomnet_amd import jpegdec, jpegenc

# zigzag position -> natural (row-major) position
NATURAL = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49,
           56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]
QUALITY = 95


def info16():
    return jpegenc.encode_info(16, 16, QUALITY)


def blocks16():
    """(flat coefficients of a 16x16 image, all zero; the same memory as [6, 64] blocks)"""
    c = np.zeros(6 * 64, np.int16)
    return c, c.reshape(6, 64)


def scan_of(data):
    """The entropy-coded bytes of a file this encoder writes: behind the fixed-length headers, in front of EOI."""
    n = len(jpegenc.encode_headers(info16()))
    assert data[n - 14:n - 12] == b"\xff\xda" and data[-2:] == b"\xff\xd9"
    return data[n:-2]


def code_sizes(headers):
    """{(class, table id): {symbol: code length}} read from the DHT segments of a file's headers."""
    out, p = {}, 2
    while headers[p + 1] != 0xDA:
        n = (headers[p + 2] << 8) | headers[p + 3]
        if headers[p + 1] == 0xC4:
            bits, vals = headers[p + 5:p + 21], headers[p + 21:p + 2 + n]
            sizes, k = {}, 0
            for l in range(16):
                for _ in range(bits[l]):
                    sizes[vals[k]] = l + 1
                    k += 1
            out[(headers[p + 4] >> 4, headers[p + 4] & 15)] = sizes
        p += 2 + n
    return out


def scan_bits(info, coeffs):
    """The bit count of the scan before padding and stuffing: encode_one_block's symbols, counted in Python from the code
    lengths in the file's own DHT segments (independent of the encoders under test)."""
    sizes = code_sizes(jpegenc.encode_headers(info))
    mx, my = int(info.blocks_w[1]), int(info.blocks_h[1])
    comps, off = [], 0
    for c in range(3):
        n = int(info.blocks_w[c]) * int(info.blocks_h[c])
        comps.append(np.asarray(coeffs[off:off + n * 64], np.int64).reshape(int(info.blocks_h[c]), int(info.blocks_w[c]), 64))
        off += n * 64
    total, pred = 0, [0, 0, 0]
    for y in range(my):
        for x in range(mx):
            for c in range(3):
                s = 2 if c == 0 else 1
                for v in range(s):
                    for h in range(s):
                        blk = comps[c][y * s + v, x * s + h]
                        t = 1 if c else 0
                        nb = int(abs(int(blk[0]) - pred[c])).bit_length()
                        pred[c] = int(blk[0])
                        total += sizes[(0, t)][nb] + nb
                        run = 0
                        for k in range(1, 64):
                            a = abs(int(blk[NATURAL[k]]))
                            if a == 0:
                                run += 1
                                continue
                            total += (run // 16) * sizes[(1, t)][0xF0]
                            total += sizes[(1, t)][((run % 16) << 4) | a.bit_length()] + a.bit_length()
                            run = 0
                        if run:
                            total += sizes[(1, t)][0x00]
    return total


def hand_built():
    """The accepted hand-built cases."""
    out = []
    for name, zz in (("lone_zz63_three_zrl_no_eob", 63), ("lone_zz17_one_zrl", 17), ("lone_zz16_run15_no_zrl", 16)):
        c, b = blocks16()
        b[0, NATURAL[zz]] = 5
        b[4, NATURAL[zz]] = -3
        out.append((name, info16(), c))
    c, b = blocks16()
    rng = np.random.default_rng(5)
    v = rng.integers(1, 1024, (6, 63)) * rng.choice([-1, 1], (6, 63))
    b[:, 1:] = v                                            # all 63 AC values non-zero
    b[:, 0] = [7, -3, 100, 0, 5, -5]
    out.append(("all_63_ac_nonzero", info16(), c))
    c, b = blocks16()
    b[0, 0], b[1, 0], b[2, 0], b[3, 0] = 1023, -1024, 1023, -1024      # DC differences +1023, -2047, +2047, -2047
    b[4, 0], b[5, 0] = 1024, -1023
    b[0, 1], b[1, 2], b[4, 63], b[5, 8] = 1023, -1023, 1023, -1023
    out.append(("top_categories", info16(), c))
    return out


def refused():
    """Cases rn_jpeg_entropy_encode refuses: AC 1024 / -1024, a DC difference of 2048 inside an MCU and of -2048."""
    out = []
    for name, (blk, pos, val) in (("ac_1024", (0, 5, 1024)), ("ac_minus_1024_chroma", (5, 63, -1024)), ("ac_min_int16", (2, 1, -32768))):
        c, b = blocks16()
        b[blk, pos] = val
        out.append((name, info16(), c))
    c, b = blocks16()
    b[0, 0], b[1, 0] = 1024, -1024
    out.append(("dc_difference_2048", info16(), c))
    c, b = blocks16()
    b[4, 0] = -2048
    out.append(("dc_difference_minus_2048_first_chroma", info16(), c))
    return out


def stuffing():
    """Repeated AC 1023 in luma: the 16-bit code of (run 0, category 10) begins with nine 1-bits and ten 1-bits of magnitude
    follow it, so FF bytes come in pairs."""
    c, b = blocks16()
    b[:4, 1:] = 1023
    return ("stuffing_ac_1023", info16(), c)


def flat_grey():
    info = jpegenc.encode_info(72, 96, QUALITY)
    im = np.full((72, 96, 3), 128, np.uint8)
    return ("flat_grey_72x96", info, jpegenc.coeffs_from_pixels(info, im))


def padding_both_ends():
    """Two 16x16 inputs found by varying one coefficient: one whose scan needs NO padding bits, one whose padded last byte is FF
    (the last block ends in ten 1-bits of magnitude, so whatever the padding adds to gives FF).  Asserts that it found both."""
    found = {}
    for val in range(1, 1024):
        c, b = blocks16()
        b[0, 1] = val
        b[5, 63] = 1023                                     # Cr ends at zigzag 63: no EOB, the magnitude bits are 1111111111
        bits = scan_bits(info16(), c)
        if bits % 8 == 0 and "no_padding" not in found:
            found["no_padding"] = ("padding_none", info16(), c)
        if bits % 8 != 0 and "ff" not in found:
            found["ff"] = ("padding_makes_ff", info16(), c)
        if len(found) == 2:
            break
    assert len(found) == 2, "the search found %s" % sorted(found)
    return found["no_padding"], found["ff"]


def random_coeffs(info, seed):
    """In-range coefficients as tests/test_jpegenc_host.py's round-trip test draws them."""
    rng = np.random.default_rng(seed)
    n = jpegdec.coeff_count(info)
    c = rng.integers(-1023, 1024, n).astype(np.int16)
    c[rng.random(n) < 0.8] = 0
    blocks = c.reshape(-1, 64)
    blocks[:, 0] = rng.integers(-1023, 1024, len(blocks))
    blocks[::7, 1:] = rng.integers(-1023, 1024, (len(blocks[::7]), 63))
    blocks[1::5, 1:] = 0
    blocks[2::9, 63] = 5
    return c
