"""Host half of the split JPEG encoder (roomnet_amd/jpegenc.py, csrc/rn_jpeg_host.h: rn_jpeg_encode_info,
rn_jpeg_entropy_encode) and the overlay's coverage / blend split (roomnet_amd/hershey.py).  No GPU: the library's host functions
touch no device.  The reference is Pillow's encoder (libjpeg): its files byte for byte, and their quantised coefficients read
back through this project's own entropy decoder."""
import ctypes as C
import io

import numpy as np
import pytest

pytest.importorskip("PIL")

from jpeg_cases import SIZES, content  # noqa: E402
from roomnet_amd import _capi, hershey, jpegdec, jpegenc  # noqa: E402
from roomnet_amd.imageio import imwrite  # noqa: E402

ENC_SIZES = SIZES + [(120, 200)]
RN_E_INVALID, RN_E_RANGE = -1, -5


def pillow_bytes(rgb, quality):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(rgb).save(b, "JPEG", quality=quality, subsampling=2)
    return b.getvalue()


def random_coeffs(info, seed):
    """In-range coefficients: DC values whose differences stay within category 11, AC values within category 10, most of them 0
    (long zero runs: ZRL and EOB), a few blocks dense."""
    rng = np.random.default_rng(seed)
    n = jpegdec.coeff_count(info)
    c = rng.integers(-1023, 1024, n).astype(np.int16)
    c[rng.random(n) < 0.8] = 0
    blocks = c.reshape(-1, 64)
    blocks[:, 0] = rng.integers(-1023, 1024, len(blocks))          # |difference| <= 2046 < 2^11
    blocks[::7, 1:] = rng.integers(-1023, 1024, (len(blocks[::7]), 63))
    blocks[1::5, 1:] = 0
    blocks[2::9, 63] = 5                                            # 62 zeros in front: three ZRL
    return c


@pytest.mark.parametrize("quality", [30, 95, 100])
def test_coefficients_equal_those_of_pillows_file(quality):
    for h, w in ENC_SIZES:
        for kind in ("noise", "smooth"):
            rgb = content(h, w, kind, seed=3)
            info, ref = jpegdec.entropy_decode(pillow_bytes(rgb, quality))
            mine = jpegenc.encode_info(h, w, quality)
            for f in ("width", "height", "ncomp", "hsamp", "vsamp", "restart_interval", "supported"):
                assert getattr(mine, f) == getattr(info, f), (f, h, w)
            assert bytes(mine.qt) == bytes(info.qt) and list(mine.blocks_w) == list(info.blocks_w) and list(mine.blocks_h) == list(info.blocks_h)
            got = jpegenc.coeffs_from_pixels(mine, np.ascontiguousarray(rgb[:, :, ::-1]))
            np.testing.assert_array_equal(got, ref, err_msg="%dx%d %s q%d" % (h, w, kind, quality))
            np.testing.assert_array_equal(jpegenc.coeffs_from_pixels(mine, np.ascontiguousarray(rgb[:, :, ::-1]), mulhi=False), ref)


def test_encode_bgr_is_the_file_imwrite_writes(tmp_path):
    for k, (h, w) in enumerate(ENC_SIZES):
        for kind in ("noise", "smooth"):
            bgr = np.ascontiguousarray(content(h, w, kind, seed=k)[:, :, ::-1])
            p = str(tmp_path / "w.jpg")
            assert imwrite(p, bgr)
            with open(p, "rb") as f:
                want = f.read()
            got = jpegenc.encode_bgr(bgr)
            assert got == want, "%dx%d %s: %d bytes against %d" % (h, w, kind, len(got), len(want))


# zigzag position -> natural (row-major) position
NATURAL = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49,
           56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]


def dqt_of(data):
    """{table id: natural-order list} read from the file's DQT segments themselves."""
    out, p = {}, 2
    while data[p + 1] != 0xDA:
        assert data[p] == 0xFF
        n = (data[p + 2] << 8) | data[p + 3]
        if data[p + 1] == 0xDB:
            assert n == 67 and data[p + 4] < 4, "one 8-bit table per segment"
            t = [0] * 64
            for k in range(64):
                t[NATURAL[k]] = data[p + 5 + k]
            out[data[p + 4]] = t
        p += 2 + n
    return out


@pytest.mark.parametrize("quality", [1, 30, 50, 75, 95, 100])
def test_quality_tables_equal_pillows_dqt(quality):
    want = dqt_of(pillow_bytes(content(16, 16, "smooth"), quality))
    got = jpegenc.quality_tables(quality)
    info = jpegenc.encode_info(16, 16, quality)
    assert sorted(want) == [0, 1]
    for t in (0, 1):
        assert got[t].tolist() == want[t], (quality, t)
        np.testing.assert_array_equal(np.ctypeslib.as_array(info.qt[t]), got[t])
    np.testing.assert_array_equal(np.ctypeslib.as_array(info.qt[2]), got[1])


@pytest.mark.parametrize("size", [(1, 1), (17, 33), (72, 96)])
def test_round_trip_of_random_coefficients(size):
    info = jpegenc.encode_info(size[0], size[1], 100)      # (q = 1: the decoder's |coef * q| <= RN_JPEG_COEF_LIMIT holds)
    c = random_coeffs(info, seed=size[0])
    data = jpegenc.entropy_encode(info, c)
    assert len(data) <= jpegenc.encoded_bound(info)
    info2, back = jpegdec.entropy_decode(data)
    assert bytes(info2.qt) == bytes(info.qt) and (info2.width, info2.height) == (size[1], size[0])
    np.testing.assert_array_equal(back, c)


def test_a_cap_one_byte_short_is_a_range_error_and_nothing_is_written_past_it():
    info = jpegenc.encode_info(37, 53, 95)
    c = random_coeffs(info, seed=1)
    n = len(jpegenc.entropy_encode(info, c))
    buf = np.full(n + 64, 0xA5, np.uint8)
    assert jpegenc.entropy_encode_rc(info, c, buf, cap=n - 1) == (RN_E_RANGE, n)
    assert (buf[n - 1:] == 0xA5).all()
    assert jpegenc.entropy_encode_rc(info, c, buf, cap=0) == (RN_E_RANGE, n)
    assert (buf[n - 1:] == 0xA5).all()
    assert jpegenc.entropy_encode_rc(info, c, buf, cap=n) == (0, n)
    assert (buf[n:] == 0xA5).all() and buf[:n].tobytes() == jpegenc.entropy_encode(info, c)


def test_values_beyond_the_huffman_categories_are_invalid():
    info = jpegenc.encode_info(16, 16, 95)
    buf = np.empty(jpegenc.encoded_bound(info), np.uint8)
    c = np.zeros(jpegdec.coeff_count(info), np.int16)
    c[5] = 1023
    assert jpegenc.entropy_encode_rc(info, c, buf)[0] == 0
    c[5] = 1024                                       # AC category 11
    assert jpegenc.entropy_encode_rc(info, c, buf)[0] == RN_E_INVALID
    c[5] = -1024
    assert jpegenc.entropy_encode_rc(info, c, buf)[0] == RN_E_INVALID
    c[5] = 0
    c[0], c[64] = 1024, -1023                         # a DC difference of 2047: category 11, the last one
    assert jpegenc.entropy_encode_rc(info, c, buf)[0] == 0
    c[64] = -1024                                     # 2048: category 12
    assert jpegenc.entropy_encode_rc(info, c, buf)[0] == RN_E_INVALID
    assert b"category" in _capi.load_library().rn_last_error()


def test_an_info_the_encoder_does_not_write_is_invalid():
    good = jpegenc.encode_info(16, 24, 95)
    c = np.zeros(jpegdec.coeff_count(good) * 2, np.int16)
    buf = np.empty(1 << 16, np.uint8)

    def rc(change):
        info = jpegenc.encode_info(16, 24, 95)
        change(info)
        return jpegenc.entropy_encode_rc(info, c.ctypes.data, buf)[0], jpegenc.encoded_bound(info)

    def grey(i):
        i.ncomp = 1
        i.hsamp = i.vsamp = 1

    def s422(i):
        i.vsamp = 1
        i.blocks_h[0] = i.blocks_h[1]

    def grid(i):
        i.blocks_w[0] += 1

    def unsupported(i):
        i.supported = 0

    def zero_q(i):
        i.qt[1][3] = 0

    for change in (grey, s422, grid, unsupported, zero_q):
        assert rc(change) == (RN_E_INVALID, 0), change.__name__
    assert rc(lambda i: None)[0] == 0
    lib = _capi.load_library()
    info = _capi.rn_jpeg_info()
    for w, h, q in ((0, 8, 95), (8, 0, 95), (65536, 8, 95), (8, 65536, 95), (8, 8, 0), (8, 8, 101)):
        assert lib.rn_jpeg_encode_info(w, h, q, C.byref(info)) == RN_E_INVALID
    assert lib.rn_jpeg_encode_info(65535, 1, 1, C.byref(info)) == 0 and info.blocks_w[0] == 8192


def test_the_multiply_high_quantiser_equals_the_division():
    """rn_jpeg_enc.hip quantises with (|c| + 4 q) * ceil(2^32 / 8 q) >> 32: every table entry against every magnitude."""
    c = np.arange(0, 65536, dtype=np.int64)
    for q0 in range(1, 256, 51):
        q = np.arange(q0, min(q0 + 51, 256), dtype=np.int64)[:, None]
        np.testing.assert_array_equal(jpegenc.quantise_mulhi(c[None, :], q), jpegenc.quantise(c[None, :], q))
        np.testing.assert_array_equal(jpegenc.quantise_mulhi(-c[None, :], q), jpegenc.quantise(-c[None, :], q))
    # the reciprocal fits the kernel's 32-bit register
    assert int(((1 << 32) + 7) // 8) < 1 << 32


def driver_lines(h, w, label="LivingRoom", conf=np.float32(0.98765)):
    """The two lines infer._overlay_and_write draws."""
    return [("Predicted Class: " + label, (int(.5 * w), int(.90 * h)), (h / 720.) * .85, (0, 255, 0)),
            ("Confidence: " + str(round(conf * 100, 2)) + " %", (int(.5 * w), int(.95 * h)), (h / 720.) * .85, (255, 0, 0))]


@pytest.mark.parametrize("size", [(120, 200), (240, 320), (37, 53)])
def test_coverage_and_blend_equal_put_text(size):
    """The driver's two lines -- at 120 rows their boxes overlap -- and a third line whose box the right and bottom borders clip."""
    h, w = size
    im = np.ascontiguousarray(content(h, w, "noise", seed=5)[:, :, ::-1])
    want, got = im.copy(), im.copy()
    boxes = []
    for text, org, scale, color in driver_lines(h, w) + [("Clipped gy", (w - 30, h - 3), 0.7, (10, 20, 250))]:
        hershey.put_text(want, text, org, scale, color, 1)
        box = hershey.coverage(text, org, scale, (h, w), 1)
        assert box is not None
        x, y, cov = box
        assert cov.dtype == np.float32 and 0 <= cov.min() and cov.max() <= 1
        boxes.append((x, y, x + cov.shape[1], y + cov.shape[0]))
        hershey.blend(got, x, y, cov, color)
    np.testing.assert_array_equal(got, want)
    assert (want != im).any()
    assert boxes[2][2] == w and boxes[2][3] == h, "clipped by the right and the bottom border"
    if size == (120, 200):
        assert boxes[1][1] < boxes[0][3], "the two lines' boxes overlap"
    assert hershey.coverage("x", (w + 10, h // 2), 1.0, (h, w)) is None
