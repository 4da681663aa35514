"""The host model of the GPU's Huffman encode (csrc/rn_jpeg_huffenc.h: rn_jpeg_huffenc_model, rn_jpeg_encode_headers; DESIGN.md
section 19).  No GPU: the model runs the four phases of csrc/rn_jpeg_huffenc.hip on the host through the same per-position
encoder.  The reference is the sequential pass, jpegenc.entropy_encode, byte for byte; a case whose point is a property of the
STREAM asserts that property on the reference's output."""
import numpy as np
import pytest

pytest.importorskip("PIL")

import huffenc_cases as cases  # noqa: E402
from jpeg_cases import SIZES, content  # noqa: E402
from roomnet_amd import jpegdec, jpegenc  # noqa: E402

RN_E_INVALID = -1
PADDING = cases.padding_both_ends()         # (the search asserts that it found both)


def same_as_reference(info, c, name=""):
    ref = jpegenc.entropy_encode(info, c)
    got, status = jpegenc.huffenc_model(info, c)
    assert status == jpegenc.ST_OK, (name, status)
    assert got == ref, "%s: %d bytes against %d" % (name, len(got), len(ref))
    return ref


@pytest.mark.parametrize("quality", [30, 90, 100])
def test_sizes_and_qualities(quality):
    for k, (h, w) in enumerate(SIZES):
        for kind in ("noise", "smooth"):
            info = jpegenc.encode_info(h, w, quality)
            c = jpegenc.coeffs_from_pixels(info, np.ascontiguousarray(content(h, w, kind, seed=k)[:, :, ::-1]))
            same_as_reference(info, c, "%dx%d %s q%d" % (h, w, kind, quality))


def test_flat_grey_blocks_share_words():
    name, info, c = cases.flat_grey()
    ref = same_as_reference(info, c, name)
    blocks = jpegdec.coeff_count(info) // 64
    assert cases.scan_bits(info, c) == 6 * (blocks * 4 // 6) + 4 * (blocks * 2 // 6)       # 6 bits per luma block, 4 per chroma block
    assert len(cases.scan_of(ref)) < blocks                                                # less than a byte per block


@pytest.mark.parametrize("case", cases.hand_built(), ids=lambda c: c[0])
def test_hand_built_blocks(case):
    name, info, c = case
    ref = same_as_reference(info, c, name)
    assert (len(cases.scan_of(ref).replace(b"\xff\x00", b"\xff")) * 8 - cases.scan_bits(info, c)) in range(8)


def test_the_runs_of_the_hand_built_blocks_are_what_they_are_named_for():
    sizes = cases.code_sizes(jpegenc.encode_headers(cases.info16()))
    zrl, eob = sizes[(1, 0)][0xF0], sizes[(1, 0)][0x00]
    by_name = {name: (info, c) for name, info, c in cases.hand_built()}
    c, b = cases.blocks16()
    empty = cases.scan_bits(cases.info16(), c)
    for name, n_zrl, run, has_eob in (("lone_zz63_three_zrl_no_eob", 3, 14, False), ("lone_zz17_one_zrl", 1, 0, True),
                                      ("lone_zz16_run15_no_zrl", 0, 15, True)):
        info, c = by_name[name]
        luma = n_zrl * zrl + sizes[(1, 0)][(run << 4) | 3] + 3 + (eob if has_eob else 0) - eob
        chroma = n_zrl * sizes[(1, 1)][0xF0] + sizes[(1, 1)][(run << 4) | 2] + 2 + (0 if has_eob else -sizes[(1, 1)][0x00])
        assert cases.scan_bits(info, c) == empty + luma + chroma, name


@pytest.mark.parametrize("case", cases.refused(), ids=lambda c: c[0])
def test_what_the_host_pass_refuses_is_status_category(case):
    name, info, c = case
    cap = 700
    buf = np.full(cap + 64, 0xA5, np.uint8)
    assert jpegenc.entropy_encode_rc(info, c, np.empty(jpegenc.encoded_bound(info), np.uint8))[0] == RN_E_INVALID
    rc, n, status = jpegenc.huffenc_model_rc(info, c, buf, cap=cap)
    assert (rc, status) == (0, jpegenc.ST_CATEGORY), name
    assert (buf[cap:] == 0xA5).all()
    assert jpegenc.huffenc_model(info, c) == (None, jpegenc.ST_CATEGORY)


def test_the_last_accepted_categories_are_accepted():
    # (the neighbours of the refused cases: status CATEGORY exactly where the host pass returns RN_E_INVALID)
    for blk, pos, val in ((0, 5, 1023), (5, 63, -1023), (1, 0, -1023), (4, 0, -2047), (4, 0, 2047)):
        c, b = cases.blocks16()
        b[0, 0] = 1024 if (blk, pos) == (1, 0) else 0
        b[blk, pos] = val
        assert jpegenc.entropy_encode_rc(cases.info16(), c, np.empty(4096, np.uint8))[0] == 0
        same_as_reference(cases.info16(), c, str((blk, pos, val)))


def test_stuffing_of_adjacent_ff_bytes():
    name, info, c = cases.stuffing()
    ref = same_as_reference(info, c, name)
    scan = cases.scan_of(ref)
    assert b"\xff\x00\xff\x00" in scan
    assert scan.count(b"\xff\x00") >= 8


def test_padding_both_ends():
    (name0, info0, c0), (name1, info1, c1) = PADDING
    assert cases.scan_bits(info0, c0) % 8 == 0
    ref = same_as_reference(info0, c0, name0)
    assert len(cases.scan_of(ref).replace(b"\xff\x00", b"\xff")) * 8 == cases.scan_bits(info0, c0)      # no padding bits
    assert cases.scan_bits(info1, c1) % 8 != 0
    ref = same_as_reference(info1, c1, name1)
    assert ref.endswith(b"\xff\x00\xff\xd9")                 # the padded last byte became FF and is stuffed


def test_a_cap_one_byte_short_is_status_cap_and_nothing_is_written_past_it():
    info = jpegenc.encode_info(37, 53, 95)
    c = cases.random_coeffs(info, seed=1)
    ref = jpegenc.entropy_encode(info, c)
    n = len(ref)
    buf = np.full(n + 64, 0xA5, np.uint8)
    assert jpegenc.huffenc_model_rc(info, c, buf, cap=n - 1) == (0, n, jpegenc.ST_CAP)
    assert (buf[n - 1:] == 0xA5).all()
    buf[:] = 0xA5
    assert jpegenc.huffenc_model_rc(info, c, buf, cap=0) == (0, n, jpegenc.ST_CAP)
    assert (buf == 0xA5).all()
    assert jpegenc.huffenc_model_rc(info, c, buf, cap=n) == (0, n, jpegenc.ST_OK)
    assert (buf[n:] == 0xA5).all() and buf[:n].tobytes() == ref


def test_too_large_is_decided_from_the_info_alone():
    info = jpegenc.encode_info(16384, 16384, 95)
    assert jpegdec.coeff_count(info) // 64 > jpegenc.HUFFENC_MAX_BLOCKS
    c = np.zeros(64, np.int16)                               # (far too few coefficients: they are not read)
    buf = np.full(64, 0xA5, np.uint8)
    assert jpegenc.huffenc_model_rc(info, c, buf) == (0, 0, jpegenc.ST_TOO_LARGE)
    assert (buf == 0xA5).all()
    assert jpegenc.HUFFENC_MAX_BLOCKS == (2 ** 32 - 1) // 1658 and jpegenc.HUFFENC_MAX_BLOCKS * 1658 < 2 ** 32
    assert jpegdec.coeff_count(jpegenc.encode_info(1080, 1920, 95)) // 64 == 48960


def test_a_null_pointer_or_another_info_is_invalid():
    info = cases.info16()
    c, _b = cases.blocks16()
    buf = np.empty(4096, np.uint8)
    assert jpegenc.huffenc_model_rc(info, 0, buf)[0] == RN_E_INVALID
    info.ncomp = 1
    assert jpegenc.huffenc_model_rc(info, c, buf)[0] == RN_E_INVALID
    with pytest.raises(Exception):
        jpegenc.encode_headers(info)


@pytest.mark.parametrize("size,quality", [((1, 1), 30), ((37, 53), 95), ((120, 200), 100)])
def test_headers_are_the_beginning_of_the_file(size, quality):
    info = jpegenc.encode_info(size[0], size[1], quality)
    head = jpegenc.encode_headers(info)
    ref = jpegenc.entropy_encode(info, np.zeros(jpegdec.coeff_count(info), np.int16))
    assert len(head) == 623 and ref[:len(head)] == head and head[-14:-12] == b"\xff\xda"


@pytest.mark.parametrize("size", [(1, 1), (17, 33), (72, 96)])
def test_round_trip_of_random_coefficients(size):
    info = jpegenc.encode_info(size[0], size[1], 100)      # (q = 1: the decoder's |coef * q| <= RN_JPEG_COEF_LIMIT holds)
    c = cases.random_coeffs(info, seed=size[0])
    data = same_as_reference(info, c, str(size))
    info2, back = jpegdec.entropy_decode(data)
    assert (info2.width, info2.height) == (size[1], size[0])
    np.testing.assert_array_equal(back, c)
