"""Host half of the split JPEG decoder (csrc/rn_jpeg_host.h through the C ABI, roomnet_amd/jpegdec.py): no GPU, needs the built
library.  The reference is Pillow's decode of the same bytes through imageio.imread: byte for byte."""
import numpy as np
import pytest

pytest.importorskip("PIL")

from jpeg_cases import (ADOBE_APP14, SAMPLINGS, SIZES, VARIANTS, content, encode, exif_app1, hand_built_grey_8x8,  # noqa: E402
                        splice_after_soi)
from roomnet_amd import jpegdec  # noqa: E402
from roomnet_amd.imageio import imread  # noqa: E402

RN_OK, RN_E_INVALID = 0, -1
GUARD = 0x5A5A


def _write(path, data):
    with open(path, "wb") as f:
        f.write(data)
    return str(path)


@pytest.mark.parametrize("sampling", SAMPLINGS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_decode_bgr_is_byte_identical_to_imread(size, sampling, tmp_path):
    h, w = size
    p = str(tmp_path / "case.jpg")
    for kw in VARIANTS:
        for kind in ("noise", "smooth"):
            data = encode(p, content(h, w, kind), sampling, **kw)
            want = imread(p)
            got = jpegdec.decode_bgr(data)
            assert got.shape == want.shape == (h, w, 3), (kw, kind)
            np.testing.assert_array_equal(got, want, err_msg="%s %s" % (kw, kind))


@pytest.mark.parametrize("sampling, hv", [(0, (1, 1)), (1, (2, 1)), (2, (2, 2)), ("grey", (1, 1))])
def test_probe_fields(sampling, hv, tmp_path):
    h, w = 37, 53
    data = encode(str(tmp_path / "a.jpg"), content(h, w, "smooth"), sampling, quality=90, restart_marker_blocks=3)
    info = jpegdec.probe(data)
    assert (info.supported, info.width, info.height) == (1, w, h)
    assert info.ncomp == (1 if sampling == "grey" else 3)
    assert (info.hsamp, info.vsamp) == hv
    assert info.restart_interval == 3
    mx, my = -(-w // (8 * hv[0])), -(-h // (8 * hv[1]))
    assert (info.blocks_w[0], info.blocks_h[0]) == (mx * hv[0], my * hv[1])
    for c in range(1, info.ncomp):
        assert (info.blocks_w[c], info.blocks_h[c]) == (mx, my)
    # the tables against Pillow's own reading of the file (which de-zigzags them too)
    from PIL import Image
    with Image.open(str(tmp_path / "a.jpg")) as im:
        qz = im.quantization
    for c in range(info.ncomp):
        assert list(info.qt[c]) == list(qz[0 if c == 0 else 1])
    assert list(info.qt[0])[:9] == [3, 2, 2, 3, 5, 8, 10, 12, 2]            # quality 90 of Annex K's luma table, row-major
    no_rst = jpegdec.probe(encode(str(tmp_path / "b.jpg"), content(h, w, "smooth"), sampling, quality=90))
    assert no_rst.restart_interval == 0


def test_probe_leaves_other_jpeg_kinds_to_the_general_decoder(tmp_path):
    from PIL import Image
    rgb = content(24, 40, "smooth")
    base = encode(str(tmp_path / "base.jpg"), rgb, 2, quality=90)
    cases = {"progressive": encode(str(tmp_path / "p.jpg"), rgb, 2, quality=90, progressive=True)}
    Image.fromarray(rgb).convert("CMYK").save(str(tmp_path / "c.jpg"), "JPEG")
    cases["cmyk"] = open(str(tmp_path / "c.jpg"), "rb").read()
    cases["orientation 6"] = splice_after_soi(base, exif_app1(6))
    cases["orientation 6, big-endian"] = splice_after_soi(base, exif_app1(6, little_endian=False))
    cases["adobe"] = splice_after_soi(base, ADOBE_APP14)
    for name, data in cases.items():
        rc, info = jpegdec.probe_rc(data)
        assert rc == RN_OK, name
        assert info.supported == 0 and info.reason, name
        with pytest.raises(jpegdec.JpegUnsupported):
            jpegdec.decode_bgr(data)
    # Pillow reads the spliced orientation too (so the file really is one imread turns)
    assert imread(_write(tmp_path / "o6.jpg", cases["orientation 6"])).shape == (40, 24, 3)


def test_probe_png_is_invalid_and_orientation_1_is_supported(tmp_path):
    from PIL import Image
    rgb = content(24, 40, "noise")
    Image.fromarray(rgb).save(str(tmp_path / "a.png"))
    rc, _info = jpegdec.probe_rc(open(str(tmp_path / "a.png"), "rb").read())
    assert rc == RN_E_INVALID
    with pytest.raises(ValueError):
        jpegdec.probe(b"")
    base = encode(str(tmp_path / "base.jpg"), rgb, 2, quality=90)
    assert jpegdec.probe_rc(base[:100])[0] == RN_E_INVALID          # headers cut short
    for le in (True, False):
        data = splice_after_soi(base, exif_app1(1, little_endian=le))
        assert jpegdec.probe(data).supported == 1
        np.testing.assert_array_equal(jpegdec.decode_bgr(data), imread(_write(tmp_path / "o1.jpg", data)))


def _damaged_inputs(tmp_path):
    data = encode(str(tmp_path / "v.jpg"), content(37, 53, "noise"), 2, quality=90)
    cut = [data[:int(n)] for n in np.linspace(0, len(data) - 1, 40)]
    rng = np.random.default_rng(20240611)
    hit = []
    for pos in rng.integers(0, len(data), 200):
        b = bytearray(data)
        b[pos] = int(rng.integers(0, 256))
        hit.append(bytes(b))
    return data, cut + hit


def test_damaged_files_return_a_code_and_stay_inside_the_buffer(tmp_path):
    data, damaged = _damaged_inputs(tmp_path)
    good = jpegdec.probe(data)
    count = jpegdec.coeff_count(good)
    assert len(damaged) == 240
    seen = set()
    for d in damaged:
        rc, info = jpegdec.probe_rc(d)
        assert rc <= 0
        for use in ((info,) if rc == RN_OK and info.supported else ()) + (good,):
            # `cap` announces exactly what the file needs according to the info in use; 64 guard words lie behind it
            cap = jpegdec.coeff_count(use) if use is not good else count
            if cap > (1 << 24):
                continue                   # (a damaged size field can ask for more than a test should allocate)
            buf = np.full(cap + 64, GUARD, np.int16)
            rc2 = jpegdec.entropy_decode_rc(d, use, buf, cap=cap)
            assert rc2 <= 0
            seen.add(rc2)
            assert (buf[cap:] == GUARD).all()
    assert RN_OK in seen and RN_E_INVALID in seen


def test_coefficient_buffer_too_small_is_refused(tmp_path):
    data = encode(str(tmp_path / "v.jpg"), content(37, 53, "noise"), 2, quality=90)
    info = jpegdec.probe(data)
    count = jpegdec.coeff_count(info)
    buf = np.full(count + 64, GUARD, np.int16)
    assert jpegdec.entropy_decode_rc(data, info, buf, cap=count - 1) == -5          # RN_E_RANGE
    assert (buf == GUARD).all()


@pytest.mark.parametrize("q, at_limit", [(1, 1096), (2, 548)])
def test_refusal_fires_one_above_the_limit_and_not_at_it(q, at_limit):
    """RN_JPEG_COEF_LIMIT on hand-built files: |coef * q| = 1096 decodes, the next representable value is refused, for the DC
    coefficient and for an AC coefficient, either sign."""
    assert jpegdec.COEF_LIMIT == 1096 == q * at_limit
    for sign in (1, -1):
        for which in ("dc", "ac"):
            ok = hand_built_grey_8x8(q, sign * at_limit if which == "dc" else 0, sign * at_limit if which == "ac" else 0)
            info, coeffs = jpegdec.entropy_decode(ok)
            assert coeffs[0 if which == "dc" else 1] == sign * at_limit and np.count_nonzero(coeffs) == 1
            over = hand_built_grey_8x8(q, sign * (at_limit + 1) if which == "dc" else 0, sign * (at_limit + 1) if which == "ac" else 0)
            info = jpegdec.probe(over)
            assert info.supported == 1
            buf = np.zeros(64, np.int16)
            assert jpegdec.entropy_decode_rc(over, info, buf) == RN_E_INVALID


def test_32_bit_restatement_is_exact_at_the_limit():
    """What the limit promises: with |coef * q| <= 1096 the 32-bit intermediates the GPU kernel keeps give the 64-bit result.
    Worst cases by construction: for every output sample (k, c) the sign pattern that drives its two linear forms to their
    largest value, plus seeded random signs."""
    m = jpegdec._idct_pass(np.eye(8, dtype=np.int64), 0, np.int64)           # m[k, i]: weight of input i in output k of a pass
    assert int(np.abs(m).sum(1).max()) == 61214                             # the figure the limit is derived from
    sg = np.where(m >= 0, 1, -1)
    worst = np.stack([np.outer(sg[k], sg[c]) for k in range(8) for c in range(8)], 0) * jpegdec.COEF_LIMIT
    rnd = np.random.default_rng(3).choice([-1, 1], (512, 8, 8)) * jpegdec.COEF_LIMIT
    blocks = np.concatenate([worst, -worst, rnd], 0)
    np.testing.assert_array_equal(jpegdec.idct_islow(blocks, np.int32), jpegdec.idct_islow(blocks, np.int64))
    # the limit itself: the column pass's results fit the 16-bit workspace of the reference's SIMD code at 1096 and not at 1097,
    # and at 1096 no sum of either pass leaves 32 bits
    def column_pass(b):
        return (jpegdec._idct_pass(b, -2, np.int64) + 1024) >> 11
    ws = column_pass(np.concatenate([worst, -worst], 0))
    assert np.abs(ws).max() <= 32767 < np.abs(column_pass(worst // jpegdec.COEF_LIMIT * (jpegdec.COEF_LIMIT + 1))).max()
    assert np.abs(jpegdec._idct_pass(worst, -2, np.int64)).max() + 1024 < 2 ** 31
    rows = np.stack([np.outer(np.ones(8, np.int64), sg[c]) for c in range(8)], 0) * int(np.abs(ws).max())
    assert np.abs(jpegdec._idct_pass(rows, -1, np.int64)).max() + (1 << 17) < 2 ** 31
