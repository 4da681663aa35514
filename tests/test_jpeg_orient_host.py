"""Files with an EXIF orientation through the host half of the split JPEG decoder (rn_jpeg_probe_oriented,
rn_jpeg_scan_probe_oriented, rn_jpeg_oriented_size, the oriented walk inside rn_jpeg_entropy_decode / rn_jpeg_huffman_model, and
jpegdec.turn): no GPU, needs the built library.  The reference is Pillow's decode AND turn of the same bytes through
imageio.imread: byte for byte."""
import ctypes as C
import struct

import numpy as np
import pytest

pytest.importorskip("PIL")

from jpeg_cases import ADOBE_APP14, SAMPLINGS, SIZES, content, encode, exif_app1, splice_after_soi  # noqa: E402
from roomnet_amd import _capi, jpegdec  # noqa: E402
from roomnet_amd.imageio import imread  # noqa: E402

RN_OK, RN_E_INVALID = 0, -1
ORIENTATIONS = range(1, 9)


def _write(path, data):
    with open(str(path), "wb") as f:
        f.write(data)
    return str(path)


def _oriented_size(info):
    h, w = C.c_int32(-1), C.c_int32(-1)
    rc = _capi.load_library().rn_jpeg_oriented_size(C.byref(info), C.byref(h), C.byref(w))
    return rc, (h.value, w.value)


def exif_app1_entry(tag_type, count, value_field, little_endian=True):
    """An APP1 Exif segment whose IFD0 holds one orientation entry of the given type, count and raw 4-byte value field."""
    e = "<" if little_endian else ">"
    tiff = (b"II" if little_endian else b"MM") + struct.pack(e + "HI", 42, 8)
    tiff += struct.pack(e + "H", 1) + struct.pack(e + "HHI", 0x0112, tag_type, count) + value_field + struct.pack(e + "I", 0)
    body = b"Exif\x00\x00" + tiff
    return b"\xff\xe1" + struct.pack(">H", len(body) + 2) + body


def xmp_app1(orientation):
    body = (b"http://ns.adobe.com/xap/1.0/\x00<x:xmpmeta xmlns:x='adobe:ns:meta/'><rdf:RDF><rdf:Description "
            b"tiff:Orientation='%d'/></rdf:RDF></x:xmpmeta>" % orientation)
    return b"\xff\xe1" + struct.pack(">H", len(body) + 2) + body


@pytest.mark.parametrize("sampling", SAMPLINGS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_oriented_probe_and_decode_equal_imread(size, sampling, tmp_path):
    """All sizes x samplings x 8 orientations x both byte orders: the probe reads the orientation and leaves the stored size,
    rn_jpeg_oriented_size is imread's shape, rn_jpeg_probe is what it was, the coefficients are the un-spliced file's, and the
    stored image (decoded ONCE) turned 8 ways is imread's image."""
    h, w = size
    p = str(tmp_path / "case.jpg")
    base = encode(p, content(h, w, "noise"), sampling, quality=90)
    base_info, base_coeffs = jpegdec.entropy_decode(base)
    stored = jpegdec.pixels_from_coeffs(base_info, base_coeffs)
    np.testing.assert_array_equal(stored, imread(p))
    for k in ORIENTATIONS:
        for le in (True, False):
            what = "orientation %d, %s" % (k, "II" if le else "MM")
            data = splice_after_soi(base, exif_app1(k, little_endian=le))
            want = imread(_write(p, data))
            rc, info = jpegdec.probe_oriented_rc(data)
            assert rc == RN_OK and info.supported == k, what
            assert (info.height, info.width) == (h, w), what
            assert list(info.blocks_w) == list(base_info.blocks_w) and list(info.blocks_h) == list(base_info.blocks_h), what
            assert bytes(info.qt) == bytes(base_info.qt), what
            assert _oriented_size(info) == (RN_OK, want.shape[:2]), what
            assert jpegdec.oriented_shape(info) == want.shape[:2], what
            assert want.shape[:2] == ((w, h) if k >= 5 else (h, w)), what
            old_rc, old = jpegdec.probe_rc(data)
            assert old_rc == RN_OK and old.supported == (1 if k == 1 else 0), what
            if k != 1:
                assert old.reason == b"EXIF orientation is not 1", what
            _info, coeffs = jpegdec.entropy_decode(data, info)
            np.testing.assert_array_equal(coeffs, base_coeffs, err_msg=what)
            np.testing.assert_array_equal(jpegdec.turn(stored, k), want, err_msg=what)
    # the composed call, once per case (it decodes again)
    k = 1 + (h + w + SAMPLINGS.index(sampling)) % 8
    data = splice_after_soi(base, exif_app1(k))
    np.testing.assert_array_equal(jpegdec.decode_bgr(data, orient=True), imread(_write(p, data)))


def test_turn_is_the_table_of_the_contract():
    im = np.arange(3 * 5 * 3, dtype=np.uint8).reshape(3, 5, 3)
    H, W = 3, 5
    table = {1: lambda y, x: (y, x), 2: lambda y, x: (y, W - 1 - x), 3: lambda y, x: (H - 1 - y, W - 1 - x),
             4: lambda y, x: (H - 1 - y, x), 5: lambda y, x: (x, y), 6: lambda y, x: (H - 1 - x, y),
             7: lambda y, x: (H - 1 - x, W - 1 - y), 8: lambda y, x: (x, W - 1 - y)}
    for k, src in table.items():
        out = jpegdec.turn(im, k)
        assert out.shape == ((W, H, 3) if k >= 5 else (H, W, 3)) and out.flags["C_CONTIGUOUS"]
        for y in range(out.shape[0]):
            for x in range(out.shape[1]):
                assert (out[y, x] == im[src(y, x)]).all(), (k, y, x)
    with pytest.raises(ValueError):
        jpegdec.turn(im, 9)


def test_entropy_decode_and_the_huffman_model_compare_the_orientation(tmp_path):
    base = encode(str(tmp_path / "b.jpg"), content(37, 53, "noise"), 2, quality=90, restart_marker_blocks=3)
    base_info, base_coeffs = jpegdec.entropy_decode(base)
    data6 = splice_after_soi(base, exif_app1(6))
    info6 = jpegdec.probe_oriented(data6)
    assert info6.supported == 6
    out = np.empty(jpegdec.coeff_count(info6), np.int16)

    def both(data, info):
        rc_e = jpegdec.entropy_decode_rc(data, info, out)
        coeffs_e = out.copy()
        rc_m, status = jpegdec.huffman_model_rc(data, info, out)
        return rc_e, coeffs_e, rc_m, status, out.copy()

    rc_e, ce, rc_m, status, cm = both(data6, info6)
    assert (rc_e, rc_m, status) == (RN_OK, RN_OK, 0)
    np.testing.assert_array_equal(ce, base_coeffs)
    np.testing.assert_array_equal(cm, base_coeffs)
    # an info whose `supported` is not what these bytes say
    wrong = jpegdec.probe_oriented(data6)
    for k, data in ((8, data6), (3, data6), (6, base), (6, splice_after_soi(base, exif_app1(8))), (1, data6)):
        wrong.supported = k
        rc_e, _ce, rc_m, status, _cm = both(data, wrong)
        assert (rc_e, rc_m, status) == (RN_E_INVALID, RN_E_INVALID, -1), (k, len(data))
    # an upright info on upright bytes with an Exif segment that says 1: as before
    data1 = splice_after_soi(base, exif_app1(1))
    rc_e, ce, rc_m, status, cm = both(data1, base_info)
    assert (rc_e, rc_m, status) == (RN_OK, RN_OK, 0)
    np.testing.assert_array_equal(ce, base_coeffs)


def test_scan_probe_oriented_is_the_scan_probe_of_the_unspliced_file(tmp_path):
    base = encode(str(tmp_path / "b.jpg"), content(37, 53, "smooth"), 1, quality=90)
    app1 = exif_app1(7, little_endian=False)
    data = splice_after_soi(base, app1)
    rc0, scan0 = jpegdec.scan_probe_rc(base)
    rc, scan = jpegdec.scan_probe_oriented_rc(data)
    assert (rc0, rc) == (RN_OK, RN_OK)
    assert scan.scan_begin == scan0.scan_begin + len(app1) and scan.scan_len == scan0.scan_len and scan.scan_len > 0
    assert bytes(scan)[16:] == bytes(scan0)[16:]
    # the old scan probe leaves the turned file alone; the new one leaves an unsupported file alone
    rc_old, old = jpegdec.scan_probe_rc(data)
    assert rc_old == RN_OK and bytes(old) == bytes(C.sizeof(old))
    rc_x, x = jpegdec.scan_probe_oriented_rc(splice_after_soi(data, xmp_app1(6)))
    assert rc_x == RN_OK and bytes(x) == bytes(C.sizeof(x))
    assert jpegdec.scan_probe_oriented_rc(data[:60])[0] == RN_E_INVALID


def test_what_the_oriented_probe_refuses(tmp_path):
    rgb = content(24, 40, "smooth")
    base = encode(str(tmp_path / "base.jpg"), rgb, 2, quality=90)
    long_le = exif_app1_entry(4, 1, struct.pack("<I", 6))
    long_be = exif_app1_entry(4, 1, struct.pack(">I", 6), little_endian=False)
    two_shorts = exif_app1_entry(3, 2, struct.pack("<HH", 6, 6))
    cases = {
        "conflicting Exif segments": (splice_after_soi(splice_after_soi(base, exif_app1(8)), exif_app1(6)), b"conflicting EXIF segments"),
        "conflict with a later upright one": (splice_after_soi(splice_after_soi(base, exif_app1(1)), exif_app1(6)), b"conflicting EXIF segments"),
        "conflict with an earlier upright one": (splice_after_soi(splice_after_soi(base, exif_app1(3)), exif_app1(1)), b"conflicting EXIF segments"),
        "XMP orientation": (splice_after_soi(base, xmp_app1(6)), b"XMP orientation"),
        "XMP orientation behind an Exif one": (splice_after_soi(splice_after_soi(base, xmp_app1(6)), exif_app1(6)), b"XMP orientation"),
        "LONG entry": (splice_after_soi(base, long_le), None),
        "LONG entry, big-endian": (splice_after_soi(base, long_be), None),
        "two SHORTs": (splice_after_soi(base, two_shorts), None),
        "adobe": (splice_after_soi(splice_after_soi(base, ADOBE_APP14), exif_app1(6)), b"Adobe APP14 segment"),
        "progressive": (splice_after_soi(encode(str(tmp_path / "p.jpg"), rgb, 2, quality=90, progressive=True), exif_app1(6)), b"progressive"),
    }
    for name, (data, reason) in cases.items():
        rc, info = jpegdec.probe_oriented_rc(data)
        assert rc == RN_OK, name
        assert info.supported == 0 and info.reason, name
        if reason is not None:
            assert info.reason == reason, name
        assert _oriented_size(info)[0] == RN_E_INVALID, name
        with pytest.raises(jpegdec.JpegUnsupported):
            jpegdec.decode_bgr(data, orient=True)
    assert jpegdec.probe_oriented_rc(b"\xff\xd8" + exif_app1(6))[0] == RN_E_INVALID          # no frame at all
    with pytest.raises(ValueError):
        jpegdec.probe_oriented(b"")


def test_tag_values_outside_2_to_8_read_as_upright_and_agreeing_segments_are_supported(tmp_path):
    base = encode(str(tmp_path / "base.jpg"), content(24, 40, "noise"), 2, quality=90)
    p = tmp_path / "t.jpg"
    for value in (0, 9, 255):
        for le in (True, False):
            data = splice_after_soi(base, exif_app1(value, little_endian=le))
            info = jpegdec.probe_oriented(data)
            assert info.supported == 1, value
            assert _oriented_size(info) == (RN_OK, (24, 40))
            np.testing.assert_array_equal(jpegdec.decode_bgr(data, orient=True), imread(_write(p, data)))
    for k in (1, 6, 7):
        twice = splice_after_soi(splice_after_soi(base, exif_app1(k, little_endian=False)), exif_app1(k))
        assert jpegdec.probe_oriented(twice).supported == k
        np.testing.assert_array_equal(jpegdec.decode_bgr(twice, orient=True), imread(_write(p, twice)))
    # the first segment decides: an out-of-range value in it reads as 1 and a later 1 agrees with it
    first_junk = splice_after_soi(splice_after_soi(base, exif_app1(1)), exif_app1(9))
    assert jpegdec.probe_oriented(first_junk).supported == 1
    np.testing.assert_array_equal(jpegdec.decode_bgr(first_junk, orient=True), imread(_write(p, first_junk)))
    # without any APP1 the two probes agree on every byte
    assert bytes(jpegdec.probe_oriented(base)) == bytes(jpegdec.probe(base))


def test_oriented_size_refuses_what_is_no_supported_info(tmp_path):
    info = jpegdec.probe_oriented(splice_after_soi(encode(str(tmp_path / "a.jpg"), content(9, 4, "noise"), 0, quality=90), exif_app1(5)))
    assert _oriented_size(info) == (RN_OK, (4, 9))
    for bad in (0, 9, -1):
        info.supported = bad
        assert _oriented_size(info)[0] == RN_E_INVALID
    info.supported = 5
    info.blocks_w[0] += 1
    assert _oriented_size(info)[0] == RN_E_INVALID
    lib = _capi.load_library()
    assert lib.rn_jpeg_oriented_size(None, None, None) == RN_E_INVALID


def test_loaders_take_turned_files_only_when_asked(tmp_path):
    base = encode(str(tmp_path / "base.jpg"), content(37, 53, "noise"), 2, quality=90)
    p = _write(tmp_path / "o6.jpg", splice_after_soi(base, exif_app1(6)))
    want = imread(p)

    class Ring:                       # (the loaders only ask a ring for a buffer)
        def buffer(self, slot, count):
            return np.empty(count + 64, np.int16 if self.words else np.uint8)

    ring = Ring()
    ring.words = True
    off = jpegdec.load_file(p, ring, 0)
    assert off[0] == "image"
    np.testing.assert_array_equal(off[1], want)
    on = jpegdec.load_file(p, ring, 0, orient=True)
    assert on[0] == "jpeg" and on[1].supported == 6
    np.testing.assert_array_equal(jpegdec.turn(jpegdec.pixels_from_coeffs(on[1], on[2][:jpegdec.coeff_count(on[1])]), 6), want)
    ring.words = False
    assert jpegdec.load_file_bytes(p, ring, 0)[0] == "image"
    kind, info, scan, data = jpegdec.load_file_bytes(p, ring, 0, orient=True)
    assert kind == "file" and info.supported == 6 and len(data) == scan.scan_len > 0


@pytest.mark.parametrize("fn", ["groundtruth_validation", "classify_im_dir", "recalibrate_from_dir", "fine_tune_from_list"])
def test_drivers_refuse_gpu_orient_without_gpu_decode(fn, tmp_path):
    from roomnet_amd import infer
    args = {"groundtruth_validation": (None, str(tmp_path / "l.txt")), "classify_im_dir": (None, str(tmp_path)),
            "recalibrate_from_dir": (None, str(tmp_path)), "fine_tune_from_list": (None, str(tmp_path / "l.txt"), 1)}[fn]
    with pytest.raises(ValueError, match="gpu_orient=True needs gpu_decode=True"):
        getattr(infer, fn)(*args, gpu_orient=True)
