"""The parallel Huffman decode on the host (csrc/rn_jpeg_huff.h through rn_jpeg_huffman_model, and rn_jpeg_scan_probe): no GPU, needs
the built library.  The model runs the GPU's four phases lane by lane at any subsequence length; the reference is the sequential
pass, rn_jpeg_entropy_decode, on the same bytes: equal coefficients where it accepts, a non-zero status exactly where it refuses."""
import numpy as np
import pytest

pytest.importorskip("PIL")

from jpeg_cases import SAMPLINGS, SIZES, VARIANTS, content, encode, hand_built_grey_8x8  # noqa: E402
from roomnet_amd import _capi, jpegdec  # noqa: E402

RN_OK, RN_E_INVALID, RN_E_RANGE = 0, -1, -5
GUARD = 0x5A5A


def host(data, info=None):
    info = info or jpegdec.probe(data)
    out = np.empty(jpegdec.coeff_count(info), np.int16)
    return jpegdec.entropy_decode_rc(data, info, out), out


def model(data, subseq_bytes, info=None):
    """(code, status, coefficients, the 64 guard words behind them)"""
    info = info or jpegdec.probe(data)
    cap = jpegdec.coeff_count(info)
    buf = np.full(cap + 64, GUARD, np.int16)
    rc, status = jpegdec.huffman_model_rc(data, info, buf, subseq_bytes, cap=cap)
    return rc, status, buf[:cap], buf[cap:]


def test_whole_corpus_at_five_subsequence_lengths(tmp_path):
    """Every file of the split decoder's corpus; 4096 bytes is one subsequence for all but the largest files."""
    p = str(tmp_path / "case.jpg")
    compared = 0
    for h, w in SIZES:
        for sampling in SAMPLINGS:
            for kw in VARIANTS:
                for kind in ("noise", "smooth"):
                    data = encode(p, content(h, w, kind), sampling, **kw)
                    rc, want = host(data)
                    assert rc == RN_OK
                    for sb in (4, 8, 64, 128, 4096):
                        rc, status, got, guard = model(data, sb)
                        assert (rc, status) == (RN_OK, 0), (h, w, sampling, kw, kind, sb)
                        assert np.array_equal(got, want), (h, w, sampling, kw, kind, sb)
                        assert (guard == GUARD).all()
                        compared += 1
    assert compared == 672 * 5


def symbols(data):
    """The sequential decoder's walk of a supported file, restated on the tables rn_jpeg_scan_probe returns: the scan's bytes and
    [(raw bit position of the code, of its magnitude field, behind the symbol, code length)] per symbol; a raw bit position counts
    the scan's bytes as they are in the file."""
    info = jpegdec.probe(data)
    rc, scan = jpegdec.scan_probe_rc(data)
    assert rc == RN_OK
    s = np.frombuffer(data, np.uint8)[int(scan.scan_begin):]
    vals, raw, markers, b = [], [], set(), 0
    while b < len(s):
        if s[b] != 0xFF:
            vals.append(int(s[b])), raw.append(b)
            b += 1
        elif b + 1 < len(s) and s[b + 1] == 0x00:
            vals.append(0xFF), raw.append(b)
            b += 2
        elif b + 1 < len(s) and 0xD0 <= s[b + 1] <= 0xD7:
            markers.add(len(vals))
            b += 2
        else:
            break
    raw.append(b)
    bits = "".join(format(v, "08b") for v in vals) + "0" * 64

    def rawbit(pos):
        return raw[pos // 8] * 8 + pos % 8

    def code(tab, pos):
        for length in range(1, 17):
            c = int(bits[pos:pos + length], 2)
            if c <= tab.maxcode[length]:
                return tab.vals[c + tab.valoff[length]], length
        raise AssertionError("no code")

    luma = info.hsamp * info.vsamp
    comps = [0] * luma + list(range(1, info.ncomp))
    mcus = (info.blocks_w[0] // info.hsamp) * (info.blocks_h[0] // info.vsamp)
    out, pos = [], 0
    for mcu in range(mcus):
        if info.restart_interval and mcu and mcu % info.restart_interval == 0:
            pos = -(-pos // 8) * 8
            assert pos // 8 in markers
        for c in comps:
            sym, length = code(scan.dc[c], pos)
            out.append((rawbit(pos), rawbit(pos + length), rawbit(pos + length + sym), length))
            pos += length + sym
            k = 1
            while k < 64:
                sym, length = code(scan.ac[c], pos)
                size = sym & 15
                out.append((rawbit(pos), rawbit(pos + length), rawbit(pos + length + size), length))
                pos += length + size
                if size == 0 and sym != 0xF0:
                    break
                k += 16 if size == 0 else (sym >> 4) + 1
    return s, out


def sweep_files(tmp_path):
    p = str(tmp_path / "s.jpg")
    return [encode(p, content(17, 33, "noise"), 2, quality=100),
            encode(p, content(17, 33, "noise"), 2, quality=90, restart_marker_blocks=3),
            encode(p, content(17, 33, "noise", seed=1), 2, quality=100, optimize=True)]


def test_a_seam_at_every_byte_of_small_files(tmp_path):
    """subseq_bytes 4 .. 64 on the 17 x 33 4:2:0 quality-100 file, the restart_marker_blocks=3 file and an optimize=True file; the
    four situations a seam can fall into are asserted to occur, found from the bytes and the sequential decoder's symbols."""
    seen = dict(between_ff_and_00=0, on_a_restart_marker=0, inside_a_16_bit_code=0, inside_a_magnitude_field=0)
    for data in sweep_files(tmp_path):
        rc, want = host(data)
        assert rc == RN_OK
        s, syms = symbols(data)
        seams = set()
        for sb in range(4, 65):
            rc, status, got, guard = model(data, sb)
            assert (rc, status) == (RN_OK, 0), sb
            assert np.array_equal(got, want), sb
            assert (guard == GUARD).all()
            seams.update(range(sb, len(s), sb))
        for b in sorted(seams):
            seen["between_ff_and_00"] += int(s[b - 1] == 0xFF and s[b] == 0x00)
            seen["on_a_restart_marker"] += int((s[b] == 0xFF and b + 1 < len(s) and 0xD0 <= s[b + 1] <= 0xD7) or
                                               (s[b - 1] == 0xFF and 0xD0 <= s[b] <= 0xD7))
        for at, mag, end, length in syms:
            inside_code = any(at < 8 * b < mag for b in range(at // 8 + 1, mag // 8 + 1) if b in seams)
            seen["inside_a_16_bit_code"] += int(length == 16 and inside_code)
            seen["inside_a_magnitude_field"] += int(any(mag < 8 * b < end for b in range(mag // 8 + 1, end // 8 + 1) if b in seams))
    assert all(seen.values()), seen


def damaged(tmp_path):
    """[(name, bytes)]: damaged scans of small files whose headers are intact."""
    p = str(tmp_path / "d.jpg")
    out = []
    plain = encode(p, content(17, 33, "noise"), 2, quality=90)
    rst = encode(p, content(37, 53, "noise"), 2, quality=90, restart_marker_blocks=3)
    for name, data in (("plain", plain), ("restart", rst)):
        begin = int(jpegdec.scan_probe_rc(data)[1].scan_begin)
        out += [("%s cut at %d" % (name, n), data[:n]) for n in range(begin, len(data))]
    big = encode(p, content(37, 53, "noise"), 2, quality=90)
    begin = int(jpegdec.scan_probe_rc(big)[1].scan_begin)
    rng = np.random.default_rng(20240611)
    for pos in rng.integers(begin, len(big), 200):
        b = bytearray(big)
        b[pos] = int(rng.integers(0, 256))
        out.append(("byte %d overwritten" % pos, bytes(b)))
    s = np.frombuffer(rst, np.uint8)
    marks = [i for i in range(int(jpegdec.scan_probe_rc(rst)[1].scan_begin), len(rst) - 1) if s[i] == 0xFF and 0xD0 <= s[i + 1] <= 0xD7]
    assert len(marks) >= 3
    wrong = bytearray(rst)
    wrong[marks[1] + 1] = 0xD0 + ((wrong[marks[1] + 1] + 3) & 7)
    out.append(("wrong RSTn number", bytes(wrong)))
    out.append(("missing restart marker", rst[:marks[1]] + rst[marks[1] + 2:]))
    out.append(("restart marker twice", rst[:marks[1]] + rst[marks[1]:marks[1] + 2] + rst[marks[1]:]))
    for dc, ac in ((1097, 0), (-1097, 0), (0, 1097), (0, -1097)):
        out.append(("coefficient %d / %d" % (dc, ac), hand_built_grey_8x8(1, dc, ac)))
    return out


def test_damaged_scans_get_a_status_exactly_where_the_sequential_pass_refuses(tmp_path):
    cases = damaged(tmp_path)
    refused = accepted = 0
    codes = set()
    for name, data in cases:
        info = jpegdec.probe(data)
        assert info.supported
        rc_host, _c = host(data, info)
        for sb in (8, 128):
            rc, status, _got, guard = model(data, sb, info)
            assert rc == RN_OK and status >= 0, name
            assert (status != 0) == (rc_host != RN_OK), (name, sb, status, rc_host)
            assert (guard == GUARD).all(), name
            codes.add(status)
        refused += rc_host != RN_OK
        accepted += rc_host == RN_OK
    assert refused > 400 and accepted > 20
    assert {_capi.RN_JPEG_ST_TRUNCATED, _capi.RN_JPEG_ST_RESTART, _capi.RN_JPEG_ST_COEF_LIMIT, _capi.RN_JPEG_ST_RUN_PAST_BLOCK} <= codes


@pytest.mark.parametrize("q, at_limit", [(1, 1096), (2, 548)])
def test_the_coefficient_limit_fires_one_above_it_and_not_at_it(q, at_limit):
    for sign in (1, -1):
        for which in ("dc", "ac"):
            ok = hand_built_grey_8x8(q, sign * at_limit if which == "dc" else 0, sign * at_limit if which == "ac" else 0)
            rc, status, got, _g = model(ok, 128)
            assert (rc, status) == (RN_OK, 0) and np.array_equal(got, host(ok)[1])
            over = hand_built_grey_8x8(q, sign * (at_limit + 1) if which == "dc" else 0, sign * (at_limit + 1) if which == "ac" else 0)
            for sb in (4, 128):
                assert model(over, sb)[:2] == (RN_OK, _capi.RN_JPEG_ST_COEF_LIMIT)


def test_model_refuses_what_the_sequential_pass_refuses_to_look_at(tmp_path):
    data = encode(str(tmp_path / "v.jpg"), content(37, 53, "noise"), 2, quality=90)
    info = jpegdec.probe(data)
    count = jpegdec.coeff_count(info)
    buf = np.full(count + 64, GUARD, np.int16)
    assert jpegdec.huffman_model_rc(data, info, buf, 128, cap=count - 1)[0] == RN_E_RANGE
    assert jpegdec.huffman_model_rc(data, info, buf, 3, cap=count)[0] == RN_E_RANGE
    assert jpegdec.huffman_model_rc(data, info, buf, 4097, cap=count)[0] == RN_E_RANGE
    assert jpegdec.huffman_model_rc(data[:100], info, buf, 128, cap=count)[0] == RN_E_INVALID
    other = jpegdec.probe(encode(str(tmp_path / "w.jpg"), content(37, 54, "noise"), 2, quality=90))
    assert jpegdec.huffman_model_rc(data, other, buf, 128, cap=count)[0] == RN_E_INVALID
    assert (buf == GUARD).all()


def test_scan_probe_agrees_with_probe(tmp_path):
    from PIL import Image
    rgb = content(24, 40, "smooth")
    for sampling in SAMPLINGS:
        for kw in (dict(quality=90), dict(quality=90, optimize=True)):
            data = encode(str(tmp_path / "a.jpg"), rgb, sampling, **kw)
            rc, scan = jpegdec.scan_probe_rc(data)
            info = jpegdec.probe(data)
            assert rc == RN_OK and info.supported
            assert data[int(scan.scan_begin) - 2 - 2 - 2 * info.ncomp - 4:][:2] == b"\xff\xda"           # the SOS segment ends there
            assert scan.scan_begin + scan.scan_len == len(data)
            for c in range(info.ncomp):
                assert any(scan.dc[c].look) and any(scan.ac[c].look)
            if info.ncomp == 3:                               # Cb and Cr share their tables
                assert bytes(scan.dc[1]) == bytes(scan.dc[2]) and bytes(scan.ac[1]) == bytes(scan.ac[2])
                assert bytes(scan.ac[0]) != bytes(scan.ac[1])
    prog = encode(str(tmp_path / "p.jpg"), rgb, 2, quality=90, progressive=True)
    rc, scan = jpegdec.scan_probe_rc(prog)
    assert rc == jpegdec.probe_rc(prog)[0] == RN_OK and jpegdec.probe(prog).supported == 0
    assert scan.scan_len == 0 and not any(bytes(scan))
    Image.fromarray(rgb).save(str(tmp_path / "a.png"))
    for junk in (open(str(tmp_path / "a.png"), "rb").read(), b"", data[:100]):
        assert jpegdec.scan_probe_rc(junk)[0] == jpegdec.probe_rc(junk)[0] == RN_E_INVALID
