"""Files with an EXIF orientation through the GPU pixel stage (csrc/rn_jpeg.hip: the turned store of
jpeg_color_kernel for orientations 2-4, jpeg_color_turn_kernel for 5-8) and the drivers' gpu_orient= option.  JPEG bytes are made
with Pillow's encoder and an orientation is spliced in; the reference is Pillow's decode AND turn of the same bytes through
imageio.imread, byte for byte, and jpegdec.turn of jpegdec.pixels_from_coeffs, the host restatement."""
import ctypes as C
import os

import numpy as np
import pytest

pytest.importorskip("PIL")

from conftest import MODEL_PREFIX  # noqa: E402
from jpeg_cases import SIZES, content, encode, exif_app1, splice_after_soi  # noqa: E402
from roomnet_amd import _capi, jpegdec  # noqa: E402
from roomnet_amd.graph import build_graph  # noqa: E402
from roomnet_amd.imageio import imread  # noqa: E402

pytestmark = pytest.mark.gpu

MAX_BATCH = 16
GUARD = 64
RN_E_INVALID = -1
# 16 images: the 14 sizes of the host test's list with samplings and contents rotating as in test_hip_jpeg.py, then 67x131 and
# 131x67 at 4:2:0, which cross a 64-pixel tile edge with a remainder in both directions.  Image i of rotation r has orientation
# 1 + (i + r) % 8: every rotation holds every orientation twice, and over the 8 rotations EVERY image meets EVERY orientation --
# so each of 5-8 meets the odd sizes, the sizes below one MCU, 31x2 / 1x40 / 31x1, 240x320 and both tile-edge sizes.
MIXED = [(size, [2, 1, 0, "grey"][k % 4] if size not in ((31, 2), (240, 320)) else 2, ["noise", "smooth"][k % 2])
         for k, size in enumerate(SIZES)] + [((67, 131), 2, "noise"), ((131, 67), 2, "smooth")]
ROTATIONS = range(8)


def orientation(i, r):
    return 1 + (i + r) % 8


@pytest.fixture(scope="module")
def engine(weights):
    e = _capi.Engine(build_graph(6, 224), weights, device=0, dtype="bf16", max_batch=MAX_BATCH)
    yield e
    e.close()


@pytest.fixture(scope="module")
def mixed(tmp_path_factory):
    """Per image ``(coeffs, {k: (oriented info, imread's image)})``; the coefficients are decoded once per image (they are the same
    for all its orientations, which the host test checks), imread runs once per image and orientation."""
    d = tmp_path_factory.mktemp("jpeg_orient")
    out = []
    for i, ((h, w), sampling, kind) in enumerate(MIXED):
        p = str(d / ("m%02d.jpg" % i))
        base = encode(p, content(h, w, kind, seed=i), sampling, quality=[90, 30, 100][i % 3],
                      **({"restart_marker_blocks": 3} if i % 5 == 1 else {}))
        base_info, coeffs = jpegdec.entropy_decode(base)
        stored = jpegdec.pixels_from_coeffs(base_info, coeffs)
        per_k = {}
        for k in range(1, 9):
            data = splice_after_soi(base, exif_app1(k, little_endian=bool((i + k) % 2)))
            with open(p, "wb") as f:
                f.write(data)
            info = jpegdec.probe_oriented(data)
            assert info.supported == k and (info.height, info.width) == (h, w)
            ref = imread(p)
            np.testing.assert_array_equal(jpegdec.turn(stored, k), ref, err_msg="host restatement, image %d, orientation %d" % (i, k))
            per_k[k] = (info, ref)
        out.append((coeffs, per_k))
    assert len(out) == 16
    return out


def batch_of(mixed, r, pick=None):
    """[(info, coeffs, ref)] of rotation r (images ``pick``, default all)."""
    return [(mixed[i][1][orientation(i, r)][0], mixed[i][0], mixed[i][1][orientation(i, r)][1])
            for i in (range(len(mixed)) if pick is None else pick)]


class Guarded:
    """Destinations with GUARD bytes of 0xA5 on both sides (and ``shift(i)`` more in front, to move the image off its alignment)."""

    def __init__(self, engine, refs, shift=lambda i: 0):
        self.engine, self.refs = engine, refs
        self.shifts = [int(shift(i)) for i in range(len(refs))]
        self.sizes = [s + GUARD + ref.nbytes + GUARD for s, ref in zip(self.shifts, refs)]
        self.bases = [engine.device_malloc(n) for n in self.sizes]
        for b, n in zip(self.bases, self.sizes):
            engine.h2d(b, np.full(n, 0xA5, np.uint8))
        self.ptrs = [b + s + GUARD for b, s in zip(self.bases, self.shifts)]

    def read(self):
        """The images; asserts that every guard byte is untouched."""
        outs = []
        for i, (b, n, s, ref) in enumerate(zip(self.bases, self.sizes, self.shifts, self.refs)):
            whole = np.empty(n, np.uint8)
            self.engine.d2h(whole, b)
            assert (whole[:s + GUARD] == 0xA5).all(), "image %d: bytes in front of the destination were written" % i
            assert (whole[s + GUARD + ref.nbytes:] == 0xA5).all(), "image %d: bytes behind the destination were written" % i
            outs.append(whole[s + GUARD:s + GUARD + ref.nbytes].reshape(ref.shape))
        return outs

    def close(self):
        for b in self.bases:
            self.engine.device_free(b)


def decode_into(engine, batch, dst):
    arr = engine._jpeg_images([(info, coeffs) for info, coeffs, _ref in batch])
    _capi._check(engine.lib, engine.lib.rn_jpeg_decode_batch_device(engine.handle, arr, len(batch), (C.c_void_p * len(batch))(*dst.ptrs)),
                 "rn_jpeg_decode_batch_device")


@pytest.mark.parametrize("r", ROTATIONS)
def test_mixed_batch_is_byte_identical_to_imread_inside_its_guards(engine, mixed, r):
    batch = batch_of(mixed, r)
    assert {int(info.supported) for info, _c, _ref in batch} == set(range(1, 9))
    first = Guarded(engine, [ref for _i, _c, ref in batch])
    again = Guarded(engine, [ref for _i, _c, ref in batch], shift=lambda i: i % 4)      # the same call, rows off their alignment
    try:
        decode_into(engine, batch, first)
        decode_into(engine, batch, again)
        engine.sync()
        got, got2 = first.read(), again.read()
        for i, (info, _coeffs, ref) in enumerate(batch):
            what = "%s, orientation %d" % (MIXED[i], info.supported)
            assert got[i].shape == ref.shape == jpegdec.oriented_shape(info) + (3,), what
            np.testing.assert_array_equal(got[i], ref, err_msg=what)
            np.testing.assert_array_equal(got2[i], got[i], err_msg=what + ", second call")
        assert engine.jpeg_last_decode_ms() > 0
    finally:
        first.close()
        again.close()


def test_engine_decode_batch_returns_turned_shapes(engine, mixed):
    batch = batch_of(mixed, 2)
    got = engine.jpeg_decode_batch([(info, coeffs) for info, coeffs, _ref in batch])
    for g, (_info, _coeffs, ref) in zip(got, batch):
        assert g.shape == ref.shape
        np.testing.assert_array_equal(g, ref)


def test_upright_and_turned_images_share_a_batch(engine, mixed):
    """Upright images beside images of orientation 6 and 3 only: the upright ones as the parent's launches leave them, the turned
    ones through the third launch and the mirrored store."""
    pick = list(range(len(mixed)))
    ks = [1, 6, 1, 3] * 4
    batch = [(mixed[i][1][ks[i]][0], mixed[i][0], mixed[i][1][ks[i]][1]) for i in pick]
    dst = Guarded(engine, [ref for _i, _c, ref in batch])
    try:
        decode_into(engine, batch, dst)
        engine.sync()
        for i, (g, (_info, _coeffs, ref)) in enumerate(zip(dst.read(), batch)):
            np.testing.assert_array_equal(g, ref, err_msg="%s, orientation %d" % (MIXED[i], ks[i]))
        # all upright: two launches, and the bytes of test_hip_jpeg.py's references
        up = [(mixed[i][1][1][0], mixed[i][0], mixed[i][1][1][1]) for i in pick]
        for g, (_info, _coeffs, ref) in zip(engine.jpeg_decode_batch([(info, coeffs) for info, coeffs, _ref in up]), up):
            np.testing.assert_array_equal(g, ref)
    finally:
        dst.close()


def test_back_to_back_decodes_without_a_sync(engine, mixed):
    """Three calls whose tables differ -- the first half at rotation 0, the second half at rotation 3 (sizes and orientations
    differ), the first half reversed at rotation 5 (on the first call's table set) -- into separate destinations, no sync between
    them, one at the end.  The contract of rn_jpeg_decode_batch_device, as tests/test_hip_jpeg.py states it for upright files."""
    half = len(mixed) // 2
    calls = [batch_of(mixed, 0, range(half)), batch_of(mixed, 3, range(half, len(mixed))), batch_of(mixed, 5, range(half))[::-1]]
    dsts = [Guarded(engine, [ref for _i, _c, ref in call]) for call in calls]
    try:
        for call, dst in zip(calls, dsts):
            decode_into(engine, call, dst)
        engine.sync()
        for n, (call, dst) in enumerate(zip(calls, dsts)):
            for i, (g, (info, _coeffs, ref)) in enumerate(zip(dst.read(), call)):
                np.testing.assert_array_equal(g, ref, err_msg="call %d, image %d (%dx%d, orientation %d)"
                                              % (n + 1, i, info.width, info.height, info.supported))
        assert engine.jpeg_last_decode_ms() > 0
    finally:
        for dst in dsts:
            dst.close()


def oriented_file_item(data):
    info = jpegdec.probe_oriented(data)
    rc, scan = jpegdec.scan_probe_oriented_rc(data)
    assert rc == 0 and info.supported and scan.scan_len == len(data) - scan.scan_begin
    return info, scan, np.frombuffer(data, np.uint8)[int(scan.scan_begin):].copy()


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_the_crop_window_is_the_turned_images(weights, tmp_path, dtype):
    """Eight non-square files at orientations 1..8: a crop window taken from the stored size would be the wrong one for 5..8 and
    a window of the right size at the wrong place shows for a mirrored content."""
    eng = _capi.Engine(build_graph(6, 224), weights, device=0, dtype=dtype, max_batch=8)
    try:
        datas, refs = [], []
        for k in range(8):
            h, w = ((300, 400), (400, 300))[(k // 2) % 2]
            p = str(tmp_path / ("c%d.jpg" % k))
            base = encode(p, content(h, w, ["smooth", "noise"][k % 2], seed=k), [0, 1, 2][k % 3], quality=90)
            datas.append(splice_after_soi(base, exif_app1(k + 1, little_endian=bool(k % 2))))
            with open(p, "wb") as f:
                f.write(datas[-1])
            refs.append(imread(p))
        assert {r.shape[:2] for r in refs[4:]} == {(300, 400), (400, 300)}
        want_ids, want_probs = eng.classify_images(refs)
        ids, probs = eng.classify_jpegs([jpegdec.entropy_decode(d, jpegdec.probe_oriented(d)) for d in datas])
        np.testing.assert_array_equal(ids, want_ids)
        np.testing.assert_array_equal(probs, want_probs)
        ids, probs, status = eng.classify_jpeg_files([oriented_file_item(d) for d in datas])
        assert status.tolist() == [0] * 8
        np.testing.assert_array_equal(ids, want_ids)
        np.testing.assert_array_equal(probs, want_probs)
        # the Huffman stage alone takes the oriented infos too: the coefficients of the stored image
        status, coeffs = eng.jpeg_huffman_batch([oriented_file_item(d) for d in datas[4:]])
        assert status.tolist() == [0] * 4
        for c, d in zip(coeffs, datas[4:]):
            np.testing.assert_array_equal(c, jpegdec.entropy_decode(d, jpegdec.probe_oriented(d))[1])
    finally:
        eng.close()


def test_refusals_leave_the_handle_usable(engine, mixed):
    batch = batch_of(mixed, 1)
    items = [(info, coeffs) for info, coeffs, _ref in batch]
    lib, h = engine.lib, engine.handle
    d = engine.device_malloc(1 << 20)
    try:
        ptrs = (C.c_void_p * 2)(d, d)
        probs, ids, status = np.empty((2, 6), np.float32), np.empty(2, np.int64), np.zeros(2, np.int32)
        scan_bytes = np.zeros(16, np.uint8)
        files = engine._jpeg_files([(info, _capi.rn_jpeg_scan(), scan_bytes) for info, _c in items[:2]])
        outs = (C.c_void_p * 2)(d, d)
        for bad_value in (9, -1, 0):
            bad = engine._jpeg_images(items[:2])
            bad[1].info.supported = bad_value
            assert lib.rn_jpeg_decode_batch_device(h, bad, 2, ptrs) == RN_E_INVALID, bad_value
            assert b"not a supported JPEG" in lib.rn_last_error()
            assert lib.rn_classify_jpegs(h, bad, 2, probs.ctypes.data, ids.ctypes.data) == RN_E_INVALID, bad_value
            files[1].info.supported = bad_value
            assert lib.rn_jpeg_huffman_batch_device(h, files, 2, outs, status.ctypes.data) == RN_E_INVALID, bad_value
            assert lib.rn_jpeg_huffman_batch(h, files, 2, outs, status.ctypes.data) == RN_E_INVALID, bad_value
            assert lib.rn_classify_jpeg_files(h, files, 2, probs.ctypes.data, ids.ctypes.data, status.ctypes.data) == RN_E_INVALID, bad_value
    finally:
        engine.device_free(d)
    for g, (_info, _coeffs, ref) in zip(engine.jpeg_decode_batch(items), batch):
        np.testing.assert_array_equal(g, ref)


@pytest.fixture(scope="module")
def phone_dir(tmp_path_factory):
    """A directory as a phone leaves it: files of orientations 1..8 (300x400 / 400x300 / 224x224 stored, the driver tests' sizes),
    a progressive file, a PNG and a file that is no image.  Returns (directory, number of turned files)."""
    from PIL import Image
    d = tmp_path_factory.mktemp("phone") / "images"
    os.makedirs(str(d))
    for k in range(8):
        h, w = ((300, 400), (400, 300), (224, 224))[k % 3]
        p = str(d / ("o%d.jpg" % (k + 1)))
        base = encode(p, content(h, w, ["smooth", "noise"][k % 2], seed=k), [2, 1, 0][k % 3], quality=90)
        with open(p, "wb") as f:
            f.write(splice_after_soi(base, exif_app1(k + 1, little_endian=bool(k % 2))))
    encode(str(d / "prog.jpg"), content(300, 400, "smooth", seed=7), 2, quality=90, progressive=True)
    Image.fromarray(content(260, 300, "smooth", seed=8)).save(str(d / "p.png"))
    with open(str(d / "junk.jpg"), "wb") as f:
        f.write(b"\xff\xd8 not an image")
    return d, 7


def test_infer_files_and_prepare_files_with_gpu_orient(phone_dir):
    from roomnet_amd.infer import classify_im_dir, groundtruth_validation
    from roomnet_amd.network import RoomNet
    d, turned = phone_dir
    nn = RoomNet(num_classes=6, im_side=224, compute_bn_mean_var=False, optimized_inference=True, max_batch=4, dtype="bf16")
    nn.load(MODEL_PREFIX)
    try:
        paths = sorted(os.path.join(str(d), f) for f in os.listdir(str(d)))
        want = nn.infer_files(paths, batch_size=4)
        assert nn.last_decode_paths == {"jpeg": 1, "file": 0, "image": turned + 2, "unreadable": 1}
        host = nn.infer_images([imread(p) for p, ok in zip(paths, want[2]) if ok])
        np.testing.assert_array_equal(want[0][want[2]], host[0])
        np.testing.assert_array_equal(want[1][want[2]], host[1])
        got = nn.infer_files(paths, batch_size=4, gpu_orient=True)
        assert nn.last_decode_paths == {"jpeg": 8, "file": 0, "image": 2, "unreadable": 1}
        for a, b in zip(got, want):
            np.testing.assert_array_equal(a, b)
        got = nn.infer_files(paths, batch_size=4, gpu_orient=True, gpu_huffman=True)
        assert nn.last_decode_paths == {"jpeg": 0, "file": 8, "image": 2, "unreadable": 1} and nn.huffman_fallbacks == 0
        for a, b in zip(got, want):
            np.testing.assert_array_equal(a, b)
        nn.infer_files(paths, batch_size=4, gpu_huffman=True)
        assert nn.last_decode_paths == {"jpeg": 0, "file": 1, "image": turned + 2, "unreadable": 1}
        # the batches recalibrate_from_dir / fine_tune_from_list feed
        batches = {}
        for arm in (False, True):
            at, parts, bad = [], [], []
            for a, b, c in nn.prepare_files(paths, batch_size=4, gpu_orient=arm):
                at, parts, bad = at + a, parts + [b], bad + c
            assert [os.path.basename(paths[i]) for i in bad] == ["junk.jpg"]
            batches[arm] = (at, np.concatenate(parts, 0))
            assert nn.last_decode_paths["image"] == (2 if arm else turned + 2)
        assert batches[True][0] == batches[False][0]
        np.testing.assert_array_equal(batches[True][1], batches[False][1])
        np.testing.assert_array_equal(batches[True][1], nn._batch_from([imread(paths[i]) for i in batches[True][0]], "test"))
        with pytest.raises(ValueError, match="gpu_orient"):
            classify_im_dir(nn, str(d), overlay=False, gpu_decode=False, gpu_orient=True)
        with pytest.raises(ValueError, match="gpu_orient"):
            groundtruth_validation(nn, str(d / "none.txt"), gpu_decode=False, gpu_orient=True)
    finally:
        nn.sess.close()


def run_dir(nn, d, capsys, **kw):
    from roomnet_amd.infer import classify_im_dir
    out_dir = str(d) + "_classified"
    xl = classify_im_dir(nn, str(d), overlay=True, batch_size=4, **kw)
    printed = capsys.readouterr().out
    files = {}
    for dirpath, _dirs, names in os.walk(out_dir):
        for name in names:
            p = os.path.join(dirpath, name)
            with open(p, "rb") as f:
                files[os.path.relpath(p, out_dir)] = f.read()
            os.remove(p)
    with open(xl, "rb") as f:
        return f.read(), printed, files


def test_classify_im_dir_writes_the_host_arms_files_with_gpu_orient(phone_dir, capsys):
    from roomnet_amd.network import RoomNet
    d, turned = phone_dir
    nn = RoomNet(num_classes=6, im_side=224, compute_bn_mean_var=False, optimized_inference=True, max_batch=4, dtype="bf16")
    nn.load(MODEL_PREFIX)
    capsys.readouterr()                   # (what loading the model printed)
    try:
        for host_kw, gpu_kw in ((dict(heatmap="s6.bn"), dict(heatmap="s6.bn")), ({}, dict(gpu_huffman_encode=True))):
            base = run_dir(nn, d, capsys, **host_kw)
            mine = run_dir(nn, d, capsys, gpu_decode=True, gpu_encode=True, gpu_orient=True, **gpu_kw)
            assert nn.last_decode_paths == {"jpeg": 8, "file": 0, "image": 2, "unreadable": 1}
            assert base[1].count("unreadable image, skipped") == 1 and base[1].count("--->") == 11 and len(base[2]) == 10
            assert mine[1] == base[1] and mine[0] == base[0]
            assert sorted(mine[2]) == sorted(base[2])
            for name, data in base[2].items():
                assert mine[2][name] == data, name
        # without the option the turned files take the imread way, and the outputs are the same again
        off = run_dir(nn, d, capsys, gpu_decode=True, gpu_encode=True)
        assert nn.last_decode_paths["image"] == turned + 2
        assert off[0] == base[0] and off[2] == base[2]
    finally:
        nn.sess.close()
