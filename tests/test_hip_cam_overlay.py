"""Grad-CAM heat maps drawn on the GPU (csrc/rn_cam_overlay.hip: rn_cam_overlay_batch_device), Engine.explain_resident and
classify_im_dir's heatmap= path.  The reference is cam.overlay_image, byte for byte: no comparison here takes a tolerance."""
import ctypes as C
import os

import numpy as np
import pytest

pytest.importorskip("PIL")

from conftest import MODEL_PREFIX  # noqa: E402
import cam_cases  # noqa: E402
from cam_cases import SHAPES, WEIGHTS  # noqa: E402
from jpeg_cases import content, encode  # noqa: E402
from roomnet_amd import _capi, cam, hershey, jpegdec, jpegenc  # noqa: E402
from roomnet_amd.graph import build_graph  # noqa: E402

pytestmark = pytest.mark.gpu

MAX_BATCH = len(SHAPES)
RN_E_INVALID, RN_E_RANGE = -1, -5


@pytest.fixture(scope="module")
def engine(weights):
    e = _capi.Engine(build_graph(6, 224), weights, device=0, dtype="bf16", max_batch=MAX_BATCH)
    yield e
    e.close()


@pytest.fixture(scope="module")
def images():
    return cam_cases.images()


@pytest.fixture(scope="module")
def cases(images):
    """Per weight: its maps and what cam.overlay_image makes of every image; computed once, never modified."""
    out = []
    for turn, weight in enumerate(WEIGHTS):
        maps = cam_cases.maps(turn)
        out.append((weight, maps, [cam.overlay_image(im, m, weight) for im, m in zip(images, maps)]))
    return out


class Resident:
    """Images and maps in device memory."""

    def __init__(self, engine, ims, maps):
        self.engine, self.ims, self.maps = engine, ims, maps
        self.d_im = [engine.device_malloc(im.nbytes) for im in ims]
        self.d_map = [engine.device_malloc(m.nbytes) for m in maps]
        for d, a in zip(self.d_im + self.d_map, list(ims) + list(maps)):
            engine.h2d(d, a)

    def items(self):
        return [(d, im.shape[:2], dm, m.shape) for d, im, dm, m in zip(self.d_im, self.ims, self.d_map, self.maps)]

    def download(self):
        out = [np.empty(im.shape, np.uint8) for im in self.ims]
        for a, d in zip(out, self.d_im):
            self.engine.d2h(a, d)
        return out

    def close(self):
        for d in self.d_im + self.d_map:
            self.engine.device_free(d)


def assert_images(got, want, shapes=SHAPES):
    for k, (a, w) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(a, w, err_msg=str(shapes[k]))


@pytest.mark.parametrize("turn", range(len(WEIGHTS)))
def test_mixed_batch_equals_overlay_image(engine, images, cases, turn):
    weight, maps, want = cases[turn]
    assert {m.shape for m in maps} == {(46, 46), (21, 21)} and not maps[cam_cases.ZERO_MAP].any()
    assert np.count_nonzero(maps[cam_cases.HOT_PIXEL]) == 1
    res = Resident(engine, images, maps)
    try:
        engine.cam_overlay_batch(res.items(), weight)
        engine.sync()
        assert_images(res.download(), want)
        assert engine.cam_last_overlay_ms() > 0
        if weight > 0:
            assert all((w != im).any() for w, im in zip(want, images))
    finally:
        res.close()


def driver_lines(im, label="Kitchen", conf=np.float32(0.98765)):
    h, w = im.shape[:2]
    return [("Predicted Class: " + label, (int(.5 * w), int(.90 * h)), (h / 720.) * .85, (0, 255, 0)),
            ("Confidence: " + str(round(conf * 100, 2)) + " %", (int(.5 * w), int(.95 * h)), (h / 720.) * .85, (255, 0, 0))]


def test_the_heat_is_under_the_text_and_in_the_encoded_file(engine, images, cases):
    weight, maps, want = cases[1]
    res = Resident(engine, images, maps)
    infos = [jpegenc.encode_info(im.shape[0], im.shape[1]) for im in images]
    coeffs = [_capi.PinnedArray((jpegdec.coeff_count(i),), np.int16) for i in infos]
    try:
        overlays, drawn = [], []
        for im, heat in zip(images, want):
            boxes = [(hershey.coverage(text, org, scale, im.shape[:2], 1), color) for text, org, scale, color in driver_lines(im)]
            overlays.append([(b[0], b[1], b[2], color) for b, color in boxes if b is not None])
            out = heat.copy()
            for text, org, scale, color in driver_lines(im):
                hershey.put_text(out, text, org, scale, color, 1)
            drawn.append(out)
        assert any((d != w).any() for d, w in zip(drawn, want))
        engine.cam_overlay_batch(res.items(), weight)
        engine.jpeg_overlay_batch([(d, info, ovs, None) for d, info, ovs in zip(res.d_im, infos, overlays)])
        engine.jpeg_encode_batch([(d, info, [], c.array) for d, info, c in zip(res.d_im, infos, coeffs)])
        engine.sync()
        assert_images(res.download(), drawn)
        for k, out in enumerate(drawn):
            assert jpegenc.entropy_encode(infos[k], coeffs[k].array.copy()) == jpegenc.encode_bgr(out), SHAPES[k]
    finally:
        res.close()
        for c in coeffs:
            c.close()


def test_two_calls_without_a_sync_between_them(engine, images, cases):
    """The second call's table and maxima go into the other set: the first call's launches still read theirs."""
    (w0, maps0, want0), (w1, maps1, want1) = cases[0], cases[1]
    first, second = Resident(engine, images[6:], maps0[6:]), Resident(engine, images[:6], maps1[:6])
    try:
        engine.cam_overlay_batch(first.items(), w0)
        engine.cam_overlay_batch(second.items(), w1)
        engine.sync()
        assert_images(first.download(), want0[6:], SHAPES[6:])
        assert_images(second.download(), want1[:6], SHAPES[:6])
        # a third and a fourth call reuse both sets, on the images the first two drew on
        engine.cam_overlay_batch(second.items(), w0)
        engine.cam_overlay_batch(first.items(), w1)
        engine.sync()
        assert_images(second.download(), [cam.overlay_image(a, m, w0) for a, m in zip(want1[:6], maps1[:6])], SHAPES[:6])
        assert_images(first.download(), [cam.overlay_image(a, m, w1) for a, m in zip(want0[6:], maps0[6:])], SHAPES[6:])
    finally:
        first.close()
        second.close()


def test_the_same_call_on_fresh_copies_gives_the_same_bytes(engine, images, cases):
    weight, maps, want = cases[0]
    got = []
    for _ in range(2):
        res = Resident(engine, images, maps)
        try:
            engine.cam_overlay_batch(res.items(), weight)
            engine.sync()
            got.append(res.download())
        finally:
            res.close()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(*got))
    assert_images(got[0], want)


def test_errors_enqueue_nothing_and_leave_the_handle_usable(engine, images, cases):
    weight, maps, want = cases[0]
    res = Resident(engine, images[:3], maps[:3])
    try:
        lib, h = engine.lib, engine.handle

        def targets(change=None):
            arr = (_capi.rn_cam_target * (MAX_BATCH + 1))()
            for k, (d_bgr, (hh, ww), d_cam, (mh, mw)) in enumerate(res.items()):
                arr[k].d_bgr, arr[k].height, arr[k].width, arr[k].d_cam, arr[k].cam_h, arr[k].cam_w = d_bgr, hh, ww, d_cam, mh, mw
            for k in range(3, MAX_BATCH + 1):
                arr[k] = arr[0]
            if change:
                change(arr)
            return arr

        assert lib.rn_cam_overlay_batch_device(h, targets(), 0, 0.5) == RN_E_RANGE
        assert lib.rn_cam_overlay_batch_device(h, targets(), -1, 0.5) == RN_E_RANGE
        assert lib.rn_cam_overlay_batch_device(h, targets(), MAX_BATCH + 1, 0.5) == RN_E_RANGE
        assert lib.rn_cam_overlay_batch_device(h, None, 3, 0.5) == RN_E_INVALID
        assert lib.rn_cam_overlay_batch_device(None, targets(), 3, 0.5) == RN_E_INVALID
        for bad in (-0.1, 1.0000001, float("nan"), float("inf")):
            assert lib.rn_cam_overlay_batch_device(h, targets(), 3, bad) == RN_E_INVALID, bad
        assert b"weight" in lib.rn_last_error()

        def no_image(a):
            a[1].d_bgr = None

        def no_map(a):
            a[2].d_cam = None

        def no_rows(a):
            a[0].height = 0

        def negative_width(a):
            a[2].width = -5

        def empty_map(a):
            a[1].cam_h = 0

        def negative_map(a):
            a[0].cam_w = -1

        for change in (no_image, no_map, no_rows, negative_width, empty_map, negative_map):
            assert lib.rn_cam_overlay_batch_device(h, targets(change), 3, 0.5) == RN_E_INVALID, change.__name__
        ms = C.c_float(0)
        assert lib.rn_cam_last_overlay_ms(h, None) == RN_E_INVALID and lib.rn_cam_last_overlay_ms(None, C.byref(ms)) == RN_E_INVALID
        with pytest.raises(ValueError):
            engine.cam_overlay_batch(res.items(), 2.0)
        engine.sync()
        assert_images(res.download(), images[:3])             # nothing was drawn
        engine.cam_overlay_batch(res.items(), weight)
        engine.sync()
        assert_images(res.download(), want[:3])
    finally:
        res.close()


@pytest.fixture(scope="module")
def jpeg_items(tmp_path_factory):
    """A landscape, a portrait and a square baseline JPEG file as classify_resident takes them: [(info, coefficients)]."""
    d = tmp_path_factory.mktemp("explain")
    out = []
    for k, (h, w) in enumerate([(300, 400), (401, 300), (224, 224)]):
        data = encode(str(d / ("e%d.jpg" % k)), content(h, w, ["smooth", "noise"][k % 2], seed=k), [2, 1, 0][k], quality=90)
        out.append(jpegdec.entropy_decode(data))
    return out


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_explain_resident_keeps_classify_residents_results_and_grad_cams_maps(weights, jpeg_items, dtype):
    eng = _capi.Engine(build_graph(6, 224), weights, device=0, dtype=dtype, max_batch=4)
    try:
        extra = np.ascontiguousarray(content(260, 300, "smooth", seed=8)[:, :, ::-1])
        ids0, probs0, addrs0, shapes0 = eng.classify_resident(jpeg_items, [extra])
        batch = np.empty((4, 224, 224, 3), np.uint8)
        eng.d2h(batch, eng._jpeg_dst)                     # the cropped, resized batch both calls run on
        for layer, side in (("s6.bn", 46), ("s7.bn", 21)):
            for cls in (None, [4, 0, 5, 2]):
                ids, probs, addrs, shapes, d_cams, map_shape = eng.explain_resident(jpeg_items, [extra], layer, class_ids=cls)
                assert ids.tobytes() == ids0.tobytes() and probs.tobytes() == probs0.tobytes()
                assert addrs == addrs0 and shapes == shapes0 == [(300, 400), (401, 300), (224, 224), (260, 300)]
                assert map_shape == (side, side) and len(d_cams) == 4
                got = np.empty((4, side, side), np.float32)
                for k, d in enumerate(d_cams):
                    eng.d2h(got[k], d)
                want, ids1, probs1 = eng.grad_cam(batch, class_ids=cls, layer=layer)
                assert got.tobytes() == want.tobytes(), (layer, cls)
                assert ids1.tobytes() == ids0.tobytes() and probs1.tobytes() == probs0.tobytes()
                assert got.max() > 0
        # the resident images take the maps: explain -> heat, downloaded, equals the host statement on the decoded files
        ids, probs, addrs, shapes, d_cams, map_shape = eng.explain_resident(jpeg_items, [extra], "s7.bn")
        maps = np.empty((4, 21, 21), np.float32)
        before = []
        for k, (h, w) in enumerate(shapes):
            eng.d2h(maps[k], d_cams[k])
            before.append(np.empty((h, w, 3), np.uint8))
            eng.d2h(before[k], addrs[k])
        eng.cam_overlay_batch([(addrs[k], shapes[k], d_cams[k], map_shape) for k in range(4)], 0.5)
        eng.sync()
        for k, (h, w) in enumerate(shapes):
            after = np.empty((h, w, 3), np.uint8)
            eng.d2h(after, addrs[k])
            np.testing.assert_array_equal(after, cam.overlay_image(before[k], maps[k], 0.5), err_msg=str((h, w)))
        with pytest.raises(ValueError):
            eng.explain_resident(jpeg_items, [extra], "s5.bn")
    finally:
        eng.close()


@pytest.mark.parametrize("dtype,layer", [("bf16", "s6.bn"), ("f32", "s7.bn")])
def test_classify_im_dir_draws_the_same_heat_maps_on_the_host_and_on_the_gpu(tmp_path, capsys, dtype, layer):
    from PIL import Image
    from roomnet_amd.infer import classify_im_dir
    from roomnet_amd.network import RoomNet
    nn = RoomNet(num_classes=6, im_side=224, compute_bn_mean_var=False, optimized_inference=True, max_batch=4, dtype=dtype)
    nn.load(MODEL_PREFIX)
    d = tmp_path / "images"
    os.makedirs(str(d))
    for k, (h, w) in enumerate([(150, 200), (201, 150), (224, 224), (120, 161), (96, 72)]):
        encode(str(d / ("b%d.jpg" % k)), content(h, w, ["smooth", "noise"][k % 2], seed=k), [2, 1, 0][k % 3], quality=90)
    encode(str(d / "prog.jpg"), content(150, 200, "smooth", seed=7), 2, quality=90, progressive=True)
    Image.fromarray(content(131, 150, "smooth", seed=8)).save(str(d / "p.png"))
    with open(str(d / "junk.jpg"), "wb") as f:
        f.write(b"\xff\xd8 not an image")
    out_dir = str(d) + "_classified"
    runs = {}
    capsys.readouterr()                   # (what loading the model printed)
    for arm, gpu, heat in (("host", False, layer), ("gpu", True, layer), ("plain", True, None)):
        xl = classify_im_dir(nn, str(d), overlay=True, batch_size=4, gpu_decode=gpu, gpu_encode=gpu, heatmap=heat, heatmap_weight=0.5)
        printed = capsys.readouterr().out
        files = {}
        for dirpath, _dirs, names in os.walk(out_dir):
            for name in names:
                p = os.path.join(dirpath, name)
                with open(p, "rb") as f:
                    files[os.path.relpath(p, out_dir)] = f.read()
                os.remove(p)
        with open(xl, "rb") as f:
            runs[arm] = (f.read(), printed, files)
        assert printed.count("unreadable image, skipped") == 1 and "junk.jpg" in printed
        assert printed.count("--->") == 8 and len(files) == 7
    for arm in ("host", "gpu"):
        assert runs[arm][1] == runs["plain"][1]
        assert runs[arm][0] == runs["plain"][0]
        assert sorted(runs[arm][2]) == sorted(runs["plain"][2])
    for name, data in runs["host"][2].items():
        assert runs["gpu"][2][name] == data, name
        assert runs["plain"][2][name] != data, name
    nn.sess.close()
