"""GPU overlay and pixel stage of the split JPEG encoder (csrc/rn_jpeg_enc.hip: rn_jpeg_overlay_batch_device,
rn_jpeg_encode_batch_device) and classify_im_dir's gpu_encode path.  The references: jpegenc.coeffs_from_pixels, the host
restatement of the stage (exactly), Pillow's encoder through imageio.imwrite (byte for byte), and hershey.put_text for the overlay
(byte for byte)."""
import os

import numpy as np
import pytest

pytest.importorskip("PIL")

from conftest import MODEL_PREFIX  # noqa: E402
from jpeg_cases import content, encode  # noqa: E402
from roomnet_amd import _capi, hershey, jpegdec, jpegenc  # noqa: E402
from roomnet_amd.graph import build_graph  # noqa: E402
from roomnet_amd.imageio import imwrite  # noqa: E402

pytestmark = pytest.mark.gpu

# the smallest shapes at which each rule of the stage can go wrong: one MCU, an even height that is no multiple of 16 (8x24, 72x96,
# 120x200: the chroma rows below the image), odd sizes, dummy luma blocks to the right and below (8x24, 37x53, 17x33), one pixel,
# two columns, more than one workgroup of blocks (240x320)
SHAPES = [(16, 16), (8, 24), (37, 53), (17, 33), (1, 1), (31, 2), (50, 49), (72, 96), (120, 200), (240, 320)]
MAX_BATCH = 10
RN_E_INVALID, RN_E_RANGE = -1, -5


@pytest.fixture(scope="module")
def engine(weights):
    e = _capi.Engine(build_graph(6, 224), weights, device=0, dtype="bf16", max_batch=MAX_BATCH)
    yield e
    e.close()


@pytest.fixture(scope="module")
def images():
    """BGR images of SHAPES, noise and smooth content alternating; never modified."""
    ims = [np.ascontiguousarray(content(h, w, ["noise", "smooth"][k % 2], seed=k)[:, :, ::-1]) for k, (h, w) in enumerate(SHAPES)]
    for im in ims:
        im.setflags(write=False)
    return ims


@pytest.fixture(scope="module")
def pillow_files(images, tmp_path_factory):
    """The file imageio.imwrite writes for each image; computed once."""
    d = tmp_path_factory.mktemp("jpegenc")
    out = []
    for k, im in enumerate(images):
        p = str(d / ("p%d.jpg" % k))
        assert imwrite(p, im)
        with open(p, "rb") as f:
            out.append(f.read())
    return out


def driver_overlays(im, label="LivingRoom", conf=np.float32(0.98765)):
    """The two lines infer._overlay_and_write draws, as (x, y, coverage, colour) and as put_text arguments."""
    h, w = im.shape[:2]
    lines = [("Predicted Class: " + label, (int(.5 * w), int(.90 * h)), (h / 720.) * .85, (0, 255, 0)),
             ("Confidence: " + str(round(conf * 100, 2)) + " %", (int(.5 * w), int(.95 * h)), (h / 720.) * .85, (255, 0, 0))]
    ovs = []
    for text, org, scale, color in lines:
        box = hershey.coverage(text, org, scale, (h, w), 1)
        if box is not None:
            ovs.append((box[0], box[1], box[2], color))
    return ovs, lines


def drawn_on_host(im, lines):
    out = im.copy()
    for text, org, scale, color in lines:
        hershey.put_text(out, text, org, scale, color, 1)
    return out


class Uploaded:
    """Images in device memory, a page-locked coefficient buffer each."""

    def __init__(self, engine, ims):
        self.engine, self.ims = engine, ims
        self.infos = [jpegenc.encode_info(im.shape[0], im.shape[1]) for im in ims]
        self.d = [engine.device_malloc(im.nbytes) for im in ims]
        self.coeffs = [_capi.PinnedArray((jpegdec.coeff_count(i),), np.int16) for i in self.infos]
        for c in self.coeffs:
            c.array[:] = 12345
        for d, im in zip(self.d, ims):
            engine.h2d(d, im)

    def items(self, overlays=None):
        return [(d, info, overlays[k] if overlays else [], c.array) for k, (d, info, c) in enumerate(zip(self.d, self.infos, self.coeffs))]

    def download(self):
        out = [np.empty(im.shape, np.uint8) for im in self.ims]
        for a, d in zip(out, self.d):
            self.engine.d2h(a, d)
        return out

    def close(self):
        for d in self.d:
            self.engine.device_free(d)
        for c in self.coeffs:
            c.close()


def test_mixed_batch_equals_the_host_restatement_and_pillows_files(engine, images, pillow_files):
    up = Uploaded(engine, images)
    try:
        engine.jpeg_encode_batch(up.items())
        engine.sync()
        for k, im in enumerate(images):
            got = up.coeffs[k].array.copy()
            np.testing.assert_array_equal(got, jpegenc.coeffs_from_pixels(up.infos[k], im), err_msg=str(SHAPES[k]))
            assert jpegenc.entropy_encode(up.infos[k], got) == pillow_files[k], SHAPES[k]
        for a, im in zip(up.download(), images):
            np.testing.assert_array_equal(a, im)              # (no overlay: the source is untouched)
        assert engine.jpeg_last_encode_ms() > 0
    finally:
        up.close()


def test_overlay_equals_put_text_and_the_encode_equals_encode_bgr(engine, images):
    up = Uploaded(engine, images)
    try:
        both = [driver_overlays(im) for im in images]
        assert all(len(ovs) == 2 for ovs, _l in both)
        y1, y2 = both[8][0][0][1] + both[8][0][0][2].shape[0], both[8][0][1][1]
        assert SHAPES[8] == (120, 200) and y2 < y1, "the two boxes of the 120-row image overlap"
        engine.jpeg_overlay_batch(up.items([ovs for ovs, _l in both]))
        engine.sync()
        want = [drawn_on_host(im, lines) for im, (_o, lines) in zip(images, both)]
        for k, a in enumerate(up.download()):
            np.testing.assert_array_equal(a, want[k], err_msg=str(SHAPES[k]))
        assert any((w != im).any() for w, im in zip(want, images))
        engine.jpeg_encode_batch(up.items())
        engine.sync()
        for k, w in enumerate(want):
            assert jpegenc.entropy_encode(up.infos[k], up.coeffs[k].array.copy()) == jpegenc.encode_bgr(w), SHAPES[k]
    finally:
        up.close()


def test_errors_enqueue_nothing_and_leave_the_handle_usable(engine, images):
    up = Uploaded(engine, images[:3])
    try:
        lib, h = engine.lib, engine.handle
        ovs = [driver_overlays(im)[0] for im in images[:3]]
        big, _keep_big = engine._jpeg_sources(up.items() * 4)             # 12 entries
        for fn in (lib.rn_jpeg_encode_batch_device, lib.rn_jpeg_overlay_batch_device):
            assert fn(h, big, 0) == RN_E_RANGE
            assert fn(h, big, MAX_BATCH + 1) == RN_E_RANGE

            def rc(change, fn=fn):
                arr, _keep = engine._jpeg_sources(up.items(ovs))
                change(arr)
                return fn(h, arr, 3)

            def unsupported(a):
                a[1].info.supported = 0

            def grid(a):
                a[1].info.blocks_w[0] += 1

            def grey(a):
                a[2].info.ncomp = 1

            def box_right(a):
                a[0].overlays[1].x = a[0].info.width - a[0].overlays[1].w + 1

            def box_below(a):
                a[2].overlays[0].y = a[2].info.height - a[2].overlays[0].h + 1

            def box_negative(a):
                a[0].overlays[0].x = -1

            def box_empty(a):
                a[0].overlays[0].w = 0

            def no_coverage(a):
                a[1].overlays[1].coverage = None

            def too_many(a):
                a[1].n_overlays = _capi.RN_JPEG_MAX_OVERLAYS + 1

            def no_image(a):
                a[0].d_bgr = None

            for change in (unsupported, grid, grey, box_right, box_below, box_negative, box_empty, no_coverage, too_many, no_image):
                assert rc(change) == RN_E_INVALID, change.__name__

        def no_coeffs(a):
            a[2].coeffs = None
        arr, _keep = engine._jpeg_sources(up.items(ovs))
        no_coeffs(arr)
        assert lib.rn_jpeg_encode_batch_device(h, arr, 3) == RN_E_INVALID
        assert b"coefficient buffer" in lib.rn_last_error()
        engine.sync()
        for a, im in zip(up.download(), images[:3]):
            np.testing.assert_array_equal(a, im)              # nothing was drawn
        assert all((c.array == 12345).all() for c in up.coeffs)
        engine.jpeg_encode_batch(up.items(ovs))
        engine.sync()
        for k, im in enumerate(images[:3]):
            want = drawn_on_host(im, driver_overlays(im)[1])
            assert jpegenc.entropy_encode(up.infos[k], up.coeffs[k].array.copy()) == jpegenc.encode_bgr(want), SHAPES[k]
    finally:
        up.close()


def test_two_calls_without_a_sync_between_them(engine, images):
    """The second call's tables and coverages go into the other set: the first call's launches still read theirs."""
    first, second = Uploaded(engine, images[5:]), Uploaded(engine, images[:5])
    try:
        ov1 = [driver_overlays(im, "Bathroom", np.float32(0.5))[0] for im in first.ims]
        ov2 = [driver_overlays(im, "Backyard", np.float32(0.123456))[0][::-1] for im in second.ims]      # other texts, other order
        engine.jpeg_encode_batch(first.items(ov1))
        engine.jpeg_encode_batch(second.items(ov2))
        engine.sync()
        for up, ovs in ((first, ov1), (second, ov2)):
            for k, im in enumerate(up.ims):
                want = im.copy()
                for x, y, cov, color in ovs[k]:
                    hershey.blend(want, x, y, cov, color)
                assert jpegenc.entropy_encode(up.infos[k], up.coeffs[k].array.copy()) == jpegenc.encode_bgr(want), im.shape
        # a third and a fourth call reuse both sets
        engine.jpeg_encode_batch(first.items())
        engine.jpeg_encode_batch(second.items())
        engine.sync()
        got = first.download()
        assert jpegenc.entropy_encode(first.infos[0], first.coeffs[0].array.copy()) == jpegenc.encode_bgr(got[0])
    finally:
        first.close()
        second.close()


def test_classify_im_dir_writes_the_same_files_with_gpu_decode_and_gpu_encode(tmp_path, capsys):
    from PIL import Image
    from roomnet_amd.infer import classify_im_dir
    from roomnet_amd.network import RoomNet
    nn = RoomNet(num_classes=6, im_side=224, compute_bn_mean_var=False, optimized_inference=True, max_batch=4, dtype="bf16")
    nn.load(MODEL_PREFIX)
    d = tmp_path / "images"
    os.makedirs(str(d))
    for k in range(6):
        h, w = ((300, 400), (400, 300), (224, 224))[k % 3]
        encode(str(d / ("b%d.jpg" % k)), content(h, w, ["smooth", "noise"][k % 2], seed=k), [2, 1, 0][k % 3], quality=90)
    encode(str(d / "prog.jpg"), content(300, 400, "smooth", seed=7), 2, quality=90, progressive=True)
    Image.fromarray(content(260, 300, "smooth", seed=8)).save(str(d / "p.png"))
    with open(str(d / "junk.jpg"), "wb") as f:
        f.write(b"\xff\xd8 not an image")
    out_dir = str(d) + "_classified"
    runs = {}
    capsys.readouterr()                   # (what loading the model printed)
    for arm in (False, True):             # the same directory twice: the second run overwrites the first one's outputs
        xl = classify_im_dir(nn, str(d), overlay=True, batch_size=4, gpu_decode=arm, gpu_encode=arm)
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
        assert printed.count("--->") == 9 and len(files) == 8
    assert runs[True][1] == runs[False][1]
    assert runs[True][0] == runs[False][0]
    assert sorted(runs[True][2]) == sorted(runs[False][2])
    for name, data in runs[False][2].items():
        assert runs[True][2][name] == data, name
    with pytest.raises(ValueError):
        classify_im_dir(nn, str(d), overlay=False, gpu_decode=True, gpu_encode=True)
    with pytest.raises(ValueError):
        classify_im_dir(nn, str(d), overlay=True, gpu_decode=False, gpu_encode=True)
    nn.sess.close()
