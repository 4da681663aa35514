"""GPU pixel stage of the split JPEG decoder (csrc/rn_jpeg.hip: rn_jpeg_decode_batch_device, rn_classify_jpegs) and the
drivers' gpu_decode path.  JPEG bytes are made with Pillow's encoder; the reference is Pillow's decode of the same bytes
through imageio.imread, byte for byte, and jpegdec.pixels_from_coeffs, the host restatement of the stage."""
import os

import numpy as np
import pytest

pytest.importorskip("PIL")

from conftest import MODEL_PREFIX  # noqa: E402
from jpeg_cases import SIZES, content, encode  # noqa: E402
from roomnet_amd import _capi, jpegdec  # noqa: E402
from roomnet_amd.graph import build_graph  # noqa: E402
from roomnet_amd.imageio import imread  # noqa: E402

pytestmark = pytest.mark.gpu

MAX_BATCH = 14
# 14 images: every size of the host test's list, samplings and contents rotating, so that every sampling meets odd sizes, sizes
# below one MCU, the <= 2-column replication case (31x2, 31x1, 1x1 at 4:2:0 / 4:2:2) and more than one workgroup (240x320)
MIXED = [(size, [2, 1, 0, "grey"][k % 4] if size not in ((31, 2), (240, 320)) else 2, ["noise", "smooth"][k % 2])
         for k, size in enumerate(SIZES)]


@pytest.fixture(scope="module")
def engine(weights):
    e = _capi.Engine(build_graph(6, 224), weights, device=0, dtype="bf16", max_batch=MAX_BATCH)
    yield e
    e.close()


@pytest.fixture(scope="module")
def mixed(tmp_path_factory):
    """[(info, coeffs, imread's image)] of the 14 mixed files; computed once."""
    d = tmp_path_factory.mktemp("jpeg_mixed")
    out = []
    for k, ((h, w), sampling, kind) in enumerate(MIXED):
        p = str(d / ("m%02d.jpg" % k))
        data = encode(p, content(h, w, kind, seed=k), sampling, quality=[90, 30, 100][k % 3],
                      **({"restart_marker_blocks": 3} if k % 5 == 1 else {}))
        info, coeffs = jpegdec.entropy_decode(data)
        out.append((info, coeffs, imread(p)))
    assert len(out) == 14 and {int(i.hsamp) * 10 + int(i.vsamp) for i, _c, _r in out} == {11, 21, 22}
    return out


def test_mixed_batch_is_byte_identical_to_imread_and_to_the_host_restatement(engine, mixed):
    items = [(info, coeffs) for info, coeffs, _ref in mixed]
    got = engine.jpeg_decode_batch(items)
    for k, (info, coeffs, ref) in enumerate(mixed):
        assert got[k].shape == ref.shape, MIXED[k]
        np.testing.assert_array_equal(got[k], ref, err_msg=str(MIXED[k]))
        np.testing.assert_array_equal(got[k], jpegdec.pixels_from_coeffs(info, coeffs), err_msg=str(MIXED[k]))
    again = engine.jpeg_decode_batch(items)
    for a, b in zip(got, again):
        np.testing.assert_array_equal(a, b)
    assert engine.jpeg_last_decode_ms() > 0


def test_back_to_back_decodes_without_a_sync(engine, mixed):
    """The contract include/roomnet_hip.h states for rn_jpeg_decode_batch_device: back-to-back calls without a sync are fine.
    Three calls with three different tables into separate destinations -- the first half of the mixed files, the second half, the
    first half reversed (on the first call's table set) -- no sync between them, one at the end; every image as the mixed-batch test
    checks it.  A contract, not a regression trap: a library whose single table happened to be copied in time passes it too."""
    import ctypes as C
    half = len(mixed) // 2
    calls = [mixed[:half], mixed[half:], mixed[:half][::-1]]
    d_outs = [[engine.device_malloc(ref.nbytes) for _info, _coeffs, ref in call] for call in calls]
    try:
        for call, ds in zip(calls, d_outs):
            arr = engine._jpeg_images([(info, coeffs) for info, coeffs, _ref in call])
            _capi._check(engine.lib, engine.lib.rn_jpeg_decode_batch_device(engine.handle, arr, len(call), (C.c_void_p * len(call))(*ds)),
                         "rn_jpeg_decode_batch_device")
        engine.sync()
        for k, (call, ds) in enumerate(zip(calls, d_outs)):
            for i, ((info, coeffs, ref), d) in enumerate(zip(call, ds)):
                got = np.empty(ref.shape, np.uint8)
                engine.d2h(got, d)
                what = "call %d, image %d (%dx%d)" % (k + 1, i, info.width, info.height)
                np.testing.assert_array_equal(got, ref, err_msg=what)
                np.testing.assert_array_equal(got, jpegdec.pixels_from_coeffs(info, coeffs), err_msg=what)
        assert engine.jpeg_last_decode_ms() > 0
    finally:
        for d in [d for ds in d_outs for d in ds]:
            engine.device_free(d)


@pytest.mark.parametrize("n", [1, MAX_BATCH])
def test_batch_of_one_and_of_max_batch(engine, mixed, n):
    pick = [mixed[-1]] if n == 1 else [mixed[(3 * k) % len(mixed)] for k in range(n)]
    got = engine.jpeg_decode_batch([(info, coeffs) for info, coeffs, _ref in pick])
    assert len(got) == n
    for g, (_info, _coeffs, ref) in zip(got, pick):
        np.testing.assert_array_equal(g, ref)


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_classify_jpegs_equals_classify_images_of_the_pillow_decode(weights, tmp_path, dtype):
    eng = _capi.Engine(build_graph(6, 224), weights, device=0, dtype=dtype, max_batch=8)
    try:
        items, refs = [], []
        for k in range(8):
            h, w = ((300, 400), (400, 300))[k % 2]
            p = str(tmp_path / ("c%d.jpg" % k))
            data = encode(p, content(h, w, ["smooth", "noise"][(k // 2) % 2], seed=k), [0, 1, 2][k % 3], quality=90)
            items.append(jpegdec.entropy_decode(data))
            refs.append(imread(p))
        want_ids, want_probs = eng.classify_images(refs)
        ids, probs = eng.classify_jpegs(items)
        np.testing.assert_array_equal(ids, want_ids)
        np.testing.assert_array_equal(probs, want_probs)
        ids2, probs2 = eng.classify_jpegs(items[:3])           # a smaller batch on the grown scratch
        np.testing.assert_array_equal(ids2, want_ids[:3])
        np.testing.assert_array_equal(probs2, want_probs[:3])
    finally:
        eng.close()


def test_errors_leave_the_handle_usable(engine, mixed):
    items = [(info, coeffs) for info, coeffs, _ref in mixed]
    lib, h = engine.lib, engine.handle
    arr = engine._jpeg_images(items)
    d = engine.device_malloc(1 << 20)
    try:
        import ctypes as C
        ptrs = (C.c_void_p * (MAX_BATCH + 1))(*([d] * (MAX_BATCH + 1)))
        assert lib.rn_jpeg_decode_batch_device(h, arr, 0, ptrs) == -5                      # RN_E_RANGE
        assert lib.rn_jpeg_decode_batch_device(h, arr, MAX_BATCH + 1, ptrs) == -5
        probs, ids = np.empty((MAX_BATCH + 1, 6), np.float32), np.empty(MAX_BATCH + 1, np.int64)
        assert lib.rn_classify_jpegs(h, arr, 0, probs.ctypes.data, ids.ctypes.data) == -5
        assert lib.rn_classify_jpegs(h, arr, MAX_BATCH + 1, probs.ctypes.data, ids.ctypes.data) == -5
        bad = engine._jpeg_images(items[:2])
        bad[1].info.supported = 0
        assert lib.rn_jpeg_decode_batch_device(h, bad, 2, ptrs) == -1                      # RN_E_INVALID
        assert b"not a supported JPEG" in lib.rn_last_error()
        bad[1].info.supported = 1
        bad[1].info.blocks_w[0] += 1                                                       # a block grid the sizes do not give
        assert lib.rn_jpeg_decode_batch_device(h, bad, 2, ptrs) == -1
    finally:
        engine.device_free(d)
    got = engine.jpeg_decode_batch(items[:2])
    np.testing.assert_array_equal(got[1], mixed[1][2])


def test_classify_im_dir_writes_the_same_workbook_with_gpu_decode(tmp_path, capsys):
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
    xls = {}
    for arm in (False, True):             # the same directory twice: the second run overwrites the first one's outputs
        with open(classify_im_dir(nn, str(d), overlay=False, batch_size=4, gpu_decode=arm), "rb") as f:
            xls[arm] = f.read()
        out = capsys.readouterr().out
        assert out.count("unreadable image, skipped") == 1 and "junk.jpg" in out
        assert out.count("--->") == 9
    assert xls[True] == xls[False]
    with pytest.raises(ValueError):
        classify_im_dir(nn, str(d), overlay=True, gpu_decode=True)
    # the batches recalibrate_from_dir / fine_tune_from_list feed with gpu_decode=True: the bytes of the host preparation
    paths = sorted(os.path.join(str(d), f) for f in os.listdir(str(d)))
    at, batches, bad = [], [], []
    for a, b, c in nn.prepare_files(paths, batch_size=4):
        at, batches, bad = at + a, batches + [b], bad + c
    assert [os.path.basename(paths[i]) for i in bad] == ["junk.jpg"] and sorted(at + bad) == list(range(9))
    np.testing.assert_array_equal(np.concatenate(batches, 0), nn._batch_from([imread(paths[i]) for i in at], "test"))
    nn.sess.close()
