"""Occlusion-sensitivity maps on the GPU (csrc/rn_occlusion.hip: rn_occlusion_*), Engine.occlusion_resident and classify_im_dir's
heatmap="occlusion" path.  The reference is roomnet_amd/occlusion.py with the handle's own forward pass on the same chunks: the
mask bytes, the drops and the maps are compared for equality, no comparison here takes a tolerance."""
import ctypes as C
import os

import numpy as np
import pytest

import checkpoints as CK
from conftest import MODEL_PREFIX, parity_set_of
from roomnet_amd import _capi, occlusion as O
from roomnet_amd.graph import build_graph

pytestmark = pytest.mark.gpu

MAX_BATCH = 32
RN_E_INVALID, RN_E_RANGE = -1, -5
PICK = [14, 41, 52]                      # a seeded textured image and two of the class-covering field images of the parity set
P, T = 64, 48                            # 5 x 5 windows at 224: 75 masked passes for 3 images, chunks of 32 / 32 / 11


@pytest.fixture(scope="module")
def ims(parity_images):
    return np.ascontiguousarray(parity_images[PICK])


@pytest.fixture(scope="module")
def engines(weights):
    made = {}

    def get(dtype):
        if dtype not in made:
            made[dtype] = _capi.Engine(build_graph(6, 224), weights, device=0, dtype=dtype, max_batch=MAX_BATCH)
        return made[dtype]

    yield get
    for e in made.values():
        e.close()


class Dev:
    """Device buffers of one test, freed together."""

    def __init__(self, eng):
        self.eng, self.ptrs = eng, []

    def put(self, a):
        a = np.ascontiguousarray(a)
        d = self.eng.device_malloc(a.nbytes)
        self.ptrs.append(d)
        self.eng.h2d(d, a)
        return d

    def room(self, nbytes):
        d = self.eng.device_malloc(nbytes)
        self.ptrs.append(d)
        return d

    def get(self, d, shape, dtype):
        out = np.empty(shape, dtype)
        self.eng.d2h(out, d)
        return out

    def close(self):
        for d in self.ptrs:
            self.eng.device_free(d)


def masks_of(eng, batch, patch, stride, fill, first, count):
    dev = Dev(eng)
    try:
        s = batch.shape[1]
        d_out = dev.room(count * s * s * 3)
        eng.occlusion_masks_device(dev.put(batch), len(batch), patch, stride, fill, first, count, d_out)
        eng.sync()
        return dev.get(d_out, (count, s, s, 3), np.uint8)
    finally:
        dev.close()


class Call:
    """One rn_occlusion_u8_device call in three steps, so that several calls can be enqueued with nothing between them: the
    constructor allocates and uploads (Engine.h2d waits for the handle's stream), ``enqueue`` only enqueues, ``read`` syncs."""

    def __init__(self, eng, dev, batch, class_ids, patch, stride, fill):
        self.eng, self.dev, self.patch, self.stride, self.fill = eng, dev, patch, stride, fill
        self.n, self.s, self.nc = len(batch), batch.shape[1], eng.graph.num_classes
        self.g = O.grid(self.s, patch, stride)
        self.d_cls = dev.put(np.asarray(class_ids, np.int32)) if class_ids is not None else None
        self.d_drop, self.d_map = dev.room(self.n * self.g * self.g * 4), dev.room(self.n * self.s * self.s * 4)
        self.d_probs, self.d_ids = dev.room(self.n * self.nc * 4), dev.room(self.n * 8)
        self.d_bgr = dev.put(batch)

    def enqueue(self):
        self.eng.occlusion_u8_device(self.d_bgr, self.n, self.d_cls, self.patch, self.stride, self.fill, self.d_drop, self.d_map,
                                     self.d_probs, self.d_ids)

    def read(self):
        self.eng.sync()
        n, s, g, get = self.n, self.s, self.g, self.dev.get
        return (get(self.d_map, (n, s, s), np.float32), get(self.d_drop, (n, g, g), np.float32), get(self.d_ids, (n,), np.int64),
                get(self.d_probs, (n, self.nc), np.float32))


def device_call(eng, batch, class_ids, patch, stride, fill):
    """rn_occlusion_u8_device on uploaded images -> (maps, drops, ids, probs)."""
    dev = Dev(eng)
    try:
        call = Call(eng, dev, batch, class_ids, patch, stride, fill)
        call.enqueue()
        return call.read()
    finally:
        dev.close()


def host_call(eng, batch, class_ids, patch, stride, fill):
    """The NumPy statement over rn_forward_u8 of the same handle: the same chunk sizes, so the same launches."""
    return O.occlusion_map_host(lambda b: eng.forward_u8(b)[1], batch, class_ids=class_ids, patch=patch, stride=stride, fill=fill,
                                max_batch=eng.max_batch)


def assert_same(got, want, what=""):
    for name, a, b in zip(("map", "drop", "ids", "probs"), got, want):
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name)
        if not np.array_equal(a, b):
            at = np.argwhere(a != b)
            raise AssertionError("%s %s: %d of %d entries differ, first at %s: %r != %r" % (what, name, len(at), a.size, at[0].tolist(),
                                                                                             a[tuple(at[0])], b[tuple(at[0])]))


# ------------------------------------------------------------------------------------------------ 1. mask bytes
@pytest.mark.parametrize("fill", ["mean", (7, 200, 31)])
def test_mask_bytes_at_224_across_an_image_boundary(engines, ims, fill):
    eng = engines("bf16")
    want = np.concatenate([O.windows(im, P, T, fill) for im in ims])[20:52]           # 25 windows per image: images 0, 1 and 2
    got = masks_of(eng, ims, P, T, fill, 20, 32)
    np.testing.assert_array_equal(got, want)
    assert (got != np.repeat(ims, 25, 0)[20:52]).any(axis=(1, 2, 3)).all()             # every one of them is masked
    if fill == "mean":               # index 20 is image 0's window (4, 0) at row 160; 25 and 50 are the first windows of images 1 and 2
        assert [got[0][160, 0].tolist(), got[5][0, 0].tolist(), got[30][0, 0].tolist()] == [O.fill_colour(im).tolist() for im in ims]
    # the last masked image of the call, alone, and the whole first chunk
    np.testing.assert_array_equal(masks_of(eng, ims, P, T, fill, 74, 1)[0], O.windows(ims[2], P, T, fill)[24])
    np.testing.assert_array_equal(masks_of(eng, ims, P, T, fill, 0, 32), np.concatenate([O.windows(im, P, T, fill) for im in ims[:2]])[:32])


@pytest.mark.parametrize("fill", ["mean", (255, 0, 128)])
def test_mask_bytes_at_185_take_the_byte_path(fill):
    """3 * 185 is no multiple of 4: rows and images start at any byte, window edges fall inside dwords (P = 7, T = 5)."""
    side = 185
    g = build_graph(6, side)
    batch = np.ascontiguousarray(parity_set_of(side)[[17, 45]])
    eng = _capi.Engine(g, CK.live(g, 0, CK.LIVE_GAIN), device=0, dtype="bf16", max_batch=MAX_BATCH)
    try:
        G = O.grid(side, 7, 5)
        pos = O.positions(side, 7, 5)
        assert G == 37 and pos[-2:] == [175, 178]
        np.testing.assert_array_equal(O.windows(batch[1], 7, 5, fill)[G + 36], O.masked(batch[1], 5, 178, 7, fill))
        # the end of image 0's windows and the start of image 1's; the flush last column and row; the very last window
        for first, count in ((G * G - 20, 32), (G - 3, 6), (2 * G * G - 5, 5)):
            # (entry f % G^2 of occlusion.windows of image f // G^2, without building all 1369 of them)
            want = np.stack([O.masked(batch[f // (G * G)], pos[f % (G * G) // G], pos[f % G], 7, fill) for f in range(first, first + count)])
            np.testing.assert_array_equal(masks_of(eng, batch, 7, 5, fill, first, count), want, err_msg=str((first, count)))
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ 2. drops and maps
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_drops_and_maps_equal_the_host_statement_over_the_same_forward(engines, ims, dtype):
    eng = engines(dtype)
    assert eng.occlusion_plan(3, P, T) == (5, 75, 3)
    ids_f, probs_f = eng.forward_u8(ims)
    got = device_call(eng, ims, None, P, T, "mean")
    assert np.array_equal(got[2], ids_f) and np.array_equal(got[3], probs_f)
    want = host_call(eng, ims, None, P, T, "mean")
    print("%s: drops of image 0\n%s\nmap range %g .. %g, %.3f ms on the device" % (dtype, got[1][0], got[0].min(), got[0].max(),
                                                                                  eng.occlusion_last_ms()))
    assert_same(got, want, dtype)
    assert np.abs(got[1]).max() > 0 and np.isfinite(got[0]).all()
    # the blocking host form returns the same
    assert_same(eng.occlusion_u8(ims, patch=P, stride=T), want, dtype + " rn_occlusion_u8")
    maps, drops, ids, probs = eng.occlusion_u8(ims, patch=P, stride=T, with_map=False)
    assert maps is None and np.array_equal(drops, want[1])


# ------------------------------------------------------------------------------------------------ 3. class and edge cases
def test_given_classes_one_window_and_back_to_back_calls(engines, ims):
    eng = engines("bf16")
    ids_f, probs_f = eng.forward_u8(ims)
    other = ((ids_f + 1) % 6).astype(np.int32)
    cls = np.array([ids_f[0], other[1], other[2]], np.int32)               # the argmax and two classes that are not
    got = device_call(eng, ims, cls, P, T, (0, 0, 0))
    assert_same(got, host_call(eng, ims, cls, P, T, (0, 0, 0)), "given classes")
    assert np.array_equal(got[2], ids_f) and np.array_equal(got[3], probs_f)
    assert not np.array_equal(got[1][1], device_call(eng, ims, None, P, T, (0, 0, 0))[1][1])
    # P = S: one window, the whole image is the fill; the map is that one drop everywhere
    one = device_call(eng, ims, None, 224, 7, "mean")
    assert one[1].shape == (3, 1, 1)
    assert_same(one, host_call(eng, ims, None, 224, 7, "mean"), "P = S")
    assert np.array_equal(one[0], np.broadcast_to(one[1], (3, 224, 224)))
    # calls back to back with different (P, T, fill) and NO sync between them: every buffer is allocated and uploaded first (an
    # upload waits for the stream), no class ids are given (the library reads those back, which waits too), then the calls are
    # enqueued one after the other and the stream is drained once.  They share the handle's masked chunk, its probabilities and
    # the per-image fills: the third call's mean fills of other images must not reach the first call's masks.
    cases = [(ims, 96, 64, "mean"), (ims[:2], 80, 72, (255, 255, 255)), (np.ascontiguousarray(ims[::-1]), 64, 48, "mean")]
    dev = Dev(eng)
    try:
        calls = [Call(eng, dev, batch, None, patch, stride, fill) for batch, patch, stride, fill in cases]
        eng.sync()
        for call in calls:
            call.enqueue()
        got = [call.read() for call in calls]
    finally:
        dev.close()
    for k, (batch, patch, stride, fill) in enumerate(cases):
        assert_same(got[k], host_call(eng, batch, None, patch, stride, fill), "call %d of %d back to back" % (k + 1, len(cases)))


# ------------------------------------------------------------------------------------------------ 4. refusals
def test_refusals_enqueue_nothing_and_leave_the_handle_usable(engines, ims, golden_parity):
    eng = engines("bf16")
    lib, h = eng.lib, eng.handle
    ids_f, probs_f = eng.forward_u8(ims)
    assert np.array_equal(ids_f, golden_parity["ids"][PICK])
    dev = Dev(eng)
    try:
        d_bgr = dev.put(ims)
        d_bad = dev.put(np.array([0, 6, 1], np.int32))
        d_neg = dev.put(np.array([0, 1, -1], np.int32))
        d_drop, d_map, d_probs, d_ids = dev.room(75 * 4), dev.room(3 * 224 * 224 * 4), dev.room(3 * 6 * 4), dev.room(3 * 8)
        d_out = dev.room(MAX_BATCH * 224 * 224 * 3)
        for b in (d_drop, d_map, d_probs, d_ids):
            eng.h2d(b, np.full(3 * 6 if b == d_probs else (75 if b == d_drop else 6), 0x5A5A5A5A, np.uint32))
        v = C.c_void_p

        def full(n=3, cls=None, patch=P, stride=T):
            return lib.rn_occlusion_u8_device(h, v(d_bgr), n, v(cls) if cls else None, patch, stride, None, v(d_drop), v(d_map), v(d_probs),
                                              v(d_ids))

        def masks(n=3, patch=P, stride=T, first=0, count=32):
            return lib.rn_occlusion_masks_device(h, v(d_bgr), n, patch, stride, None, first, count, v(d_out))

        def still_usable():
            # (the golden file holds the float64 reference, not this handle's bf16 bits: the ids were compared with it above, the
            #  probabilities are compared with the same handle's own result from before the first refusal -- weaker than committed
            #  bits would be, and all that exists to compare with)
            ids, probs = eng.forward_u8(ims)
            assert np.array_equal(ids, ids_f) and np.array_equal(probs, probs_f)

        for what, call, rc in [("T > P", lambda: full(patch=32, stride=33), RN_E_INVALID),
                               ("P > S", lambda: full(patch=225, stride=16), RN_E_INVALID),
                               ("class id 6", lambda: full(cls=d_bad), RN_E_INVALID),
                               ("class id -1", lambda: full(cls=d_neg), RN_E_INVALID),
                               ("n = 0", lambda: full(n=0), RN_E_INVALID),
                               ("n > max_batch", lambda: full(n=MAX_BATCH + 1), RN_E_RANGE),
                               ("masks: T > P", lambda: masks(patch=32, stride=33), RN_E_INVALID),
                               ("masks: n = 0", lambda: masks(n=0), RN_E_INVALID),
                               ("masks: count > max_batch", lambda: masks(count=MAX_BATCH + 1), RN_E_RANGE),
                               ("masks: count = 0", lambda: masks(count=0), RN_E_RANGE),
                               ("masks: past the end", lambda: masks(first=60, count=16), RN_E_RANGE),
                               ("masks: first < 0", lambda: masks(first=-1, count=4), RN_E_RANGE)]:
            assert call() == rc, what
            assert b"rn_occlusion" in lib.rn_last_error(), what
            still_usable()
        assert lib.rn_occlusion_u8_device(h, None, 3, None, P, T, None, v(d_drop), v(d_map), v(d_probs), v(d_ids)) == RN_E_INVALID
        assert lib.rn_occlusion_u8_device(None, v(d_bgr), 3, None, P, T, None, v(d_drop), v(d_map), v(d_probs), v(d_ids)) == RN_E_INVALID
        ms = C.c_float(0)
        assert lib.rn_occlusion_last_ms(h, None) == RN_E_INVALID and lib.rn_occlusion_last_ms(None, C.byref(ms)) == RN_E_INVALID
        with pytest.raises(ValueError):
            eng.occlusion_u8(ims, patch=32, stride=33)
        with pytest.raises(ValueError):
            eng.occlusion_u8(ims, class_ids=[0, 1, 6], patch=P, stride=T)
        with pytest.raises(ValueError):
            eng.occlusion_u8(ims, patch=P, stride=T, fill="median")
        # nothing was enqueued: the result buffers still hold what was put there
        eng.sync()
        assert (dev.get(d_drop, (75,), np.uint32) == 0x5A5A5A5A).all() and (dev.get(d_probs, (18,), np.uint32) == 0x5A5A5A5A).all()
        # ... and the same buffers take a good call
        assert full() == 0
        eng.sync()
        assert np.array_equal(dev.get(d_probs, (3, 6), np.float32), probs_f)
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------------ 5. resident chunk and drivers
@pytest.fixture(scope="module")
def jpeg_dir(tmp_path_factory):
    pytest.importorskip("PIL")
    from jpeg_cases import content, encode
    d = tmp_path_factory.mktemp("occlusion") / "images"
    os.makedirs(str(d))
    for k, (h, w) in enumerate([(150, 200), (201, 150), (224, 224)]):          # a landscape, a portrait and a square file
        encode(str(d / ("o%d.jpg" % k)), content(h, w, ["smooth", "noise"][k % 2], seed=k), [2, 1, 0][k], quality=90)
    return d


def test_occlusion_resident_keeps_the_maps_on_the_device(weights, jpeg_dir):
    from roomnet_amd import cam, jpegdec
    eng = _capi.Engine(build_graph(6, 224), weights, device=0, dtype="bf16", max_batch=4)
    try:
        items = [jpegdec.entropy_decode(open(str(jpeg_dir / ("o%d.jpg" % k)), "rb").read()) for k in range(3)]
        ids0, probs0, addrs0, shapes0 = eng.classify_resident(items, [])
        batch = np.empty((3, 224, 224, 3), np.uint8)
        eng.d2h(batch, eng._jpeg_dst)
        for cls in (None, [4, 0, 5]):
            ids, probs, addrs, shapes, d_maps, map_shape = eng.occlusion_resident(items, [], P, T, "mean", class_ids=cls)
            assert ids.tobytes() == ids0.tobytes() and probs.tobytes() == probs0.tobytes()
            assert addrs == addrs0 and shapes == shapes0 == [(150, 200), (201, 150), (224, 224)] and map_shape == (224, 224)
            got = np.empty((3, 224, 224), np.float32)
            for k, d in enumerate(d_maps):
                eng.d2h(got[k], d)
            want = eng.occlusion_u8(batch, class_ids=cls, patch=P, stride=T)
            assert got.tobytes() == want[0].tobytes(), cls
        before = []
        for k, (h, w) in enumerate(shapes):
            before.append(np.empty((h, w, 3), np.uint8))
            eng.d2h(before[k], addrs[k])
        eng.cam_overlay_batch([(addrs[k], shapes[k], d_maps[k], map_shape) for k in range(3)], 0.5)
        eng.sync()
        for k, (h, w) in enumerate(shapes):
            after = np.empty((h, w, 3), np.uint8)
            eng.d2h(after, addrs[k])
            np.testing.assert_array_equal(after, cam.overlay_image(before[k], got[k], 0.5), err_msg=str((h, w)))
        with pytest.raises(ValueError):
            eng.occlusion_resident(items, [], 32, 33)
    finally:
        eng.close()


def test_classify_im_dir_draws_the_same_occlusion_maps_on_the_host_and_on_the_gpu(jpeg_dir, capsys):
    from roomnet_amd.infer import classify_im_dir
    from roomnet_amd.network import RoomNet
    nn = RoomNet(num_classes=6, im_side=224, compute_bn_mean_var=False, optimized_inference=True, max_batch=MAX_BATCH, dtype="bf16")
    nn.load(MODEL_PREFIX)
    out_dir = str(jpeg_dir) + "_classified"
    runs = {}
    capsys.readouterr()
    for arm, gpu, heat in (("host", False, "occlusion"), ("gpu", True, "occlusion"), ("plain", True, None)):
        kw = dict(occlusion_patch=64, occlusion_stride=48) if heat else {}
        xl = classify_im_dir(nn, str(jpeg_dir), overlay=True, batch_size=4, gpu_decode=gpu, gpu_encode=gpu, heatmap=heat, **kw)
        printed = capsys.readouterr().out
        if arm == "gpu":
            assert nn.last_decode_paths == {"jpeg": 3, "file": 0, "image": 0, "unreadable": 0}       # no host fallback
        files = {}
        for dirpath, _dirs, names in os.walk(out_dir):
            for name in names:
                p = os.path.join(dirpath, name)
                with open(p, "rb") as f:
                    files[os.path.relpath(p, out_dir)] = f.read()
                os.remove(p)
        with open(xl, "rb") as f:
            runs[arm] = (f.read(), printed, files)
        assert printed.count("--->") == 3 and len(files) == 3
    assert runs["host"][0] == runs["gpu"][0] == runs["plain"][0]                  # the workbook
    assert runs["host"][1] == runs["gpu"][1] == runs["plain"][1]
    assert sorted(runs["host"][2]) == sorted(runs["gpu"][2]) == sorted(runs["plain"][2])
    for name, data in runs["host"][2].items():
        assert runs["gpu"][2][name] == data, name
        assert runs["plain"][2][name] != data, name
    maps, drops, ids, probs = nn.occlusion_map(np.zeros((2, 224, 224, 3), np.uint8), patch=64, stride=48)
    assert maps.shape == (2, 224, 224) and drops.shape == (2, 5, 5) and ids.shape == (2,) and probs.shape == (2, 6)
    nn.sess.close()
