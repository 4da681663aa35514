"""The Huffman pass of the output JPEG on the GPU (csrc/rn_jpeg_huffenc.hip: rn_jpeg_huffenc_batch, rn_jpeg_encode_files_device)
and classify_im_dir's gpu_huffman_encode path.  The reference is the host pass, jpegenc.entropy_encode / encode_bgr, byte for
byte (and through it Pillow's files).

Tile sizes of the implementation (csrc/rn_jpeg_huffenc.h): the offsets scan works on tiles of 256 blocks, the stuffing on chunks
of 1024 unstuffed bytes, and one workgroup per image scans 256 tile sums (or chunk counts) per round.  240x320 has 1 800 blocks
(8 tiles); 480x640 noise at quality 100 has 7 200 blocks (29 tiles) and more than 256 KB of scan (more than 256 chunks: the
second round of the sums' scan, asserted below).  Both scans run the same sums kernel, so its carry is covered there."""
import os

import numpy as np
import pytest

pytest.importorskip("PIL")

import huffenc_cases as cases  # noqa: E402
from conftest import MODEL_PREFIX  # noqa: E402
from jpeg_cases import content, encode  # noqa: E402
from roomnet_amd import _capi, hershey, jpegdec, jpegenc  # noqa: E402
from roomnet_amd.graph import build_graph  # noqa: E402
from roomnet_amd.imageio import imwrite  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(16, 16), (8, 24), (37, 53), (17, 33), (1, 1), (31, 2), (50, 49), (72, 96), (120, 200), (240, 320)]      # tests/test_hip_jpegenc.py's
MAX_BATCH = 10
RN_E_INVALID, RN_E_RANGE = -1, -5
GUARD = 64


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
def host_files(images):
    """jpegenc.encode_bgr of each image; computed once."""
    return [jpegenc.encode_bgr(im) for im in images]


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
    """Images in device memory and a guarded output buffer each."""

    def __init__(self, engine, ims):
        self.engine, self.ims = engine, ims
        self.infos = [jpegenc.encode_info(im.shape[0], im.shape[1]) for im in ims]
        self.d = [engine.device_malloc(im.nbytes) for im in ims]
        self.caps = [jpegenc.encoded_bound(i) for i in self.infos]
        self.bufs = [np.full(c + GUARD, 0xA5, np.uint8) for c in self.caps]
        for d, im in zip(self.d, ims):
            engine.h2d(d, im)

    def items(self, overlays=None):
        return [(d, info, overlays[k] if overlays else [], None) for k, (d, info) in enumerate(zip(self.d, self.infos))]

    def encode(self, overlays=None, caps=None):
        lens, status = self.engine.jpeg_encode_files(self.items(overlays), self.bufs, self.caps if caps is None else caps)
        return lens, list(status)

    def files(self, lens):
        return [b[:n].tobytes() for b, n in zip(self.bufs, lens)]

    def guards_untouched(self, caps=None):
        return all((b[c:] == 0xA5).all() for b, c in zip(self.bufs, self.caps if caps is None else caps))

    def download(self):
        out = [np.empty(im.shape, np.uint8) for im in self.ims]
        for a, d in zip(out, self.d):
            self.engine.d2h(a, d)
        return out

    def close(self):
        for d in self.d:
            self.engine.device_free(d)


def test_mixed_batch_equals_the_host_pass_and_pillows_files(engine, images, host_files, tmp_path):
    up = Uploaded(engine, images)
    try:
        lens, status = up.encode()
        assert status == [0] * len(images)
        for k, (got, im) in enumerate(zip(up.files(lens), images)):
            assert got == host_files[k], SHAPES[k]
            p = str(tmp_path / "p.jpg")
            assert imwrite(p, im)
            with open(p, "rb") as f:
                assert got == f.read(), SHAPES[k]
        assert up.guards_untouched()
        for a, im in zip(up.download(), images):
            np.testing.assert_array_equal(a, im)              # (no overlay: the source is untouched)
        assert engine.jpeg_last_huffenc_ms() > 0
    finally:
        up.close()


def test_overlays_are_drawn_in_front_of_the_encode(engine, images):
    up = Uploaded(engine, images)
    try:
        both = [driver_overlays(im) for im in images]
        lens, status = up.encode([ovs for ovs, _l in both])
        assert status == [0] * len(images)
        for k, got in enumerate(up.files(lens)):
            assert got == jpegenc.encode_bgr(drawn_on_host(images[k], both[k][1])), SHAPES[k]
    finally:
        up.close()


def coefficient_batch(engine, batch, caps=None):
    bufs = [np.full((jpegenc.encoded_bound(info) if caps is None else caps[k]) + GUARD, 0xA5, np.uint8) for k, (_n, info, _c) in enumerate(batch)]
    announced = [b.size - GUARD for b in bufs]
    files, lens, status = engine.jpeg_huffenc_batch([(info, c) for _n, info, c in batch], bufs, announced)
    assert all((b[a:] == 0xA5).all() for b, a in zip(bufs, announced)), "stored past a buffer's cap"
    return files, lens, list(status)


def test_coefficient_patterns_pixels_cannot_produce(engine):
    refused = cases.refused()
    batch = cases.hand_built()[:3] + [refused[0]] + cases.hand_built()[3:] + [cases.stuffing()] + list(cases.padding_both_ends()) + [cases.flat_grey()]
    assert len(batch) == MAX_BATCH
    files, lens, status = coefficient_batch(engine, batch)
    for k, (name, info, c) in enumerate(batch):
        if k == 3:
            assert status[k] == jpegenc.ST_CATEGORY and files[k] is None, name
        else:
            assert status[k] == 0 and files[k] == jpegenc.entropy_encode(info, c), name
    # every refusal of the host pass, between two accepted images
    batch = [cases.hand_built()[0]] + refused + [cases.stuffing()]
    files, lens, status = coefficient_batch(engine, batch)
    assert status == [0] + [jpegenc.ST_CATEGORY] * len(refused) + [0]
    for k in (0, len(batch) - 1):
        assert files[k] == jpegenc.entropy_encode(batch[k][1], batch[k][2])


@pytest.fixture(scope="module")
def large_cases():
    out = []
    for h, w in ((240, 320), (480, 640)):
        info = jpegenc.encode_info(h, w, 100)
        c = jpegenc.coeffs_from_pixels(info, np.ascontiguousarray(content(h, w, "noise", seed=h)[:, :, ::-1]))
        out.append(("noise_%dx%d_q100" % (h, w), info, c, jpegenc.entropy_encode(info, c)))
    return out


def test_more_than_one_workgroup_in_both_scans(engine, large_cases):
    assert [jpegdec.coeff_count(info) // 64 for _n, info, _c, _r in large_cases] == [1800, 7200]
    assert len(large_cases[1][3]) > 256 * 1024 + 1024           # more than 256 chunks: a second round of the sums' scan
    files, lens, status = coefficient_batch(engine, [(n, info, c) for n, info, c, _r in large_cases])
    assert status == [0, 0]
    for got, (name, _info, _c, ref) in zip(files, large_cases):
        assert got == ref, name


def test_two_calls_back_to_back_and_a_repeated_call(engine, images, host_files, large_cases):
    first, second = Uploaded(engine, images[5:]), Uploaded(engine, images[:5])
    try:
        # other work of the handle in front, no sync anywhere: the second call's tables go into the other set, the zeroed
        # stream of the first call is not the second one's
        other = _capi.PinnedArray((jpegdec.coeff_count(first.infos[4]),), np.int16)
        engine.jpeg_encode_batch([(first.d[4], first.infos[4], [], other.array)])
        lens1, status1 = first.encode()
        lens2, status2 = second.encode()
        assert status1 == [0] * 5 and status2 == [0] * 5
        assert first.files(lens1) == host_files[5:] and second.files(lens2) == host_files[:5]
        big = [(n, info, c) for n, info, c, _r in large_cases[:1]]
        files, _lens, status = coefficient_batch(engine, big)      # a larger stream, then the small ones again: scratch zeroing
        assert status == [0] and files[0] == large_cases[0][3]
        again1, _s = first.encode()
        assert first.files(again1) == host_files[5:]
        files2, _lens, _status = coefficient_batch(engine, big)
        assert files2 == files                                    # a repeated call gives identical bytes
        other.close()
    finally:
        first.close()
        second.close()


def test_errors_enqueue_nothing_and_leave_the_handle_usable(engine, images, host_files):
    up = Uploaded(engine, images[:3])
    try:
        lens, status = up.encode()
        before = [b.copy() for b in up.bufs]
        lib, h = engine.lib, engine.handle
        ovs = [driver_overlays(im)[0] for im in images[:3]]
        big, _keep_big = engine._jpeg_sources(up.items() * 4)             # 12 entries
        ptrs, sizes, out_lens = engine._file_buffers(up.bufs * 4, up.caps * 4)
        st = np.zeros(12, np.int32)
        assert lib.rn_jpeg_encode_files_device(h, big, 0, ptrs, sizes, out_lens, st.ctypes.data) == RN_E_RANGE
        assert lib.rn_jpeg_encode_files_device(h, big, MAX_BATCH + 1, ptrs, sizes, out_lens, st.ctypes.data) == RN_E_RANGE

        def rc(change):
            arr, _keep = engine._jpeg_sources(up.items(ovs))
            change(arr)
            return lib.rn_jpeg_encode_files_device(h, arr, 3, ptrs, sizes, out_lens, st.ctypes.data)

        def unsupported(a):
            a[1].info.supported = 0

        def grid(a):
            a[1].info.blocks_w[0] += 1

        def no_image(a):
            a[0].d_bgr = None

        def box_right(a):
            a[0].overlays[1].x = a[0].info.width - a[0].overlays[1].w + 1

        for change in (unsupported, grid, no_image, box_right):
            assert rc(change) == RN_E_INVALID, change.__name__
        arr, _keep = engine._jpeg_sources(up.items(ovs))
        assert lib.rn_jpeg_encode_files_device(h, arr, 3, None, sizes, out_lens, st.ctypes.data) == RN_E_INVALID
        # the coefficient entry point
        infos = (_capi.rn_jpeg_info * 12)(*(up.infos * 4))
        coeffs = [np.zeros(jpegdec.coeff_count(i), np.int16) for i in up.infos]
        cptr = (_capi.C.c_void_p * 12)(*[c.ctypes.data for c in coeffs] * 4)
        fn = lib.rn_jpeg_huffenc_batch
        assert fn(h, infos, cptr, 0, ptrs, sizes, out_lens, st.ctypes.data) == RN_E_RANGE
        assert fn(h, infos, cptr, MAX_BATCH + 1, ptrs, sizes, out_lens, st.ctypes.data) == RN_E_RANGE
        infos[1].ncomp = 1
        assert fn(h, infos, cptr, 3, ptrs, sizes, out_lens, st.ctypes.data) == RN_E_INVALID
        infos[1].ncomp = 3
        cptr[2] = None
        assert fn(h, infos, cptr, 3, ptrs, sizes, out_lens, st.ctypes.data) == RN_E_INVALID
        engine.sync()
        for a, im in zip(up.download(), images[:3]):
            np.testing.assert_array_equal(a, im)              # nothing was drawn
        for b, want in zip(up.bufs, before):
            np.testing.assert_array_equal(b, want)            # earlier output is unchanged
        lens, status = up.encode(ovs)
        assert status == [0, 0, 0]
        for k, got in enumerate(up.files(lens)):
            assert got == jpegenc.encode_bgr(drawn_on_host(images[k], driver_overlays(images[k])[1])), SHAPES[k]
    finally:
        up.close()


def test_a_buffer_one_byte_short_is_status_cap_and_the_fallback_writes_the_same_bytes(engine, images):
    """What classify_files_to_dir does with a file whose status is not 0: the second pass draws no overlays."""
    ims = images[6:9]
    up = Uploaded(engine, ims)
    try:
        both = [driver_overlays(im) for im in ims]
        want = [jpegenc.encode_bgr(drawn_on_host(im, lines)) for im, (_o, lines) in zip(ims, both)]
        caps = [len(want[0]), len(want[1]) - 1, len(want[2])]
        lens, status = up.encode([ovs for ovs, _l in both], caps)
        assert status == [0, jpegenc.ST_CAP, 0] and lens == [len(w) for w in want]
        assert up.guards_untouched(caps)
        assert up.files(lens)[0] == want[0] and up.files(lens)[2] == want[2]
        coeffs = _capi.PinnedArray((jpegdec.coeff_count(up.infos[1]),), np.int16)
        try:
            engine.jpeg_encode_batch([(up.d[1], up.infos[1], [], coeffs.array)])
            engine.sync()
            assert jpegenc.entropy_encode(up.infos[1], coeffs.array.copy()) == want[1]
        finally:
            coeffs.close()
    finally:
        up.close()


def test_too_large_gets_no_launch_and_does_not_disturb_its_neighbour(engine):
    info = jpegenc.encode_info(16384, 16384, 95)
    name, small, c = cases.hand_built()[0]
    bufs = [np.full(1024, 0xA5, np.uint8), np.full(4096, 0xA5, np.uint8)]
    files, lens, status = engine.jpeg_huffenc_batch([(info, np.zeros(64, np.int16)), (small, c)], bufs)
    assert list(status) == [jpegenc.ST_TOO_LARGE, 0] and lens[0] == 0 and (bufs[0] == 0xA5).all()
    assert files[1] == jpegenc.entropy_encode(small, c)


def test_the_timer_before_any_batch_is_a_state_error(weights):
    e = _capi.Engine(build_graph(6, 224), weights, device=0, dtype="bf16", max_batch=1)
    try:
        with pytest.raises(Exception, match="no batch has been Huffman-encoded on this handle"):
            e.jpeg_last_huffenc_ms()
    finally:
        e.close()


def run_dir(nn, d, capsys, **kw):
    from roomnet_amd.infer import classify_im_dir
    out_dir = str(d) + "_classified"
    xl = classify_im_dir(nn, str(d), overlay=True, batch_size=4, gpu_decode=True, gpu_encode=True, **kw)
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


def test_classify_im_dir_writes_the_same_files_with_gpu_huffman_encode(tmp_path, capsys, monkeypatch):
    from PIL import Image
    from roomnet_amd import network
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
    capsys.readouterr()                   # (what loading the model printed)
    for heat in ({}, dict(heatmap="s6.bn")):
        base = run_dir(nn, d, capsys, **heat)
        mine = run_dir(nn, d, capsys, gpu_huffman_encode=True, **heat)
        assert base[1].count("unreadable image, skipped") == 1 and base[1].count("--->") == 9 and len(base[2]) == 8
        assert mine[1] == base[1] and mine[0] == base[0]
        assert sorted(mine[2]) == sorted(base[2])
        for name, data in base[2].items():
            assert mine[2][name] == data, name
        assert nn.huffenc_fallbacks == 0
    with pytest.raises(ValueError, match="gpu_huffman_encode"):
        classify_im_dir(nn, str(d), overlay=True, gpu_decode=True, gpu_encode=False, gpu_huffman_encode=True)

    def same_files(mine):
        assert mine[1] == base[1] and mine[0] == base[0] and sorted(mine[2]) == sorted(base[2])
        for name, data in base[2].items():
            assert mine[2][name] == data, name

    # The driver's own fallback.  Slots of 50 000 bytes hold the smooth files (at most 44 KB) and not the noise ones (59 KB and
    # more): files of both kinds in one chunk, ST_CAP for the second kind, the second pass without overlays.
    base = run_dir(nn, d, capsys)
    with monkeypatch.context() as m:
        m.setattr(network, "_huffenc_slot_bytes", lambda info: 50000)
        nn._jpeg_out_ring.close()                         # (the ring keeps a slot's buffer while it is large enough)
        nn._jpeg_out_ring = None
        same_files(run_dir(nn, d, capsys, gpu_huffman_encode=True))
        assert 0 < nn.huffenc_fallbacks < 8
    # An image the call enqueued nothing for (what ST_TOO_LARGE means; a real one has more than 2 590 450 blocks): the call is
    # made without the chunk's first image and reports that status for it, so nothing drew its overlays and the second pass must.
    eng = nn._engine()
    real = eng.jpeg_encode_files

    def without_the_first(items, bufs, caps=None):
        lens, status = real(items[1:], bufs[1:]) if len(items) > 1 else ([], np.zeros(0, np.int32))
        return [0] + lens, np.concatenate([[jpegenc.ST_TOO_LARGE], status]).astype(np.int32)

    with monkeypatch.context() as m:
        m.setattr(eng, "jpeg_encode_files", without_the_first)
        same_files(run_dir(nn, d, capsys, gpu_huffman_encode=True))
        assert nn.huffenc_fallbacks >= 2                  # (one per chunk that went through the device)
    nn.sess.close()
