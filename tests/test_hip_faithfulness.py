"""Deletion and insertion curves of a heat map on the GPU (csrc/rn_faith.hip: rn_faith_*), RoomNet.map_faithfulness and
infer.compare_heatmaps.  The reference is roomnet_amd/faithfulness.py with the handle's own forward pass on the same chunks: ranks,
mask bytes, curves and areas are compared for equality, no comparison here takes a tolerance."""
import ctypes as C
import os

import numpy as np
import pytest

import checkpoints as CK
from conftest import MODEL_PREFIX, parity_set_of
from roomnet_amd import _capi, cam, faithfulness as F, occlusion as O
from roomnet_amd.graph import build_graph

pytestmark = pytest.mark.gpu

MAX_BATCH = 32
RN_E_INVALID, RN_E_RANGE = -1, -5
PICK = [14, 41, 52]                      # a seeded textured image and two of the class-covering field images of the parity set
J = 5                                    # with both modes 12 passes per image: 36 for 3 images, chunks of 32 / 4


@pytest.fixture(scope="module")
def ims(parity_images):
    return np.ascontiguousarray(parity_images[PICK])


@pytest.fixture(scope="module")
def engines(weights):
    """Engines by name: "bf16" / "f32" at 224 on the shipped checkpoint, "185" on the seeded live checkpoint (bf16)."""
    made = {}

    def get(name):
        if name not in made:
            if name == "185":
                g = build_graph(6, 185)
                made[name] = _capi.Engine(g, CK.live(g, 0, CK.LIVE_GAIN), device=0, dtype="bf16", max_batch=MAX_BATCH)
            else:
                made[name] = _capi.Engine(build_graph(6, 224), weights, device=0, dtype=name, max_batch=MAX_BATCH)
        return made[name]

    yield get
    for e in made.values():
        e.close()


@pytest.fixture(scope="module")
def ims185():
    return np.ascontiguousarray(parity_set_of(185)[[17, 45, 3]])


def special_map(side, seed):
    """+-0, +-inf, NaNs of both signs and denormals among ordinary values."""
    rng = np.random.default_rng(seed)
    npix = side * side
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, 1e-45, -1e-45], np.float32)
    m = np.where(rng.random(npix) < 0.6, special[rng.integers(0, len(special), npix)], rng.normal(0, 1, npix).astype(np.float32)).astype(np.float32)
    neg_nan = np.isnan(m) & (rng.random(npix) < 0.5)
    m.view(np.uint32)[neg_nan] = 0xFFC00001
    return m.reshape(side, side)


def three_maps(eng, batch, patch, stride):
    """An occlusion map from a 5 x 5 grid (piecewise constant: heavy ties), an upsampled ReLU'd coarse map (one large zero
    plateau) and a map strewn with +-0, +-inf and NaN."""
    side = batch.shape[1]
    assert O.grid(side, patch, stride) == 5
    if side == 224:
        occ = eng.occlusion_u8(batch[:1], patch=patch, stride=stride)[0][0]
    else:                     # (the same piecewise-constant form from seeded drops: no forward pass is needed for it)
        occ = O.pixel_map(np.random.default_rng(7).normal(0, 0.1, (5, 5)).astype(np.float32), side, patch, stride)
    assert len(np.unique(occ)) <= 81                      # at most 9 x 9 cells of constant value
    coarse = cam.upsample(np.random.default_rng(side).normal(-0.5, 1, (46, 46)), side)
    assert (coarse == 0).mean() > 0.3
    return np.ascontiguousarray(np.stack([occ, coarse, special_map(side, side)]), dtype=np.float32)


@pytest.fixture(scope="module")
def maps(engines, ims):
    return three_maps(engines("bf16"), ims, 64, 48)


@pytest.fixture(scope="module")
def maps185(engines, ims185):
    return three_maps(engines("185"), ims185, 61, 31)


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


def ranks_of(eng, m):
    dev = Dev(eng)
    try:
        d_rank = dev.room(m.size * 4)
        eng.faith_ranks_device(dev.put(m), len(m), d_rank)
        eng.sync()
        return dev.get(d_rank, m.shape, np.uint32)
    finally:
        dev.close()


def masks_of(eng, batch, m, steps, modes, fill, first, count):
    dev = Dev(eng)
    try:
        s = batch.shape[1]
        d_out = dev.room(count * s * s * 3)
        eng.faith_masks_device(dev.put(batch), dev.put(m), len(batch), steps, modes, fill, first, count, d_out)
        eng.sync()
        return dev.get(d_out, (count, s, s, 3), np.uint8)
    finally:
        dev.close()


class Call:
    """One rn_faith_u8_device call in three steps, so that several calls can be enqueued with nothing between them: the constructor
    allocates and uploads (Engine.h2d waits for the handle's stream), ``enqueue`` only enqueues, ``read`` syncs."""

    def __init__(self, eng, dev, batch, m, class_ids, steps, modes, fill):
        self.eng, self.dev, self.steps, self.modes, self.fill = eng, dev, steps, modes, fill
        self.n, self.nc, self.m_curves = len(batch), eng.graph.num_classes, len(F.mode_slots(modes))
        self.d_cls = dev.put(np.asarray(class_ids, np.int32)) if class_ids is not None else None
        self.d_curve, self.d_auc = dev.room(self.n * self.m_curves * (steps + 1) * 4), dev.room(self.n * self.m_curves * 4)
        self.d_probs, self.d_ids = dev.room(self.n * self.nc * 4), dev.room(self.n * 8)
        self.d_bgr, self.d_map = dev.put(batch), dev.put(m)

    def enqueue(self):
        self.eng.faith_u8_device(self.d_bgr, self.d_map, self.n, self.d_cls, self.steps, self.modes, self.fill, self.d_curve, self.d_auc,
                                 self.d_probs, self.d_ids)

    def read(self):
        self.eng.sync()
        n, get = self.n, self.dev.get
        return (get(self.d_curve, (n, self.m_curves, self.steps + 1), np.float32), get(self.d_auc, (n, self.m_curves), np.float32),
                get(self.d_ids, (n,), np.int64), get(self.d_probs, (n, self.nc), np.float32))


def device_call(eng, batch, m, class_ids, steps, modes, fill):
    dev = Dev(eng)
    try:
        call = Call(eng, dev, batch, m, class_ids, steps, modes, fill)
        call.enqueue()
        return call.read()
    finally:
        dev.close()


def host_call(eng, batch, m, class_ids, steps, modes, fill):
    """The NumPy statement over rn_forward_u8 of the same handle: the same chunk sizes, so the same launches."""
    return F.curves_host(lambda b: eng.forward_u8(b)[1], batch, m, class_ids=class_ids, steps=steps, modes=modes, fill=fill,
                         max_batch=eng.max_batch)


def assert_same(got, want, what="", names=("curve", "auc", "ids", "probs")):
    for name, a, b in zip(names, got, want):
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name, a.dtype, b.dtype, a.shape, b.shape)
        if not np.array_equal(a, b):
            at = np.argwhere(a != b)
            raise AssertionError("%s %s: %d of %d entries differ, first at %s: %r != %r" % (what, name, len(at), a.size, at[0].tolist(),
                                                                                             a[tuple(at[0])], b[tuple(at[0])]))


# ------------------------------------------------------------------------------------------------ 1. ranks
@pytest.mark.parametrize("which", ["224", "185"])
def test_ranks_equal_the_stable_argsort(engines, maps, maps185, which):
    """185 x 185 = 34 225 pixels = 49 mod 64: the tail tile; 224 x 224 = 784 whole tiles, 49 per wave."""
    eng, m = (engines("bf16"), maps) if which == "224" else (engines("185"), maps185)
    side = m.shape[1]
    got = ranks_of(eng, m)
    print("%s: the rank launch of 3 maps took %.3f ms" % (which, eng.faith_last_ms()))
    for k in range(3):
        assert np.array_equal(got[k], F.ranks(m[k])), k
        assert np.array_equal(np.sort(got[k].ravel()), np.arange(side * side, dtype=np.uint32)), k
    assert np.array_equal(ranks_of(eng, m), got)                                   # the same map, the same ranks
    flat = np.stack([np.full((side, side), -2.5, np.float32), np.arange(side * side, dtype=np.float32).reshape(side, side)])
    got = ranks_of(eng, flat)
    assert np.array_equal(got[0].ravel(), np.arange(side * side))                   # all equal: the raster index
    assert np.array_equal(got[1].ravel(), np.arange(side * side)[::-1])             # a strictly increasing ramp: reversed
    assert np.array_equal(ranks_of(eng, m[2:])[0], F.ranks(m[2]))                   # one image alone


# ------------------------------------------------------------------------------------------------ 2. mask bytes
@pytest.mark.parametrize("fill", ["mean", (7, 200, 31)])
@pytest.mark.parametrize("which", ["224", "185"])
def test_mask_bytes_across_a_curve_and_an_image_boundary(engines, ims, maps, ims185, maps185, which, fill):
    """36 passes for 3 images with J = 5 and both modes, 12 per image: deletion 0 .. 5, then insertion 0 .. 5.  [0, 32) holds images 0
    and 1 and image 2 up to the second point of its insertion curve: it crosses curve and image boundaries; [30, 36) is the end of
    the call, the range of the second chunk and two passes more; [10, 14) crosses from image 0 to image 1 alone.  n_1 = 10 035 at 224
    is no multiple of 4: a mask edge inside a dword.  185 takes the byte path."""
    eng, batch, m = (engines("bf16"), ims, maps) if which == "224" else (engines("185"), ims185, maps185)
    assert eng.faith_plan(3, J, 3) == (36, 2)
    rank_maps = [F.ranks(x) for x in m]
    fills = [O._fill_of(im, fill) for im in batch]
    want = np.stack([F.masked_pass(batch, rank_maps, fills, f, J, 3) for f in range(36)])
    n1 = F.step_counts(batch.shape[1], J)[1]
    assert np.array_equal(want[1], F.deleted(batch[0], rank_maps[0], n1, fill))
    assert np.array_equal(want[12 + 6 + 4], F.inserted(batch[1], rank_maps[1], F.step_counts(batch.shape[1], J)[4], fill))
    assert np.array_equal(want[0], batch[0]) and np.array_equal(want[11], batch[0])             # n_0 deleted, n_J inserted: the image
    assert (want[5] == fills[0]).all() and (want[6] == fills[0]).all()                          # n_J deleted, n_0 inserted: the fill
    for first, count in ((0, 32), (30, 6), (10, 4), (35, 1)):
        got = masks_of(eng, batch, m, J, 3, fill, first, count)
        np.testing.assert_array_equal(got, want[first:first + count], err_msg=str((first, count)))
    # one mode alone: insertion is slot 0 then
    got = masks_of(eng, batch, m, J, "insertion", fill, 4, 10)
    np.testing.assert_array_equal(got, np.stack([F.masked_pass(batch, rank_maps, fills, f, J, 2) for f in range(4, 14)]))
    np.testing.assert_array_equal(got[:2], want[[6 + 4, 6 + 5]])


# ------------------------------------------------------------------------------------------------ 3. curves and areas
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_curves_and_areas_equal_the_host_statement_over_the_same_forward(engines, ims, maps, dtype):
    eng = engines(dtype)
    ids_f, probs_f = eng.forward_u8(ims)
    got = device_call(eng, ims, maps, None, J, 3, "mean")
    assert np.array_equal(got[2], ids_f) and np.array_equal(got[3], probs_f)
    want = host_call(eng, ims, maps, None, J, 3, "mean")
    print("%s: curves of image 0\n%s\nareas\n%s\n%.3f ms on the device" % (dtype, got[0][0], got[1], eng.faith_last_ms()))
    assert_same(got, want, dtype)
    assert np.isfinite(got[0]).all() and (got[0].max(-1) > got[0].min(-1)).all()
    # the blocking host form returns the same
    assert_same(eng.faith_u8(ims, maps, steps=J), want, dtype + " rn_faith_u8")
    # given classes that are not the argmax
    other = ((ids_f + 1) % 6).astype(np.int32)
    cls = np.array([ids_f[0], other[1], other[2]], np.int32)
    given = device_call(eng, ims, maps, cls, J, 3, (0, 0, 0))
    assert_same(given, host_call(eng, ims, maps, cls, J, 3, (0, 0, 0)), dtype + " given classes")
    assert np.array_equal(given[2], ids_f) and np.array_equal(given[3], probs_f)
    assert_same(eng.faith_u8(ims, maps, class_ids=cls, steps=J, fill=(0, 0, 0)), given, dtype + " rn_faith_u8, given classes")
    # one mode alone (18 passes: one chunk), another step count
    for modes in (1, 2):
        one = device_call(eng, ims, maps, None, 4, modes, "mean")
        assert one[0].shape == (3, 1, 5) and one[1].shape == (3, 1)
        assert_same(one, host_call(eng, ims, maps, None, 4, modes, "mean"), "%s modes = %d" % (dtype, modes))


# ------------------------------------------------------------------------------------------------ 4. back to back
def test_calls_back_to_back_share_the_masked_chunk_with_occlusion(engines, ims, maps):
    """Two faithfulness calls with different (J, modes, fill) and an occlusion call between them on the same handle, enqueued with
    NO sync between them: every buffer is allocated and uploaded first (an upload waits for the stream), no class ids are given
    (the library reads those back, which waits too).  They share the handle's masked chunk, its probabilities and the per-image
    fills; the occlusion call's mean fills of OTHER images must not reach either neighbour's masks."""
    eng = engines("bf16")
    rev = np.ascontiguousarray(ims[::-1])
    dev = Dev(eng)
    try:
        first = Call(eng, dev, ims, maps, None, J, 3, "mean")
        third = Call(eng, dev, ims[:2], maps[1:], None, 7, 2, (255, 255, 255))
        nc, g = eng.graph.num_classes, O.grid(224, 64, 48)
        d_bgr, d_drop, d_map = dev.put(rev), dev.room(3 * g * g * 4), dev.room(3 * 224 * 224 * 4)
        d_probs, d_ids = dev.room(3 * nc * 4), dev.room(3 * 8)
        eng.sync()
        first.enqueue()
        eng.occlusion_u8_device(d_bgr, 3, None, 64, 48, "mean", d_drop, d_map, d_probs, d_ids)
        third.enqueue()
        got_first, got_third = first.read(), third.read()
        got_occ = (dev.get(d_map, (3, 224, 224), np.float32), dev.get(d_drop, (3, g, g), np.float32), dev.get(d_ids, (3,), np.int64),
                   dev.get(d_probs, (3, nc), np.float32))
    finally:
        dev.close()
    assert_same(got_first, host_call(eng, ims, maps, None, J, 3, "mean"), "call 1 of 3 back to back")
    want_occ = O.occlusion_map_host(lambda b: eng.forward_u8(b)[1], rev, patch=64, stride=48, fill="mean", max_batch=eng.max_batch)
    assert_same(got_occ, want_occ, "call 2 of 3 back to back (occlusion)", ("map", "drop", "ids", "probs"))
    assert_same(got_third, host_call(eng, ims[:2], maps[1:], None, 7, 2, (255, 255, 255)), "call 3 of 3 back to back")


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals_enqueue_nothing_and_leave_the_handle_usable(engines, ims, maps, golden_parity):
    eng = engines("bf16")
    lib, h = eng.lib, eng.handle
    ids_f, probs_f = eng.forward_u8(ims)
    assert np.array_equal(ids_f, golden_parity["ids"][PICK])
    dev = Dev(eng)
    try:
        d_bgr, d_map = dev.put(ims), dev.put(maps)
        d_bad = dev.put(np.array([0, 6, 1], np.int32))
        d_neg = dev.put(np.array([0, 1, -1], np.int32))
        sizes = {"curve": 36, "auc": 6, "probs": 18, "ids": 6, "rank": 64, "out": 64}          # in dwords (the last two: their heads)
        bufs = {"curve": dev.room(36 * 4), "auc": dev.room(6 * 4), "probs": dev.room(18 * 4), "ids": dev.room(3 * 8),
                "rank": dev.room(3 * 224 * 224 * 4), "out": dev.room(MAX_BATCH * 224 * 224 * 3)}
        for name, b in bufs.items():
            eng.h2d(b, np.full(sizes[name], 0x5A5A5A5A, np.uint32))
        v = C.c_void_p

        def full(n=3, cls=None, steps=J, modes=3, bgr=d_bgr, m=d_map, curve=bufs["curve"], auc=bufs["auc"], probs=bufs["probs"],
                 ids=bufs["ids"], handle=h):
            opt = lambda p: v(p) if p else None       # noqa: E731
            return lib.rn_faith_u8_device(handle, opt(bgr), opt(m), n, opt(cls), steps, modes, None, opt(curve), opt(auc), opt(probs), opt(ids))

        def masks(n=3, steps=J, modes=3, first=0, count=32, m=d_map):
            return lib.rn_faith_masks_device(h, v(d_bgr), v(m) if m else None, n, steps, modes, None, first, count, v(bufs["out"]))

        def rank_call(n=3, m=d_map, rank=bufs["rank"]):
            return lib.rn_faith_ranks_device(h, v(m) if m else None, n, v(rank) if rank else None)

        def untouched_and_usable(what):
            eng.sync()
            for name, b in bufs.items():
                assert (dev.get(b, (sizes[name],), np.uint32) == 0x5A5A5A5A).all(), (what, name)
            # (the golden file holds the float64 reference, not this handle's bf16 bits: the ids were compared with it above, the
            #  probabilities are compared with the same handle's own result from before the first refusal)
            ids, probs = eng.forward_u8(ims)
            assert np.array_equal(ids, ids_f) and np.array_equal(probs, probs_f), what

        for what, call, rc in [("J = 0", lambda: full(steps=0), RN_E_INVALID),
                               ("J = -1", lambda: full(steps=-1), RN_E_INVALID),
                               ("J > S^2", lambda: full(steps=224 * 224 + 1), RN_E_INVALID),
                               ("modes = 0", lambda: full(modes=0), RN_E_INVALID),
                               ("modes = 4", lambda: full(modes=4), RN_E_INVALID),
                               ("n = 0", lambda: full(n=0), RN_E_INVALID),
                               ("n = -2", lambda: full(n=-2), RN_E_INVALID),
                               ("null image", lambda: full(bgr=None), RN_E_INVALID),
                               ("null map", lambda: full(m=None), RN_E_INVALID),
                               ("null curve", lambda: full(curve=None), RN_E_INVALID),
                               ("null auc", lambda: full(auc=None), RN_E_INVALID),
                               ("null probs", lambda: full(probs=None), RN_E_INVALID),
                               ("null ids", lambda: full(ids=None), RN_E_INVALID),
                               ("null handle", lambda: full(handle=None), RN_E_INVALID),
                               ("class id 6", lambda: full(cls=d_bad), RN_E_INVALID),
                               ("class id -1", lambda: full(cls=d_neg), RN_E_INVALID),
                               ("n > max_batch", lambda: full(n=MAX_BATCH + 1), RN_E_RANGE),
                               ("more than 2^20 passes", lambda: full(n=MAX_BATCH, steps=16384), RN_E_RANGE),
                               ("masks: J = 0", lambda: masks(steps=0), RN_E_INVALID),
                               ("masks: modes = 4", lambda: masks(modes=4), RN_E_INVALID),
                               ("masks: n = 0", lambda: masks(n=0), RN_E_INVALID),
                               ("masks: null map", lambda: masks(m=None), RN_E_INVALID),
                               ("masks: n > max_batch", lambda: masks(n=MAX_BATCH + 1), RN_E_RANGE),
                               ("masks: count > max_batch", lambda: masks(count=MAX_BATCH + 1), RN_E_RANGE),
                               ("masks: count = 0", lambda: masks(count=0), RN_E_RANGE),
                               ("masks: past the end", lambda: masks(first=30, count=7), RN_E_RANGE),
                               ("masks: first < 0", lambda: masks(first=-1, count=4), RN_E_RANGE),
                               ("ranks: n = 0", lambda: rank_call(n=0), RN_E_INVALID),
                               ("ranks: null map", lambda: rank_call(m=None), RN_E_INVALID),
                               ("ranks: null ranks", lambda: rank_call(rank=None), RN_E_INVALID),
                               ("ranks: n > max_batch", lambda: rank_call(n=MAX_BATCH + 1), RN_E_RANGE)]:
            assert call() == rc, what
            assert b"rn_faith" in lib.rn_last_error(), what
            untouched_and_usable(what)
        ms = C.c_float(0)
        assert lib.rn_faith_last_ms(h, None) == RN_E_INVALID and lib.rn_faith_last_ms(None, C.byref(ms)) == RN_E_INVALID
        with pytest.raises(ValueError):
            eng.faith_u8(ims, maps, steps=0)
        with pytest.raises(ValueError):
            eng.faith_u8(ims, maps, class_ids=[0, 1, 6], steps=J)
        with pytest.raises(ValueError):
            eng.faith_u8(ims, maps, steps=J, fill="median")
        with pytest.raises(ValueError):
            eng.faith_u8(ims, maps, steps=J, modes=("removal",))
        with pytest.raises(ValueError):
            eng.faith_u8(ims, maps[:2], steps=J)
        untouched_and_usable("the Python refusals")
        # ... and the same buffers take a good call
        assert full() == 0
        eng.sync()
        assert np.array_equal(dev.get(bufs["probs"], (3, 6), np.float32), probs_f)
        assert_same((dev.get(bufs["curve"], (3, 2, J + 1), np.float32), dev.get(bufs["auc"], (3, 2), np.float32)),
                    host_call(eng, ims, maps, None, J, 3, "mean")[:2], "after the refusals")
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------------ 6. the Python surface
def test_map_faithfulness_and_compare_heatmaps(tmp_path, capsys):
    pytest.importorskip("PIL")
    from jpeg_cases import content, encode
    from roomnet_amd.infer import compare_heatmaps
    from roomnet_amd.network import RoomNet
    nn = RoomNet(num_classes=6, im_side=224, compute_bn_mean_var=False, optimized_inference=True, max_batch=MAX_BATCH, dtype="bf16")
    nn.load(MODEL_PREFIX)
    try:
        batch = np.ascontiguousarray(parity_set_of(224)[[14, 52]])
        coarse = np.random.default_rng(2).normal(0, 1, (2, 46, 46)).astype(np.float32)
        curves, aucs, ids, probs = nn.map_faithfulness(batch, coarse, steps=6)
        assert curves.shape == (2, 2, 7) and aucs.shape == (2, 2) and ids.shape == (2,) and probs.shape == (2, 6)
        assert curves.dtype == np.float32 and aucs.dtype == np.float32 and ids.dtype == np.int64
        assert np.array_equal(aucs, F.auc(curves)) and np.isfinite(curves).all()
        eng = nn._engine()
        assert_same((curves, aucs, ids, probs), eng.faith_u8(batch, cam.upsample(coarse, 224), steps=6), "map_faithfulness")
        only = nn.map_faithfulness(batch[0], coarse[0], class_ids=[3], steps=3, modes="insertion", fill=(0, 0, 0))
        assert only[0].shape == (1, 1, 4) and only[1].shape == (1, 1)
        with pytest.raises(ValueError):
            nn.map_faithfulness(batch, coarse[:1])
        d = tmp_path / "images"
        os.makedirs(str(d))
        for k, (hh, ww) in enumerate([(150, 200), (201, 150), (224, 224)]):          # a landscape, a portrait and a square file
            encode(str(d / ("f%d.jpg" % k)), content(hh, ww, ["smooth", "noise"][k % 2], seed=k), [2, 1, 0][k], quality=90)
        capsys.readouterr()
        report = compare_heatmaps(nn, str(d), steps=8, batch_size=4, patch=64, stride=48)
        printed = capsys.readouterr().out
        assert sorted(report) == ["occlusion", "s6.bn", "s7.bn"]
        for method, row in report.items():
            assert row["images"] == 3 and np.isfinite(row["deletion"]) and np.isfinite(row["insertion"]), method
            assert 0.0 <= row["deletion"] <= 1.0 and 0.0 <= row["insertion"] <= 1.0, method
            assert method in printed
        with pytest.raises(ValueError):
            compare_heatmaps(nn, str(d), methods=("s5.bn",))
    finally:
        nn.sess.close()
