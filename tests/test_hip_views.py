"""The training views on the GPU (rn_views_*, csrc/rn_imageops.hip) byte for byte against the host restatement
(``finetune.make_view`` of ``finetune.view_draw``): every resize mode, both axes, every flag combination, repeated items, and
launches back to back."""
import ctypes as C

import numpy as np
import pytest

from roomnet_amd import _capi, finetune
from roomnet_amd.graph import build_graph

pytestmark = pytest.mark.gpu

S = 224
# (height, width): copy mode, box mode, both axes, range 1, the upscale of a tiny image, one full-size photograph
SHAPES = ((224, 224), (448, 448), (300, 224), (224, 300), (225, 224), (5, 7), (1080, 1920))
SEED = (1 << 40) + 2024
STEPS = (0, 1, 2, 3, 4, 2 ** 32 + 5)


@pytest.fixture(scope="module")
def photographs():
    rng = np.random.default_rng(31)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in SHAPES]


@pytest.fixture(scope="module")
def engine(weights):
    eng = _capi.Engine(build_graph(6, S), weights, device=0, dtype="bf16", max_batch=8)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def views(engine, photographs):
    v = engine.views_create(photographs)
    yield v
    v.close()


def host_views(photographs, index, step, crop, flip, seed=SEED):
    return np.stack([finetune.make_view(photographs[i], finetune.view_draw(seed, step, b, *photographs[i].shape[:2], crop=crop, flip=flip), S)
                     for b, i in enumerate(index)], 0)


def test_the_cases_cover_every_flip_and_three_offsets(photographs):
    """What the comparisons below rest on: these steps and this seed draw all four flip combinations, and at least three distinct
    offsets for each of the two 300-pixel photographs."""
    draws = [[finetune.view_draw(SEED, step, b, *im.shape[:2]) for b, im in enumerate(photographs)] for step in STEPS]
    assert {(d["fliplr"], d["flipud"]) for row in draws for d in row} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert len({row[2]["y0"] for row in draws}) >= 3 and all(row[2]["x0"] == 0 for row in draws)
    assert len({row[3]["x0"] for row in draws}) >= 3 and all(row[3]["y0"] == 0 for row in draws)
    assert len({row[6]["x0"] for row in draws}) >= 3


@pytest.mark.parametrize("crop,flip", [(True, True), (True, False), (False, True)])
def test_views_are_the_host_restatement(engine, views, photographs, crop, flip):
    index = np.arange(len(SHAPES), dtype=np.int32)
    seen = set()
    for step in STEPS:
        got = engine.views_batch(views, index, step, seed=SEED, crop=crop, flip=flip)
        want = host_views(photographs, index, step, crop, flip)
        assert got.shape == want.shape == (len(SHAPES), S, S, 3)
        for b in index:
            d = finetune.view_draw(SEED, step, b, *SHAPES[b], crop=crop, flip=flip)
            seen.add((d["fliplr"], d["flipud"]))
            np.testing.assert_array_equal(got[b], want[b], err_msg="step %d, slot %d %s, draw %s" % (step, b, SHAPES[b], d))
    assert seen == ({(0, 0), (0, 1), (1, 0), (1, 1)} if flip else {(0, 0)})


def test_no_flags_is_the_centre_crop_resize(engine, views, photographs):
    index = np.arange(len(SHAPES), dtype=np.int32)
    want = engine.crop_resize_batch(photographs)
    for step in (0, 3):
        got = engine.views_batch(views, index, step, seed=SEED, crop=False, flip=False)
        np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(want, host_views(photographs, index, 0, False, False))


def test_a_repeated_item_gets_a_draw_per_slot(engine, views, photographs):
    index = np.array([3, 2, 3, 6, 6, 0, 3, 2], np.int32)
    step = next(s for s in range(64) if len({tuple(finetune.view_draw(SEED, s, b, 224, 300).values()) for b in (0, 2, 6)}) == 3
                and finetune.view_draw(SEED, s, 1, 300, 224) != finetune.view_draw(SEED, s, 7, 300, 224))
    got = engine.views_batch(views, index, step, seed=SEED)
    np.testing.assert_array_equal(got, host_views(photographs, index, step, True, True))
    assert not np.array_equal(got[0], got[2]) and not np.array_equal(got[1], got[7])


def test_back_to_back_launches_without_a_sync(engine, views, photographs):
    """Two launches of different steps, seeds and indices into two destinations with no synchronisation in between: the launch
    carries its arguments, there is no table to overwrite."""
    calls = [(np.array([6, 1, 2, 3, 4, 5, 0, 2], np.int32), 7, SEED), (np.array([2, 3, 6], np.int32), 2 ** 32 + 1, 99)]
    d_idx = [engine.device_malloc(idx.nbytes) for idx, _, _ in calls]
    d_dst = [engine.device_malloc(idx.size * S * S * 3) for idx, _, _ in calls]
    try:
        for d, (idx, _, _) in zip(d_idx, calls):
            engine.h2d(d, idx)
        engine.sync()
        for _ in range(2):
            for di, dd, (idx, step, seed) in zip(d_idx, d_dst, calls):
                _capi._check(engine.lib, engine.lib.rn_views_batch_device(engine.handle, views.handle, C.c_void_p(di), 0, idx.size, seed, step,
                                                                          3, C.c_void_p(dd)), "rn_views_batch_device")
        engine.sync()
        for dd, (idx, step, seed) in zip(d_dst, calls):
            got = np.empty((idx.size, S, S, 3), np.uint8)
            engine.d2h(got, dd)
            np.testing.assert_array_equal(got, host_views(photographs, idx, step, True, True, seed=seed))
        # a base into a longer index: slots [3, 6) of the first call's index
        idx, step, seed = calls[0]
        _capi._check(engine.lib, engine.lib.rn_views_batch_device(engine.handle, views.handle, C.c_void_p(d_idx[0]), 3, 3, seed, step, 3,
                                                                  C.c_void_p(d_dst[0])), "rn_views_batch_device")
        engine.sync()
        got = np.empty((3, S, S, 3), np.uint8)
        engine.d2h(got, d_dst[0])
        np.testing.assert_array_equal(got, host_views(photographs, idx[3:6], step, True, True, seed=seed))
    finally:
        for d in d_idx + d_dst:
            engine.device_free(d)


def test_refusals(engine, views):
    lib, h, v = engine.lib, engine.handle, views.handle
    d = engine.device_malloc(8 * S * S * 3)
    try:
        engine.h2d(d, np.zeros(8, np.int32))
        engine.sync()
        call = lib.rn_views_batch_device
        assert call(h, v, None, 0, 1, 0, 0, 3, C.c_void_p(d)) == -1
        assert call(h, v, C.c_void_p(d), 0, 1, 0, 0, 3, None) == -1
        assert call(h, None, C.c_void_p(d), 0, 1, 0, 0, 3, C.c_void_p(d)) == -1
        assert call(None, v, C.c_void_p(d), 0, 1, 0, 0, 3, C.c_void_p(d)) == -1
        assert call(h, v, C.c_void_p(d), 0, 1, 0, 0, 4, C.c_void_p(d)) == -1
        assert call(h, v, C.c_void_p(d), 0, 0, 0, 0, 3, C.c_void_p(d)) == -5
        assert call(h, v, C.c_void_p(d), 0, 9, 0, 0, 3, C.c_void_p(d)) == -5
        assert call(h, v, C.c_void_p(d), 0, 1, 0, -1, 3, C.c_void_p(d)) == -5
        assert call(h, v, C.c_void_p(d), -1, 1, 0, 0, 3, C.c_void_p(d)) == -5
        out = C.c_void_p()
        good = _capi.rn_view_source(d, 4, 4)
        assert lib.rn_views_create(h, None, 1, C.byref(out)) == -1
        assert lib.rn_views_create(h, C.byref(good), 0, C.byref(out)) == -1
        assert lib.rn_views_create(h, C.byref(good), 1, None) == -1
        for bad in (_capi.rn_view_source(None, 4, 4), _capi.rn_view_source(d, 0, 4), _capi.rn_view_source(d, 4, 0)):
            assert lib.rn_views_create(h, C.byref(bad), 1, C.byref(out)) == -1 and not out.value
        with pytest.raises(ValueError):
            engine.views_create([np.zeros((0, 4, 3), np.uint8)])
        with pytest.raises(ValueError):
            engine.views_batch(views, [len(SHAPES)], 0)
    finally:
        engine.device_free(d)
