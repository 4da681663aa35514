"""The training views' draw on the host (include/roomnet_hip.h: fine-tuning on fresh random views): ``rn_view_draw`` against
``finetune.view_draw``, the flags, the host restatement ``finetune.make_view``, and the distribution at a fixed seed.  No GPU."""
import ctypes as C
import itertools

import numpy as np
import pytest

from roomnet_amd import _capi, finetune
from roomnet_amd.graph import build_graph
from roomnet_amd.imageops import resize_linear_u8
from roomnet_amd.network import RoomNet

SEEDS = (0, 7, (1 << 40) + 12345, (1 << 64) - 1)
STEPS = (0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1)
SLOTS = (0, 44)
# (height, width): range 0, 1, 7 and 840 along both axes
SIZES = ((224, 224), (224, 225), (225, 224), (300, 307), (307, 300), (1080, 1920), (1920, 1080))


def c_draw(seed, step, slot, height, width, crop=True, flip=True):
    v = _capi.rn_view()
    rc = _capi.load_library().rn_view_draw(seed, step, slot, height, width, finetune.view_flags(crop, flip), C.byref(v))
    assert rc == 0, _capi.load_library().rn_last_error()
    return {"x0": v.x0, "y0": v.y0, "side": v.side, "fliplr": v.fliplr, "flipud": v.flipud}


def test_the_binding_knows_the_new_symbols():
    for name in ("rn_view_draw", "rn_views_create", "rn_views_destroy", "rn_views_batch_device", "rn_ft_run_views"):
        assert name in _capi.EXPORTED_SYMBOLS
    assert (_capi.RN_VIEW_CROP, _capi.RN_VIEW_FLIP, _capi.RN_VIEW_SITE) == (1, 2, 254) == (finetune.VIEW_CROP, finetune.VIEW_FLIP, finetune.VIEW_SITE)
    assert C.sizeof(_capi.rn_view) == 20 and C.sizeof(_capi.rn_view_source) == 16


def test_draw_parity_on_the_grid():
    assert {abs(h - w) for h, w in SIZES} == {0, 1, 7, 840}
    for seed, step, slot, (h, w) in itertools.product(SEEDS, STEPS, SLOTS, SIZES):
        got, want = c_draw(seed, step, slot, h, w), finetune.view_draw(seed, step, slot, h, w)
        assert got == want, (seed, step, slot, h, w, got, want)
        rng, offset = abs(h - w), got["x0"] + got["y0"]
        assert got["side"] == min(h, w) and got["fliplr"] in (0, 1) and got["flipud"] in (0, 1)
        # the window slides along the long axis only, and never reaches offset == range
        assert (got["y0"] == 0) if h < w else (got["x0"] == 0)
        assert 0 <= offset < rng if rng else offset == 0
        assert offset + got["side"] <= max(h, w)


def test_the_step_above_2_to_the_32_is_a_draw_of_its_own():
    draws = {s: tuple(finetune.view_draw(3, s, 5, 1080, 1920).values()) for s in (0, 1, 2 ** 32, 2 ** 32 + 1)}
    assert len(set(draws.values())) == 4


def test_draw_refusals():
    lib, v = _capi.load_library(), _capi.rn_view()
    assert lib.rn_view_draw(0, 0, 0, 10, 10, 3, None) == -1
    assert lib.rn_view_draw(0, 0, 0, 0, 10, 3, C.byref(v)) == -1
    assert lib.rn_view_draw(0, 0, 0, 10, 10, 4, C.byref(v)) == -1
    assert lib.rn_view_draw(0, -1, 0, 10, 10, 3, C.byref(v)) == -5
    assert lib.rn_view_draw(0, 0, -1, 10, 10, 3, C.byref(v)) == -5
    with pytest.raises(ValueError):
        finetune.view_draw(0, -1, 0, 10, 10)


def test_flags_off():
    net = RoomNet(6, im_side=224, compute_bn_mean_var=False, dtype="f32", max_batch=8)
    for (h, w), step in itertools.product(SIZES + ((5, 7), (7, 5), (300, 224)), (0, 3, 2 ** 32)):
        # the coordinates of every pixel: the reference's center_crop names its window
        yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        centre = net.center_crop(np.stack([yy, xx, yy], -1))
        for got in (c_draw(9, step, 2, h, w, crop=False, flip=True), finetune.view_draw(9, step, 2, h, w, crop=False, flip=True)):
            assert (got["y0"], got["x0"]) == tuple(centre[0, 0, :2]) and got["side"] == centre.shape[0] == centre.shape[1]
        for got in (c_draw(9, step, 2, h, w, crop=True, flip=False), finetune.view_draw(9, step, 2, h, w, crop=True, flip=False)):
            assert got["fliplr"] == 0 and got["flipud"] == 0
        # a flag does not move the other flag's draw
        both, crop_only, flip_only = (finetune.view_draw(9, step, 2, h, w, crop=c, flip=f) for c, f in ((1, 1), (1, 0), (0, 1)))
        assert (both["x0"], both["y0"]) == (crop_only["x0"], crop_only["y0"])
        assert (both["fliplr"], both["flipud"]) == (flip_only["fliplr"], flip_only["flipud"])


@pytest.mark.parametrize("shape,S", [((300, 224), 224), ((224, 300), 224), ((448, 448), 224), ((224, 224), 224), ((5, 7), 32), ((97, 60), 40)])
def test_make_view_is_the_flipped_host_resize(shape, S):
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    im = rng.integers(0, 256, shape + (3,), dtype=np.uint8)
    side, span = min(shape), abs(shape[0] - shape[1])
    for offset, lr, ud in itertools.product(sorted({0, span // 2, max(span - 1, 0)}), (0, 1), (0, 1)):
        x0, y0 = (offset, 0) if shape[0] < shape[1] else (0, offset)
        draw = {"x0": x0, "y0": y0, "side": side, "fliplr": lr, "flipud": ud}
        want = resize_linear_u8(np.ascontiguousarray(im[y0:y0 + side, x0:x0 + side]), S, S)
        if lr:
            want = np.fliplr(want)
        if ud:
            want = np.flipud(want)
        got = finetune.make_view(im, draw, S)
        assert got.shape == (S, S, 3) and got.dtype == np.uint8 and got.flags["C_CONTIGUOUS"]
        assert np.array_equal(got, want)
        # view[y][x] = R[flipud ? S-1-y : y][fliplr ? S-1-x : x]
        R = resize_linear_u8(np.ascontiguousarray(im[y0:y0 + side, x0:x0 + side]), S, S)
        y, x = 3, 1
        assert np.array_equal(got[y, x], R[S - 1 - y if ud else y, S - 1 - x if lr else x])


# ---- the distribution at a fixed seed: 6-sigma bounds
def test_flips_are_fair_at_this_seed():
    # 4096 fair coins: mean 2048, sigma 32; 6 sigma = 192
    draws = [finetune.view_draw(2024, 17, slot, 300, 224) for slot in range(4096)]
    for key in ("fliplr", "flipud"):
        count = sum(d[key] for d in draws)
        assert 1856 <= count <= 2240, (key, count)
    both = sum(d["fliplr"] & d["flipud"] for d in draws)
    assert 1024 - 6 * 27.8 <= both <= 1024 + 6 * 27.8, both       # p = 1/4: sigma = sqrt(4096 * 3 / 16) = 27.7


def test_offsets_are_uniform_at_this_seed():
    # 7000 draws over 7 offsets: mean 1000, sigma = sqrt(7000 * 6 / 49) = 29.3; 6 sigma = 176
    counts = np.zeros(7, np.int64)
    for step, slot in itertools.product(range(175), range(40)):
        d = finetune.view_draw(2024, step, slot, 224, 231)
        assert d["y0"] == 0 and 0 <= d["x0"] < 7
        counts[d["x0"]] += 1
    assert counts.sum() == 7000
    assert counts.min() >= 824 and counts.max() <= 1176, counts


def test_view_counters_are_no_dropout_counters():
    for depth in (2, 3):
        sites = finetune.dropout_sites(build_graph(6, 224), depth)
        assert finetune.VIEW_SITE not in sites and max(sites) < finetune.VIEW_SITE < 256
    # the site field is the low byte of the counter's last word, whatever the step
    for step in STEPS:
        assert finetune.view_counter(step, 3)[3] & 0xFF == finetune.VIEW_SITE
        assert finetune.view_counter(step, 3)[3] >> 8 == step >> 32
        assert finetune.view_counter(step, 3)[:3] == (0, 3, step & 0xFFFFFFFF)
    # and the draw is the generator at that counter
    w = finetune.philox4x32(finetune.view_counter(5, 3), (77, 0))
    d = finetune.view_draw(77, 5, 3, 224, 231)
    assert d["x0"] == (int(w[0]) * 7) >> 32 and d["fliplr"] == int(w[1]) >> 31 and d["flipud"] == int(w[2]) >> 31
