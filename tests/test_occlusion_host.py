"""Occlusion-sensitivity maps on the host: ``rn_occlusion_plan`` (host only) against ``roomnet_amd.occlusion`` and the NumPy statement
against its definition (include/roomnet_hip.h, occlusion-sensitivity maps).  No GPU."""
import ctypes as C

import numpy as np
import pytest

from roomnet_amd import _capi, occlusion as O

RN_E_INVALID, RN_E_RANGE = -1, -5

GRIDS = [(224, 64, 48), (224, 64, 64), (224, 224, 1), (185, 7, 7), (183, 1, 1)]


def plan(side, patch, stride, n, max_batch):
    lib = _capi.load_library()
    g, nw, nc = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    rc = lib.rn_occlusion_plan(side, patch, stride, n, max_batch, C.byref(g), C.byref(nw), C.byref(nc))
    return rc, g.value, nw.value, nc.value


@pytest.mark.parametrize("S,P,T", GRIDS)
def test_plan_agrees_with_positions(S, P, T):
    pos = O.positions(S, P, T)
    rc, g, nw, nc = plan(S, P, T, 3, 32)
    assert rc == 0 and g == len(pos) == O.grid(S, P, T) and nw == 3 * g * g and nc == -(-nw // 32)
    assert pos == [min(k * T, S - P) for k in range(g)] and pos[0] == 0 and pos[-1] == S - P
    assert all(b > a for a, b in zip(pos, pos[1:])) and all(b - a <= T for a, b in zip(pos, pos[1:]))
    assert _capi.occlusion_plan(S, P, T, 3, 32) == (g, nw, nc)
    assert O.chunks(nw, 32) == [(f, min(32, nw - f)) for f in range(0, nw, 32)] and len(O.chunks(nw, 32)) == nc


def test_stated_positions():
    assert O.positions(224, 64, 48) == [0, 48, 96, 144, 160] and plan(224, 64, 48, 1, 1)[1] == 5
    assert O.positions(224, 64, 64) == [0, 64, 128, 160]
    assert O.positions(224, 224, 1) == [0] and plan(224, 224, 1, 1, 1)[1] == 1
    assert O.positions(185, 7, 7)[-3:] == [168, 175, 178] and plan(185, 7, 7, 1, 1)[1] == 27
    assert plan(183, 1, 1, 1, 32) == (0, 183, 183 * 183, -(-183 * 183 // 32))
    assert plan(224, 64, 48, 3, 32)[1:] == (5, 75, 3)


def test_plan_refusals():
    assert plan(224, 32, 33, 1, 32)[0] == RN_E_INVALID                 # T > P
    assert plan(224, 225, 16, 1, 32)[0] == RN_E_INVALID                # P > S
    for bad in [(0, 1, 1, 1, 32), (224, 0, 1, 1, 32), (224, 32, 0, 1, 32), (224, 32, 16, 0, 32), (224, 32, 16, 1, 0),
                (224, 32, -1, 1, 32), (224, 32, 16, -2, 32)]:
        assert plan(*bad)[0] == RN_E_INVALID, bad                      # any value below 1 (n = 0 lands here)
    assert plan(224, 32, 16, 33, 32)[0] == RN_E_RANGE                  # n > max_batch
    assert plan(224, 32, 16, 32, 32)[0] == 0
    # the 2^20 cap: G = 183 -> 33489 windows per image; 31 images fit, 32 do not
    assert plan(183, 1, 1, 31, 64)[0] == 0 and plan(183, 1, 1, 32, 64)[0] == RN_E_RANGE
    assert plan(1024, 1, 1, 1, 1) == (0, 1024, 1 << 20, 1 << 20) and plan(1025, 1, 1, 1, 1)[0] == RN_E_RANGE
    assert b"rn_occlusion_plan" in _capi.load_library().rn_last_error()
    for bad in [(224, 32, 33), (224, 225, 16), (224, 0, 0)]:
        with pytest.raises(ValueError):
            O.positions(*bad)
    with pytest.raises(ValueError):
        _capi.occlusion_plan(224, 32, 33, 1, 32)


def brute_map(drop, S, P, T):
    """One float32 accumulator per pixel, the windows in ``ky``, then ``kx`` order, one division."""
    pos = O.positions(S, P, T)
    out = np.empty((S, S), np.float32)
    count = np.zeros((S, S), np.int64)
    for y in range(S):
        for x in range(S):
            acc = np.float32(0)
            for ky, py in enumerate(pos):
                if not py <= y < py + P:
                    continue
                for kx, px in enumerate(pos):
                    if px <= x < px + P:
                        acc = np.float32(acc + drop[ky, kx])
                        count[y, x] += 1
            out[y, x] = acc / np.float32(count[y, x])
    return out, count


@pytest.mark.parametrize("S,P,T", [(37, 8, 5), (32, 8, 8), (29, 29, 3), (23, 1, 1), (41, 16, 3)])
def test_every_pixel_is_covered_and_pixel_map_is_the_per_pixel_loop(S, P, T):
    G = O.grid(S, P, T)
    drop = np.random.default_rng(S).standard_normal((G, G)).astype(np.float32)
    want, count = brute_map(drop, S, P, T)
    assert count.min() >= 1
    got = O.pixel_map(drop, S, P, T)
    assert got.dtype == np.float32 and got.shape == (S, S)
    np.testing.assert_array_equal(got, want)
    both = O.pixel_map(np.stack([drop, -drop]), S, P, T)
    np.testing.assert_array_equal(both[0], want)
    np.testing.assert_array_equal(both[1], -want)
    if P == T and (S - P) % T == 0:
        assert count.max() == 1                  # a regular tiling: the map is the drops, block by block
        np.testing.assert_array_equal(got, np.kron(drop, np.ones((P, P), np.float32)))


@pytest.mark.parametrize("S,P,T", [g for g in GRIDS if g[1] > 1])
def test_cover_count_at_the_stated_grids(S, P, T):
    cover = np.zeros(S, int)
    for p in O.positions(S, P, T):
        cover[p:p + P] += 1
    assert cover.min() >= 1


def test_fill_colour_rounds_half_up():
    im = np.zeros((2, 2, 3), np.uint8)
    im[0, 0] = (1, 3, 255)
    im[0, 1] = (1, 0, 255)               # sums 2, 3, 1020 over 4 pixels: 0.5 -> 1, 0.75 -> 1, 255
    im[1, 0] = (0, 0, 255)
    im[1, 1] = (0, 0, 255)
    assert O.fill_colour(im).tolist() == [1, 1, 255] and O.fill_colour(im).dtype == np.uint8
    im[0, 0, 0] = 0                      # 0.25 -> 0
    assert O.fill_colour(im).tolist() == [0, 1, 255]
    im[:, :, 0] = (np.arange(4).reshape(2, 2) * 2 + 1)       # 1 + 3 + 5 + 7 = 16 -> exactly 4
    im[0, 0, 0] = 3                      # 18 / 4 = 4.5 -> 5
    assert O.fill_colour(im)[0] == 5
    rng = np.random.default_rng(0)
    big = rng.integers(0, 256, (185, 185, 3), dtype=np.uint8)
    want = np.floor(big.reshape(-1, 3).astype(np.float64).mean(0) + 0.5)
    assert O.fill_colour(big).tolist() == want.tolist()


def test_masked_touches_only_its_window():
    rng = np.random.default_rng(1)
    im = rng.integers(0, 256, (19, 19, 3), dtype=np.uint8)
    keep = im.copy()
    for y, x, P, fill in [(0, 0, 5, (1, 2, 3)), (14, 3, 5, "mean"), (7, 18, 1, (255, 0, 9)), (0, 0, 19, "mean")]:
        got = O.masked(im, y, x, P, fill)
        inside = np.zeros((19, 19), bool)
        inside[y:y + P, x:x + P] = True
        np.testing.assert_array_equal(got[~inside], im[~inside])
        want = O.fill_colour(im) if fill == "mean" else np.array(fill, np.uint8)
        assert (got[inside] == want).all()
    np.testing.assert_array_equal(im, keep)
    w = O.windows(im, 8, 5, (7, 8, 9))
    pos = O.positions(19, 8, 5)
    assert pos == [0, 5, 10, 11] and w.shape == (16, 19, 19, 3)
    np.testing.assert_array_equal(w[1 * 4 + 3], O.masked(im, 5, 11, 8, (7, 8, 9)))
    with pytest.raises(ValueError):
        O.masked(im, 0, 0, 3, "median")
    with pytest.raises(ValueError):
        O.masked(im, 0, 0, 3, (1, 2, 256))


def test_occlusion_map_host_with_a_toy_forward():
    """p[class 0] = the image's mean blue / 255, p[1] = the rest: covering a bright square with zeros lowers class 0 by its share."""
    S, P, T = 8, 4, 4
    ims = np.zeros((2, S, S, 3), np.uint8)
    ims[0, :4, :4, 0] = 128              # image 0: bright top left quarter
    ims[1, 4:, :, 0] = 64                # image 1: bottom half
    ims[1, 0, 0, 1] = 255                # (another channel: no effect)
    calls = []

    def forward(batch):
        calls.append(len(batch))
        p0 = batch[:, :, :, 0].astype(np.float32).sum((1, 2)) / np.float32(64 * 256)
        return np.stack([p0, np.float32(0.4) * np.ones_like(p0)], 1)

    maps, drops, ids, probs = O.occlusion_map_host(forward, ims, class_ids=[0, 0], patch=P, stride=T, fill=(0, 0, 0), max_batch=3)
    assert calls == [2, 3, 3, 2]                     # pass 0, then 8 masked images in chunks of 3 across the image boundary
    assert probs[:, 0].tolist() == [0.125, 0.125] and ids.tolist() == [1, 1]
    assert drops.shape == (2, 2, 2) and drops.dtype == np.float32
    assert drops[0].tolist() == [[0.125, 0.0], [0.0, 0.0]]
    assert drops[1].tolist() == [[0.0, 0.0], [0.0625, 0.0625]]
    np.testing.assert_array_equal(maps[0], np.kron(drops[0], np.ones((4, 4), np.float32)))
    # the argmax class (1) does not depend on the image: no drop anywhere; and a fill brighter than the image gives negative drops
    _m, d1, _i, _p = O.occlusion_map_host(forward, ims, patch=P, stride=T, fill=(0, 0, 0), max_batch=8, with_map=False)
    assert _m is None and not d1.any()
    _m, d2, _i, _p = O.occlusion_map_host(forward, ims[:1], class_ids=0, patch=P, stride=T, fill=(255, 0, 0), max_batch=8)
    assert d2[0, 1, 1] == np.float32(0.125) - np.float32(0.125 + 16 * 255 / (64 * 256)) and (_m[4:, 4:] < 0).all()
    with pytest.raises(ValueError):
        O.occlusion_map_host(forward, ims, class_ids=[0, 2], patch=P, stride=T)
    with pytest.raises(ValueError):
        O.occlusion_map_host(forward, ims, patch=P, stride=T, max_batch=1)


def test_the_drivers_refuse_a_bad_grid_before_they_touch_anything(tmp_path):
    from roomnet_amd.infer import classify_im_dir
    with pytest.raises(ValueError):
        classify_im_dir(None, str(tmp_path / "nothing"), heatmap="occlusion", occlusion_patch=16, occlusion_stride=17)
    with pytest.raises(ValueError):
        classify_im_dir(None, str(tmp_path / "nothing"), heatmap="occlusion", overlay=False)
    assert not (tmp_path / "nothing_classified").exists()
