"""Deletion and insertion curves of a heat map on the host: the NumPy statement (roomnet_amd/faithfulness.py), the host model of the
rank kernel (rn_faith_rank_model: csrc/rn_faith_rank.h through the built library) and the plan (rn_faith_plan) with its refusals.
No GPU."""
import numpy as np
import pytest

from roomnet_amd import _capi, faithfulness as F

PIXEL_COUNTS = [1, 63, 64, 65, 4095, 4096, 4097, 33489, 50176, 481636]


def special_map(npix, seed):
    """+-0, +-inf, NaNs of both signs, denormals and heavy ties among ordinary values."""
    rng = np.random.default_rng(seed)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, 1e-45, -1e-45, 3.4e38, -3.4e38], np.float32)
    m = np.where(rng.random(npix) < 0.6, special[rng.integers(0, len(special), npix)], rng.normal(0, 1, npix).astype(np.float32))
    m = m.astype(np.float32)
    neg_nan = np.isnan(m) & (rng.random(npix) < 0.5)
    m.view(np.uint32)[neg_nan] = 0xFFC00001                  # NaNs with the sign bit set and a payload
    return m


def maps_of(npix, seed=0):
    rng = np.random.default_rng(seed + npix)
    return np.stack([rng.normal(0, 1, npix).astype(np.float32),                              # random
                     (rng.integers(0, 8, npix) * 0.25 - 1).astype(np.float32),               # eight values: heavy ties
                     np.full(npix, 0.375, np.float32),                                        # all equal
                     np.maximum(rng.normal(-1, 1, npix), 0).astype(np.float32),               # one large zero plateau
                     special_map(npix, seed + npix)])


# ------------------------------------------------------------------------------------------------ the order
def test_ranks_are_a_permutation_and_the_stable_argsort():
    m = maps_of(50176)[0].reshape(224, 224)
    r = F.ranks(m)
    assert r.shape == m.shape and r.dtype == np.uint32
    assert np.array_equal(np.sort(r.ravel()), np.arange(m.size, dtype=np.uint32))
    order = np.argsort(-m.ravel(), kind="stable")
    assert np.array_equal(r.ravel()[order], np.arange(m.size))
    assert (np.diff(m.ravel()[order]) <= 0).all()


def test_ties_signed_zeros_and_nans_rank_as_defined():
    nan = np.float32(np.nan)
    m = np.array([1.0, -0.0, nan, 0.0, 1.0, -np.inf, np.inf, 0.0, -nan, -1.0], np.float32)
    #  order: inf(6), 1(0), 1(4), the zeros in raster order (1, 3, 7), -1(9), -inf(5), the NaNs in raster order (2, 8)
    want = np.empty(10, np.uint32)
    want[[6, 0, 4, 1, 3, 7, 9, 5, 2, 8]] = np.arange(10)
    assert np.array_equal(F.ranks(m), want)
    assert np.array_equal(F.ranks(np.full((5, 5), 2.5, np.float32)).ravel(), np.arange(25))              # all equal: the raster index
    assert np.array_equal(F.ranks(np.arange(25, dtype=np.float32)), np.arange(25)[::-1])                 # a ramp: reversed
    assert np.array_equal(_capi.faith_rank_model(m[None])[0], want)


@pytest.mark.parametrize("npix", PIXEL_COUNTS)
def test_rank_model_of_the_library_equals_the_numpy_ranks(npix):
    maps = maps_of(npix)
    got = _capi.faith_rank_model(maps)
    assert got.dtype == np.uint32 and got.shape == maps.shape
    for k, m in enumerate(maps):
        assert np.array_equal(got[k], F.ranks(m)), (npix, k)


def test_rank_model_refusals():
    with pytest.raises(ValueError):
        _capi.faith_rank_model(np.zeros((0, 4), np.float32))
    with pytest.raises(ValueError):
        _capi.faith_rank_model(np.zeros((2, 0), np.float32))
    with pytest.raises(ValueError):
        _capi.faith_rank_model(np.zeros(4, np.float32))


# ------------------------------------------------------------------------------------------------ steps and masked images
def test_step_counts():
    n = F.step_counts(224, 5)
    assert n[:3] == [0, 10035, 20070] and n[-1] == 224 * 224 and len(n) == 6
    assert all(v % 4 for v in n[1:3])                      # a mask edge in the middle of a dword
    assert F.step_counts(185, 185 * 185) == list(range(185 * 185 + 1))
    assert F.step_counts(694, 1) == [0, 694 * 694]
    assert F.step_counts(694, 7)[3] == (3 * 694 * 694) // 7
    for bad in (0, -1, 224 * 224 + 1):
        with pytest.raises(ValueError):
            F.step_counts(224, bad)


@pytest.mark.parametrize("fill", ["mean", (1, 2, 3)])
def test_deleted_and_inserted_partition_the_pixels(fill):
    rng = np.random.default_rng(3)
    S, J = 19, 7
    im = rng.integers(4, 256, (S, S, 3)).astype(np.uint8)           # no pixel has the colour (1, 2, 3)
    rank = F.ranks(rng.integers(0, 5, (S, S)).astype(np.float32))
    colour = F._fill_of(im, fill)
    for j, n_j in enumerate(F.step_counts(S, J)):
        d, i = F.deleted(im, rank, n_j, fill), F.inserted(im, rank, n_j, fill)
        gone_d, gone_i = rank < n_j, rank >= n_j
        assert gone_d.sum() == n_j and gone_i.sum() == S * S - n_j
        assert (d[gone_d] == colour).all() and np.array_equal(d[~gone_d], im[~gone_d])
        assert (i[gone_i] == colour).all() and np.array_equal(i[~gone_i], im[~gone_i])
        # every pixel is the image's in exactly one of the two
        assert np.array_equal(np.where(gone_d[..., None], i, d), im)
    assert np.array_equal(F.deleted(im, rank, 0, fill), im) and np.array_equal(F.inserted(im, rank, S * S, fill), im)


def test_modes_and_chunks():
    assert F.mode_mask(("deletion", "insertion")) == 3 and F.mode_mask("insertion") == 2 and F.mode_mask(1) == 1
    assert F.mode_slots(3) == [F.DELETION, F.INSERTION] and F.mode_slots(("insertion",)) == [F.INSERTION]
    for bad in (0, 4, "both", (), ("deletion", "x")):
        with pytest.raises(ValueError):
            F.mode_mask(bad)
    assert F.chunks(36, 32) == [(0, 32), (32, 4)] and F.chunks(32, 32) == [(0, 32)]


# ------------------------------------------------------------------------------------------------ curves and areas
def test_curves_host_on_a_forward_that_counts_the_pixels_left():
    """forward = the share of pixels that differ from the all-fill image, on an image with no fill-coloured pixel: the deletion curve
    is 1 - n_j / S^2 and the insertion curve its mirror image, whatever the map."""
    rng = np.random.default_rng(5)
    S, J, fill = 12, 9, (0, 0, 0)
    ims = rng.integers(1, 256, (3, S, S, 3)).astype(np.uint8)
    maps = rng.normal(0, 1, (3, S, S)).astype(np.float32)
    maps[1] = np.round(maps[1])                           # ties
    sizes = []

    def forward(batch):
        sizes.append(len(batch))
        share = (batch != 0).any(-1).reshape(len(batch), -1).mean(1)
        return np.stack([1 - share, share], 1).astype(np.float32)

    curves, aucs, ids, probs = F.curves_host(forward, ims, maps, class_ids=[1, 1, 1], steps=J, modes=3, fill=fill, max_batch=8)
    assert sizes == [3] + [8] * 7 + [4]                   # pass 0, then 3 * 2 * 10 = 60 passes in chunks of 8
    n = np.array(F.step_counts(S, J), np.float64)
    assert (n + n[::-1] == S * S).all()                   # (J divides S^2 here: the insertion curve is the deletion curve mirrored)
    want = ((S * S - n) / (S * S)).astype(np.float32)     # 1 - n_j / S^2, as the forward pass above forms it
    assert curves.shape == (3, 2, J + 1) and aucs.shape == (3, 2)
    for i in range(3):
        assert np.array_equal(curves[i, 0], want) and np.array_equal(curves[i, 1], want[::-1])
    assert np.array_equal(probs, np.array([[0, 1]] * 3, np.float32)) and np.array_equal(ids, [1, 1, 1])
    assert np.array_equal(aucs, F.auc(curves))
    # one mode alone: the same curve in slot 0; the argmax class when none is given
    only = F.curves_host(forward, ims, maps, steps=J, modes="insertion", fill=fill, max_batch=8)
    assert only[0].shape == (3, 1, J + 1) and np.array_equal(only[0][:, 0], curves[:, 1])
    with pytest.raises(ValueError):
        F.curves_host(forward, ims, maps, class_ids=[0, 2, 0], steps=J, max_batch=8)
    with pytest.raises(ValueError):
        F.curves_host(forward, ims, maps, steps=J, max_batch=2)
    with pytest.raises(ValueError):
        F.curves_host(forward, ims, maps[:2], steps=J, max_batch=8)


def test_auc():
    assert F.auc(np.full(33, 0.7, np.float32)) == np.float32(0.7)                  # a constant curve: that constant
    assert F.auc(np.array([0.25, 0.25], np.float32)) == np.float32(0.25)
    assert F.auc(np.linspace(0, 1, 5).astype(np.float32)) == np.float32(0.5)
    c = np.random.default_rng(1).random((2, 2, 6)).astype(np.float32)
    want = np.empty((2, 2), np.float32)
    for i in range(2):
        for s in range(2):
            total = 0.0
            for j in range(5):
                total = total + (float(c[i, s, j]) + float(c[i, s, j + 1]))
            want[i, s] = np.float32(total / 10.0)
    assert np.array_equal(F.auc(c), want) and F.auc(c).dtype == np.float32
    with pytest.raises(ValueError):
        F.auc(np.zeros(1, np.float32))


# ------------------------------------------------------------------------------------------------ the plan
def test_faith_plan_counts_and_refusals():
    assert _capi.faith_plan(224, 5, 3, 3, 32) == (36, 2)
    assert _capi.faith_plan(224, 32, 3, 64, 64) == (64 * 66, 66)
    assert _capi.faith_plan(224, 32, 1, 1, 64) == (33, 1) and _capi.faith_plan(224, 32, 2, 2, 64) == (66, 2)
    assert _capi.faith_plan(185, 185 * 185, 1, 1, 4) == (185 * 185 + 1, (185 * 185 + 1 + 3) // 4)
    assert _capi.faith_plan(224, 16383, 3, 32, 32) == (1 << 20, 1 << 15)             # exactly the limit
    lib = _capi.load_library()
    for what, args, rc in [("J = 0", (224, 0, 3, 1, 8), -1), ("J < 0", (224, -3, 3, 1, 8), -1), ("J > S^2", (224, 50177, 3, 1, 8), -1),
                           ("modes 0", (224, 5, 0, 1, 8), -1), ("modes 4", (224, 5, 4, 1, 8), -1), ("modes -1", (224, 5, -1, 1, 8), -1),
                           ("n = 0", (224, 5, 3, 0, 8), -1), ("side 0", (0, 1, 3, 1, 8), -1), ("max_batch 0", (224, 5, 3, 1, 0), -1),
                           ("n > max_batch", (224, 5, 3, 9, 8), -5), ("too many passes", (224, 16384, 3, 32, 32), -5)]:
        assert lib.rn_faith_plan(*args, None, None) == rc, what
        assert b"rn_faith_plan" in lib.rn_last_error(), what
        with pytest.raises(ValueError):
            _capi.faith_plan(*args)
    assert lib.rn_faith_plan(224, 5, 3, 3, 32, None, None) == 0                      # every pointer may be NULL
