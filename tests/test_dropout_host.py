"""The host statement of the fine-tuning dropout stream (roomnet_amd/finetune.py: philox4x32, dropout_threshold, dropout_scale,
dropout_sites, dropout_keep) and the interface around it, without a GPU: the published Philox4x32-10 known answers, the integer
thresholds, the properties of the keep mask, the exported symbols and the argument checks of RoomNet.fine_tune."""
import numpy as np
import pytest

from roomnet_amd import _capi, finetune
from roomnet_amd.graph import build_graph
from roomnet_amd.network import RoomNet

# counter, key, output: the known-answer vectors published with the generator (Random123, kat_vectors: philox4x32 10)
KAT = (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)))
SITE0 = 46 * 46 * 128          # one s6.bn item at 224: 270 848 elements


@pytest.mark.parametrize("counter,key,out", KAT)
def test_philox_known_answers(counter, key, out):
    got = finetune.philox4x32(counter, key)
    assert got.dtype == np.uint32 and got.shape == (4,)
    assert tuple(int(v) for v in got) == out
    # an array of counters gives each its own answer
    many = finetune.philox4x32(np.array([counter, (0, 0, 0, 0), counter], np.uint64), key)
    assert many.shape == (3, 4) and tuple(int(v) for v in many[0]) == out and tuple(int(v) for v in many[2]) == out


def test_thresholds_and_scale():
    assert finetune.dropout_threshold(np.float32(0.2)) == 3355444
    assert finetune.dropout_threshold(np.float32(0.35)) == 5872026
    assert finetune.dropout_threshold(np.float32(0.5)) == 8388608
    assert finetune.dropout_threshold(0.35) == 5872026            # a Python float is rounded to float32 first, as the C ABI takes it
    assert finetune.dropout_threshold(0.0) == 0
    s = finetune.dropout_scale(0.35)
    assert isinstance(s, np.float32) and s == np.float32(1.0) / (np.float32(1.0) - np.float32(0.35))
    assert finetune.dropout_scale(0.0) == np.float32(1.0)
    for bad in (1.0, -0.1, float("nan"), 1.5):
        with pytest.raises(ValueError):
            finetune.dropout_threshold(bad)
        with pytest.raises(ValueError):
            finetune.dropout_scale(bad)


def test_sites():
    g = build_graph(6, 224)
    s3, s2 = finetune.dropout_sites(g, 3), finetune.dropout_sites(g, 2)
    assert {k: v[1] for k, v in s3.items()} == {0: SITE0, 1: 64, 2: 32, 3: 16, 4: 8, 5: 6}
    assert s3[0][0] == "s6.bn" and 0 not in s2 and {k: v for k, v in s3.items() if k} == s2
    assert finetune.dropout_sites(build_graph(6, 600), 2)[1][1] == 3136
    with pytest.raises(ValueError):
        finetune.dropout_sites(g, 4)


def test_keep_is_a_prefix_and_follows_the_counter():
    seed, rate = (9 << 32) | 77, 0.35
    full = finetune.dropout_keep(seed, 3, 2, 1, 64, rate)
    assert full.dtype == np.bool_ and full.shape == (64,)
    for n in (6, 7, 64):
        assert np.array_equal(finetune.dropout_keep(seed, 3, 2, 1, n, rate), full[:n])
    # element e is word e & 3 of the output for the counter (e >> 2, slot, step lo, site | step hi << 8)
    step = (5 << 32) | 12345
    thr = finetune.dropout_threshold(rate)
    for e in (0, 5, 63):
        w = finetune.philox4x32((e >> 2, 2, step & 0xffffffff, 4 | (5 << 8)), (seed & 0xffffffff, seed >> 32))
        assert bool(finetune.dropout_keep(seed, step, 2, 4, 64, rate)[e]) == ((int(w[e & 3]) >> 8) >= thr)
    base = finetune.dropout_keep(seed, 3, 2, 1, 64, rate)
    for other in (finetune.dropout_keep(seed, 3, 2, 2, 64, rate), finetune.dropout_keep(seed, 3, 3, 1, 64, rate),
                  finetune.dropout_keep(seed, 4, 2, 1, 64, rate), finetune.dropout_keep(seed + 1, 3, 2, 1, 64, rate),
                  finetune.dropout_keep(seed + (1 << 32), 3, 2, 1, 64, rate), finetune.dropout_keep(seed, 3 + (1 << 32), 2, 1, 64, rate)):
        assert not np.array_equal(base, other)
    assert finetune.dropout_keep(seed, 3, 2, 1, 64, 0.0).all()


@pytest.mark.parametrize("rate", [0.2, 0.35])
def test_kept_share(rate):
    keep = finetune.dropout_keep(1234, 0, 0, 0, SITE0, rate)
    p = 1.0 - finetune.dropout_threshold(rate) / 2.0 ** 24
    sd = np.sqrt(p * (1.0 - p) / SITE0)
    assert abs(keep.mean() - (1.0 - rate)) <= 5 * sd, (keep.mean(), sd)


def test_symbols_are_exported():
    for name in ("rn_ft_set_dropout", "rn_ft_dropout", "rn_ft_dropout_mask"):
        assert name in _capi.EXPORTED_SYMBOLS


@pytest.mark.parametrize("enabled", [False, True])
def test_fine_tune_refuses_bad_rates_before_a_device_is_touched(enabled):
    net = RoomNet(6, im_side=224, compute_bn_mean_var=False, dropout_enabled=enabled, dtype="f32", max_batch=8)
    feats = np.zeros((2, 21, 21, 16), np.float32)
    for bad in (1.0, -0.1, float("nan")):
        with pytest.raises(ValueError, match="dropout_rate"):
            net.fine_tune(feats, [0, 1], steps=1, dropout_rate=bad)
    assert net.dropout_rate == 0.2
