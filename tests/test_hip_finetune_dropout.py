"""Dropout while fine-tuning on the GPU (rn_ft_set_dropout, rn_ft_dropout, rn_ft_dropout_mask; RoomNet.fine_tune(dropout_rate=)):
the device's masks against the host statement of the stream byte for byte, one step's loss and gradients at depth 2, at the 600
geometry and at depth 3, and a 20-step Adam trajectory against the float64 reference with the host masks
(tests/finetune_ref.py with ``set_masks``), determinism and the identities the step counter in the generator's counter buys, and the Python
surface.

Bounds: the project's existing ones, unchanged, stated with the checks in tests/finetune_harness.py; conv 7's room is evaluated on the
DROPPED s6.bn; trajectory: every parameter within max(0.01 learn_rate, 3 x the float32 torch run's drift) of float64.
Each test records the kernel's error beside the float32 torch run of the same masked mathematics through
``record("finetune_dropout", ...)``.

The depth-3 seed: with SEED = 2024 the float64 reference at the float64 oracle's s6.bn (c_oracle, the 32 items below, shipped
checkpoint, rate 0.35) has a near-kink share of 3.2e-5 at batch 1 and 3.4e-5 at batch 45, under the cap of 1e-4 -- checked on the
CPU before the first GPU run.

The 600 case's seed: its synthetic features meet the shipped head's BN statistics far from where those were taken, and with four
scaled sites behind them float32 arithmetic itself is ill-conditioned for most seeds -- the float32 torch run of the same masked
mathematics misses float64's logits by up to 3.1e-5 and its CE term by up to 1.6e-5 over seeds 0-23 (without dropout: 3.4e-6 and
9.1e-7), and at SEED = 2024 (float32 torch: logits 1.4e-5, CE 5.6e-6) the kernel measured |d loss| 1.34e-5 and gradients 9.5e-6, all
variables alike: the softmax, not the strided loop.  SEED_600 = 3 is the first seed from 0 for which the float32 torch run stays
within 5e-6 on the logits (4.1e-6) and a third of the gradient bound (1.1e-6) while each item keeps a logit strictly inside its
ReLU6 and undropped, so that every gradient is live -- chosen on the CPU from the reference's own error."""
import numpy as np
import pytest
import torch

import finetune_harness as H
from finetune_harness import LABELS, RN_E_INVALID, RN_E_RANGE, feats, images, starts  # noqa: F401  (fixtures)
from finetune_ref import FineTuneRef, host_masks
from roomnet_amd import _capi, finetune
from roomnet_amd.graph import build_graph
from roomnet_amd.network import RoomNet

pytestmark = pytest.mark.gpu

SEED = 2024
SEED_600 = 3
SEED_HI = (0x9E3 << 32) | 0x5EED                         # above 2^32: the key's second word is not zero
SITE0 = 46 * 46 * 128
SECTION = "finetune_dropout"

_trainer, _state, _same = H.trainer, H.state, H.same_bytes


def _batch_index(steps, batch, seed=11):
    """``[steps, batch]`` items of the 32: batch 45 repeats items in other slots of the same step."""
    return np.random.default_rng(seed).integers(0, 32, (steps, batch)).astype(np.int32)


# ---- 1. masks
@pytest.mark.parametrize("depth", [2, 3])
def test_masks_equal_the_host_statement(weights, depth):
    tr = _trainer(weights, depth=depth)
    try:
        sites = finetune.dropout_sites(tr.graph, depth)
        assert {k: v[1] for k, v in sites.items()} == ({1: 64, 2: 32, 3: 16, 4: 8, 5: 6} if depth == 2 else
                                                      {0: SITE0, 1: 64, 2: 32, 3: 16, 4: 8, 5: 6})
        assert tr.dropout() == (0.0, 0)
        for site, (_name, size) in sites.items():
            assert tr.dropout_mask(site, 3, 1, size).all()            # rate 0: all ones
        for rate in (0.2, 0.35):
            for seed in (SEED, SEED_HI):
                tr.set_dropout(rate, seed)
                assert tr.dropout() == (float(np.float32(rate)), seed)
                for step in (0, 1, 12345):
                    for slot in (0, 44):
                        for site, (_name, size) in sites.items():
                            got = tr.dropout_mask(site, step, slot, size)
                            ref = finetune.dropout_keep(seed, step, slot, site, size, rate)
                            assert got.dtype == np.uint8 and got.tobytes() == ref.astype(np.uint8).tobytes(), (rate, seed, step, slot, site)
        # a count that is no multiple of four, and a step above 2^32 (its high word sits beside the site in the counter)
        big = (3 << 32) | 9
        assert tr.dropout_mask(1, big, 44, 7).tobytes() == finetune.dropout_keep(SEED_HI, big, 44, 1, 7, 0.35).astype(np.uint8).tobytes()
        assert tr.dropout_mask(1, big, 44, 64).tobytes() != tr.dropout_mask(1, 9, 44, 64).tobytes()
    finally:
        tr.close()


def test_mask_and_rate_errors(weights):
    keep = np.zeros(SITE0 + 8, np.uint8)
    for depth in (2, 3):
        tr = _trainer(weights, depth=depth, max_batch=8)
        try:
            tr.set_dropout(0.35, SEED)
            call = lambda site, step, slot, count: tr.lib.rn_ft_dropout_mask(tr.handle, site, step, slot, count, keep.ctypes.data)
            assert call(0, 0, 0, 4) == (RN_E_INVALID if depth == 2 else 0)
            assert call(6, 0, 0, 4) == RN_E_INVALID and b"site" in tr.lib.rn_last_error()
            assert call(-1, 0, 0, 4) == RN_E_INVALID
            for site, size in ((1, 64), (2, 32), (5, 6)) + (((0, SITE0),) if depth == 3 else ()):
                assert call(site, 0, 0, 0) == RN_E_RANGE
                assert call(site, 0, 0, size + 1) == RN_E_RANGE and b"count" in tr.lib.rn_last_error()
                assert call(site, 0, 0, size) == 0
            assert call(1, 0, -1, 4) == RN_E_RANGE and b"slot" in tr.lib.rn_last_error()
            assert call(1, 0, 8, 4) == RN_E_RANGE
            assert call(1, 0, 7, 4) == 0
            for bad in (1.0, -0.1, float("nan"), 2.0):
                assert tr.lib.rn_ft_set_dropout(tr.handle, bad, 1) == RN_E_RANGE and b"rate" in tr.lib.rn_last_error()
                with pytest.raises(ValueError, match="rate"):
                    tr.set_dropout(bad, 1)
            assert tr.dropout() == (float(np.float32(0.35)), SEED)      # unchanged by the refused calls
        finally:
            tr.close()
    with pytest.raises(ValueError, match="rate"):
        _trainer(weights, dropout_rate=1.0)


# ---- 2.-4. one step's loss and gradients
@pytest.mark.parametrize("batch", [1, 3, 45])
@pytest.mark.parametrize("l2", [0.06, 0.0])
@pytest.mark.parametrize("start", ["shipped", "fresh"])
@pytest.mark.parametrize("rate", [0.35, 0.2])
def test_one_step_depth_2(starts, feats, record, rate, start, l2, batch):
    idx = np.arange(batch, dtype=np.int32) % 32             # batch 45: items 0-12 occur again in slots 32-44, under other masks
    r, _, _ = H.check_one_step(starts[start], feats[2], LABELS, idx, l2, record, SECTION,
                               "one_step_rate_%g_%s_l2_%g_batch_%d" % (rate, start, l2, batch), 2, rate=rate, seed=SEED)
    masks, G = r["masks"], r["G"]
    if batch == 1 and l2 == 0.0:
        # the zero check above is not empty: a dropped input's whole kernel row has no gradient
        for site, name in ((1, "dense/kernel"), (2, "dense_1/kernel"), (3, "dense_2/kernel"), (4, "dense_3/kernel")):
            dropped = ~masks[site][0]
            assert dropped.any() and not G[name][dropped].any(), name


def test_one_step_600_geometry(weights, record):
    """The 3136-element site 1: 512 threads stride over it, so the mask index is the element and not the thread."""
    g = build_graph(6, 600)
    assert finetune.dropout_sites(g, 2)[1][1] == 3136
    w = dict(weights)
    w["dense/kernel"] = np.random.default_rng(600).uniform(-0.04, 0.04, (g.flat_len, 32)).astype(np.float32)
    rng = np.random.default_rng(68)
    x7 = (rng.standard_normal((2, 68, 68, 16)) * 0.5).astype(np.float32)
    y = np.array([2, 5], np.int32)
    ref = FineTuneRef(w, 6, 600)
    ref.set_masks(host_masks(g, 2, SEED_600, 0, 2, 0.35), 0.35)
    with torch.no_grad():
        r = ref.logits(x7).numpy()
    assert (((r > 0) & (r < 6.0 * ref.scale)).sum(1) >= 1).all(), "an item without a live logit: its head gradient is zero"
    H.check_one_step(w, x7, y, np.arange(2), 0.06, record, SECTION, "one_step_600", 2, side=600, rate=0.35, seed=SEED_600)


@pytest.mark.parametrize("batch", [1, 45])
def test_one_step_depth_3(starts, feats, record, batch):
    idx = np.arange(batch, dtype=np.int32) % 32
    H.check_one_step(starts["shipped"], feats[3], LABELS, idx, 0.06, record, SECTION, "one_step_depth_3_batch_%d" % batch, 3, rate=0.35, seed=SEED)


# ---- 5. trajectory
def test_trajectory_20_steps(starts, feats, record):
    H.check_trajectory(starts["shipped"], feats[2], _batch_index(20, 45), record, SECTION, "trajectory", 2, drift32_factor=3, rate=0.35,
                       seed=SEED)


# ---- 6. determinism and identity
@pytest.mark.parametrize("depth", [2, 3])
def test_same_calls_same_bytes_and_step_splitting(starts, feats, depth):
    steps, batch = (20, 45) if depth == 2 else (4, 9)
    H.check_determinism(starts["fresh"], feats[depth], _batch_index(steps, batch), depth, dropout_rate=0.35, dropout_seed=SEED_HI)


@pytest.mark.parametrize("depth", [2, 3])
def test_resumed_run_uses_the_masks_of_its_global_step(starts, feats, depth):
    """One step with equal inputs and equal masks: with learn_rate 0 the parameters stay put, so step 7 of a run from 0 and the
    first step of a run resumed at start_step = 7 see the same parameters and the same minibatch; they must use the same masks and
    so give the same loss and gradient bits -- and step 0's differ."""
    w = starts["fresh"]
    row = _batch_index(1, 8)
    kw = dict(depth=depth, max_batch=8, learn_rate=0.0, l2_coeff=0.06, dropout_rate=0.35, dropout_seed=SEED)
    tr = _trainer(w, **kw)
    try:
        first = tr.run_host(feats[depth], LABELS, row)
        g0 = tr.read(_capi.RN_FT_GRAD)
        rest = tr.run_host(feats[depth], LABELS, np.tile(row, (7, 1)))
        g7 = tr.read(_capi.RN_FT_GRAD)
        assert tr.step_count() == 8
        for n, v in tr.read().items():
            assert v.tobytes() == np.asarray(w[n], np.float32).tobytes(), n
    finally:
        tr.close()
    tr = _trainer(w, start_step=7, **kw)
    try:
        assert tr.step_count() == 7
        resumed = tr.run_host(feats[depth], LABELS, row)
        gr = tr.read(_capi.RN_FT_GRAD)
    finally:
        tr.close()
    assert resumed.tobytes() == rest[6:7].tobytes() and resumed.tobytes() != first.tobytes()
    for n in gr:
        assert gr[n].tobytes() == g7[n].tobytes(), n
    assert any(g0[n].tobytes() != g7[n].tobytes() for n in g0)


@pytest.mark.parametrize("depth", [2, 3])
def test_rate_0_is_the_trainer_without_dropout(starts, feats, depth):
    w = starts["fresh"]
    index = _batch_index(3, 8)
    out = []
    for how in ("never", "zero", "on_then_off"):
        tr = _trainer(w, depth=depth, max_batch=8, learn_rate=2e-4, l2_coeff=0.06)
        try:
            if how == "zero":
                tr.set_dropout(0.0, SEED)
            elif how == "on_then_off":
                tr.set_dropout(0.35, SEED)
                tr.set_dropout(0.0, SEED)
            losses = tr.run_host(feats[depth], LABELS, index)
            out.append((losses, _state(tr) + [tr.read(_capi.RN_FT_GRAD)]))
        finally:
            tr.close()
    for other in out[1:]:
        assert out[0][0].tobytes() == other[0].tobytes()
        _same(out[0][1], other[1])


@pytest.mark.parametrize("depth", [2, 3])
def test_eval_never_drops(starts, feats, depth):
    w = starts["shipped"]
    res = []
    for rate in (0.0, 0.35):
        tr = _trainer(w, depth=depth, max_batch=8, l2_coeff=0.06, dropout_rate=rate, dropout_seed=SEED)
        try:
            res.append(tr.eval_host(feats[depth], LABELS))
        finally:
            tr.close()
    (l0, p0, i0), (l1, p1, i1) = res
    assert l0 == l1 and p0.tobytes() == p1.tobytes() and i0.tobytes() == i1.tobytes()


# ---- 7. Python
def test_fine_tune_with_dropout_rate(weights, images, feats, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    f = feats[2]

    def net_of(**kw):
        net = RoomNet(6, im_side=224, compute_bn_mean_var=False, learn_rate=2e-4, l2_regularizer_coeff=0.06, dtype="f32", max_batch=32, **kw)
        net.init()
        net.set_variables({k: v for k, v in weights.items() if k in net.graph.variable_shapes()})
        return net

    net = net_of(optimized_inference=True)               # (infer returns the softmax beside the ids)
    try:
        index = finetune.epoch_indices(32, 8, 5, seed=[3, 0])
        tr = _capi.Trainer(net.graph, net.sess.variables, max_batch=32, learn_rate=2e-4, l2_coeff=0.06, dropout_rate=0.35, dropout_seed=3)
        try:
            by_hand = tr.run_host(f, LABELS, index)
            params = tr.read()
        finally:
            tr.close()
        out = net.fine_tune(f, LABELS, steps=5, batch_size=8, seed=3, dropout_rate=0.35)
        assert out["losses"].tobytes() == by_hand.tobytes() and out["step"] == 5 and net.step == 5
        for n, v in params.items():
            assert net.sess.variables[n].tobytes() == v.tobytes(), n
        ids, probs = net.infer(images)
        ids2, probs2 = net.infer(images)
        assert probs.tobytes() == probs2.tobytes() and np.array_equal(ids, ids2) and np.isfinite(probs).all()
    finally:
        net.sess.close()
    plain = net_of()
    try:
        out_plain = plain.fine_tune(f, LABELS, steps=5, batch_size=8, seed=3)
        assert out_plain["losses"].tobytes() != out["losses"].tobytes()
        out_zero = net_of()
        try:
            assert out_zero.fine_tune(f, LABELS, steps=5, batch_size=8, seed=3, dropout_rate=0.0)["losses"].tobytes() == \
                out_plain["losses"].tobytes()
        finally:
            out_zero.sess.close()
    finally:
        plain.sess.close()
    ref_net = net_of(dropout_enabled=True, dropout_rate=0.35)
    try:
        with pytest.raises(ValueError, match="dropout"):
            ref_net.fine_tune(f, LABELS, steps=1)
        out_ref = ref_net.fine_tune(f, LABELS, steps=5, batch_size=8, seed=3, dropout_rate=ref_net.dropout_rate)
        assert out_ref["losses"].tobytes() == out["losses"].tobytes()
    finally:
        ref_net.sess.close()
