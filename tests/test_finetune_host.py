"""Host side of fine-tuning (roomnet_amd/finetune.py) and the float64 reference the GPU tests measure against
(tests/finetune_ref.py): the reference's gradients against finite differences, the schedule, the minibatch order, the Adam rule
and the trained-variable list.  No GPU."""
import numpy as np
import pytest
import torch

from finetune_ref import FineTuneRef
from roomnet_amd import finetune
from roomnet_amd.graph import build_graph

SECTION_1 = ["conv2d_8/kernel", "batch_normalization_10/gamma", "batch_normalization_10/beta",
             "conv2d_9/kernel", "batch_normalization_11/gamma", "batch_normalization_11/beta",
             "batch_normalization_12/gamma", "batch_normalization_12/beta",
             "dense/kernel", "batch_normalization_13/gamma", "batch_normalization_13/beta",
             "dense_1/kernel", "batch_normalization_14/gamma", "batch_normalization_14/beta",
             "dense_2/kernel", "batch_normalization_15/gamma", "batch_normalization_15/beta",
             "dense_3/kernel", "dense_3/bias"]


def test_reference_gradients_against_finite_differences(weights):
    """The yardstick itself: autograd of the float64 restatement against central differences of its loss, 2 random items at the
    224 geometry, a dozen coordinates per variable.  Per variable max |fd - g| <= 1e-6 max |g|: with h = 1e-5 the truncation
    term is O(h^2) = 1e-10 of the third derivative and the rounding term 1e-16 L / h = 1e-11 L."""
    rng = np.random.default_rng(11)
    x7 = rng.standard_normal((2, 21, 21, 16)) * 0.5
    y = np.array([1, 4])
    ref = FineTuneRef(weights, 6, 224)
    l2 = 0.06
    _, grads = ref.loss_and_grads(x7, y, l2)
    h = 1e-5
    for name in ref.names:
        p = ref.params[name]
        g = grads[name].reshape(-1)
        flat = p.detach().view(-1)
        picks = rng.choice(flat.numel(), size=min(12, flat.numel()), replace=False)
        worst = 0.0
        for k in picks:
            old = float(flat[k])
            with torch.no_grad():
                flat[k] = old + h
                lp = float(ref.loss(x7, y, l2))
                flat[k] = old - h
                lm = float(ref.loss(x7, y, l2))
                flat[k] = old
            worst = max(worst, abs((lp - lm) / (2 * h) - g[k]))
        assert np.abs(g).max() > 0, name
        assert worst <= 1e-6 * np.abs(g).max(), (name, worst, np.abs(g).max())


def test_learn_rate_schedule():
    for step, lr, ns in ((0, 1e-4, 10000), (1, 1e-4, 10000), (2500, 2e-3, 10000), (10000, 1e-4, 10000), (12345, 3e-4, 777)):
        assert finetune.learn_rate_at(step, lr, ns) == pytest.approx(lr * 0.068 ** (step / ns), rel=1e-15)
    assert finetune.learn_rate_at(10000, 1.0, 10000) == pytest.approx(0.068, rel=1e-15)
    assert finetune.learn_rate_at(5, 1.0, 10, decay_rate=0.25) == pytest.approx(0.5, rel=1e-15)


def test_epoch_indices_cover_each_epoch_once_and_reshuffle():
    n, batch = 32, 5                      # 6 batches per epoch, 2 items dropped
    per = n // batch
    idx = finetune.epoch_indices(n, batch, 4 * per + 2, seed=5)
    assert idx.shape == (4 * per + 2, batch) and idx.dtype == np.int32
    epochs = [idx[e * per:(e + 1) * per].reshape(-1) for e in range(4)]
    for ep in epochs:
        assert len(set(ep.tolist())) == per * batch            # every kept item exactly once
        assert ep.min() >= 0 and ep.max() < n
    assert any(not np.array_equal(epochs[0], ep) for ep in epochs[1:])          # a fresh shuffle per epoch
    assert len({frozenset(set(range(n)) - set(ep.tolist())) for ep in epochs}) > 1   # and other items dropped
    assert np.array_equal(idx, finetune.epoch_indices(n, batch, 4 * per + 2, seed=5))
    assert not np.array_equal(idx, finetune.epoch_indices(n, batch, 4 * per + 2, seed=6))
    assert finetune.epoch_indices(4, 9, 3, seed=0).shape == (3, 4)              # a batch larger than the set is cut to it
    whole = finetune.epoch_indices(8, 8, 2, seed=1)
    assert sorted(whole[0].tolist()) == list(range(8)) and sorted(whole[1].tolist()) == list(range(8))


def test_adam_update_against_reference(weights):
    rng = np.random.default_rng(3)
    x7 = rng.standard_normal((3, 21, 21, 16)) * 0.5
    y = np.array([0, 2, 5])
    ref = FineTuneRef(weights, 6, 224)
    mine = ref.values()
    m = {k: np.zeros_like(v) for k, v in mine.items()}
    v = {k: np.zeros_like(v) for k, v in mine.items()}
    lr0, ns, l2 = 2e-4, 100, 0.06
    for s in range(3):
        _, grads = ref.loss_and_grads(x7, y, l2)          # gradients at the reference's current parameters
        lr = finetune.learn_rate_at(7 + s, lr0, ns)
        ref.step(x7, y, l2, lr)
        for k in mine:
            mine[k], m[k], v[k] = finetune.adam_update(mine[k], grads[k], m[k], v[k], s + 1, lr)
        now = ref.values()
        for k in mine:
            assert np.abs(mine[k] - now[k]).max() <= 1e-12, (s, k)
    moved = max(np.abs(mine[k] - np.asarray(weights[k], np.float64)).max() for k in mine)
    assert moved > 2 * lr0                                  # three steps of about lr each


def test_trained_variables_match_the_list():
    for side in (224, 600):
        g = build_graph(6, side)
        assert finetune.trained_variables(g) == SECTION_1
        shapes = g.variable_shapes()
        assert all(n in shapes for n in SECTION_1)
    assert finetune.feature_shape(build_graph(6, 224)) == (21, 21, 16)
    assert finetune.feature_shape(build_graph(6, 600)) == (68, 68, 16)


def test_binding_declares_the_trainer():
    from roomnet_amd import _capi
    for name in ("rn_features_shape", "rn_features_u8", "rn_features_u8_device", "rn_ft_create", "rn_ft_destroy", "rn_ft_run",
                 "rn_ft_eval", "rn_ft_var_count", "rn_ft_var_info", "rn_ft_read", "rn_ft_step_count"):
        assert name in _capi.EXPORTED_SYMBOLS
    lib = _capi.load_library()
    assert lib.rn_ft_run.restype is not None
    import ctypes
    assert ctypes.sizeof(_capi.rn_ft_config) == 32


def test_fine_tune_refuses_dropout_before_touching_a_device():
    from roomnet_amd.network import RoomNet
    net = RoomNet(6, im_side=224, compute_bn_mean_var=False, dropout_enabled=True, learn_rate=3e-4, l2_regularizer_coeff=0.06,
                  num_steps=1234)
    assert (net.learn_rate, net.l2_regularizer_coeff, net.num_steps) == (3e-4, 0.06, 1234)
    net.init()
    with pytest.raises(ValueError, match="dropout"):
        net.fine_tune(np.zeros((2, 21, 21, 16), np.float32), [0, 1], steps=1)
    with pytest.raises(NotImplementedError):
        net.train_step(None, None)
