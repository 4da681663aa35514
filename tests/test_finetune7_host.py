"""Host side of depth-3 fine-tuning (roomnet_amd/finetune.py) and the float64 reference its GPU tests measure against
(tests/finetune_ref.py): the reference's gradients against finite differences, the trained-variable list and the feature shape of
both depths, and the shapes ``RoomNet.fine_tune`` accepts.  No GPU."""
import numpy as np
import pytest
import torch

from finetune_ref import FineTune7Ref
from roomnet_amd import finetune
from roomnet_amd.graph import build_graph

NEW_3 = ["conv2d_7/kernel", "batch_normalization_9/gamma", "batch_normalization_9/beta"]
SECTION_1 = ["conv2d_8/kernel", "batch_normalization_10/gamma", "batch_normalization_10/beta",
             "conv2d_9/kernel", "batch_normalization_11/gamma", "batch_normalization_11/beta",
             "batch_normalization_12/gamma", "batch_normalization_12/beta",
             "dense/kernel", "batch_normalization_13/gamma", "batch_normalization_13/beta",
             "dense_1/kernel", "batch_normalization_14/gamma", "batch_normalization_14/beta",
             "dense_2/kernel", "batch_normalization_15/gamma", "batch_normalization_15/beta",
             "dense_3/kernel", "dense_3/bias"]


def test_reference_gradients_against_finite_differences(weights):
    """Autograd of the float64 restatement against central differences of its loss: 2 random items at the 224 geometry, a handful
    of coordinates of each of the three new variables and of dense/kernel.  Per variable max |fd - g| <= 1e-6 max |g|, the bound of
    the depth-2 reference's test: with h = 1e-5 the truncation term is O(h^2) = 1e-10 of the third derivative, the rounding term
    1e-16 L / h = 1e-11 L.  (A coordinate whose step carries a conv-7 pre-activation across a ReLU6 kink would break this; with 2
    x 44 x 44 x 16 pre-activations of typical size 0.1 and a shift of at most h |x6| = 2e-5 none of the seeded picks does.)"""
    rng = np.random.default_rng(17)
    x6 = rng.standard_normal((2, 46, 46, 128)) * 0.5
    y = np.array([1, 4])
    ref = FineTune7Ref(weights, 6, 224)
    assert ref.names == NEW_3 + SECTION_1
    l2 = 0.06
    _, grads = ref.loss_and_grads(x6, y, l2)
    x6t = ref._t(x6)
    h = 1e-5
    for name in NEW_3 + ["dense/kernel"]:
        p = ref.params[name]
        g = grads[name].reshape(-1)
        flat = p.detach().view(-1)
        picks = rng.choice(flat.numel(), size=min(6, flat.numel()), replace=False)
        worst = 0.0
        for k in picks:
            old = float(flat[k])
            with torch.no_grad():
                flat[k] = old + h
                lp = float(ref.loss(x6t, y, l2))
                flat[k] = old - h
                lm = float(ref.loss(x6t, y, l2))
                flat[k] = old
            worst = max(worst, abs((lp - lm) / (2 * h) - g[k]))
        assert np.abs(g).max() > 0, name
        assert worst <= 1e-6 * np.abs(g).max(), (name, worst, np.abs(g).max())


def test_ambiguity_is_the_room_a_flipped_mask_takes(weights):
    """conv7_ambiguity against its definition.  u is the adjoint it claims to be: n x the mean loss's dW7 equals
    sum_p x6[p + k, ci] u[p, co] mask[p, co] (so a flipped mask at p moves dW7 of the mean by |u| |x6| / n, nothing else).  Amb
    equals the sum written out over the near positions one by one; delta = 0 leaves no room; a larger delta leaves no less."""
    rng = np.random.default_rng(23)
    x6 = rng.standard_normal((2, 46, 46, 128)) * 0.5
    y = np.array([0, 3])
    ref = FineTune7Ref(weights, 6, 224)
    pre, u = ref.conv7_adjoint(x6, y)
    pre, u = pre.numpy(), u.numpy()
    mask = ((pre > 0) & (pre < 6)).astype(np.float64)
    _, g = ref.loss_and_grads(x6, y, 0.0)
    um = u * mask
    direct = np.zeros((3, 3, 128, 16))
    for ky in range(3):
        for kx in range(3):
            direct[ky, kx] = np.einsum("nyxc,noyx->co", x6[:, ky:ky + 44, kx:kx + 44, :], um)
    gw = g["conv2d_7/kernel"]
    assert np.abs(direct - 2 * gw).max() <= 1e-12 * np.abs(gw).max()
    share0, amb0 = ref.conv7_ambiguity(x6, y, 0.0, 0.0)
    assert share0 == 0.0 and not amb0.any()
    delta = 1e-4
    share, amb = ref.conv7_ambiguity(x6, y, 0.0, delta)
    near = (np.abs(pre) <= delta) | (np.abs(pre - 6.0) <= delta)
    assert near.any() and share == pytest.approx(near.mean(), rel=1e-12)
    brute = np.zeros((3, 3, 128, 16))
    for n, co, yy, xx in zip(*np.nonzero(near)):
        brute[:, :, :, co] += abs(u[n, co, yy, xx]) * np.abs(x6[n, yy:yy + 3, xx:xx + 3, :])
    assert amb.shape == (3, 3, 128, 16) and np.abs(amb - brute).max() <= 1e-12 * brute.max()
    share2, amb2 = ref.conv7_ambiguity(x6, y, 0.06, 2 * delta)
    assert share2 >= share and np.all(amb2 >= amb - 1e-15)


def test_trained_variables_and_feature_shape_of_both_depths():
    for side, s7, s6 in ((224, 21, 46), (300, 30, 65), (600, 68, 140)):
        g = build_graph(6, side)
        assert finetune.trained_variables(g) == SECTION_1
        assert finetune.trained_variables(g, depth=2) == SECTION_1
        assert finetune.trained_variables(g, depth=3) == NEW_3 + SECTION_1
        assert len(finetune.trained_variables(g, depth=3)) == 22
        shapes = g.variable_shapes()
        assert shapes["conv2d_7/kernel"] == (3, 3, 128, 16)
        assert finetune.feature_shape(g) == finetune.feature_shape(g, depth=2) == (s7, s7, 16)
        assert finetune.feature_shape(g, depth=3) == (s6, s6, 128)
        assert finetune.depth_of_features(g, (s7, s7, 16)) == 2 and finetune.depth_of_features(g, (s6, s6, 128)) == 3
    g = build_graph(6, 224)
    for bad in (1, 4, 0, None):
        with pytest.raises(ValueError):
            finetune.trained_variables(g, depth=bad)
        with pytest.raises(ValueError):
            finetune.feature_shape(g, depth=bad)


def test_binding_declares_the_depth_entry_points():
    from roomnet_amd import _capi
    for name in ("rn_features_depth_shape", "rn_features_depth_u8", "rn_features_depth_u8_device", "rn_ft_create_depth", "rn_ft_depth"):
        assert name in _capi.EXPORTED_SYMBOLS
    lib = _capi.load_library()
    assert lib.rn_ft_create_depth.restype is not None and len(lib.rn_ft_create_depth.argtypes) == 6


def test_fine_tune_rejects_a_feature_shape_of_neither_depth():
    from roomnet_amd.network import RoomNet
    net = RoomNet(6, im_side=224, compute_bn_mean_var=False, learn_rate=3e-4)
    net.init()
    with pytest.raises(ValueError, match="neither depth"):
        net.fine_tune(np.zeros((2, 44, 44, 16), np.float32), [0, 1], steps=1)
    with pytest.raises(ValueError, match="neither depth"):
        net.fine_tune(np.zeros((2, 46, 46, 64), np.float32), [0, 1], steps=1)
    with pytest.raises(ValueError, match="depth 3"):                          # depth-2 features, an explicit depth-3 request
        net.fine_tune(np.zeros((2, 21, 21, 16), np.float32), [0, 1], steps=1, depth=3)
    with pytest.raises(ValueError, match="depth 2"):
        net.fine_tune(np.zeros((2, 46, 46, 128), np.float32), [0, 1], steps=1, depth=2)
    with pytest.raises(ValueError):
        net.fine_tune(np.zeros((2, 21, 21, 16), np.float32), [0, 1], steps=1, depth=4)
    with pytest.raises(ValueError):
        net.extract_features(np.zeros((1, 224, 224, 3), np.uint8), depth=5)
