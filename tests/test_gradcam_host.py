"""Grad-CAM without a GPU: the float64 reference of tests/gradcam_ref.py against the oracle and against finite differences,
the reduced stage-7 identity the kernels use, roomnet_amd.cam, and RoomNet.grad_cam's argument check."""
import numpy as np
import pytest
import torch

from conftest import parity_set_of
from gradcam_ref import GradCamRef


@pytest.fixture(scope="module")
def setup(weights):
    from oracle import roomnet_ref
    ims = parity_set_of(224)[[1, 14, 52]]
    r = roomnet_ref.infer(weights, ims, dtype=np.float64, taps=True)
    return GradCamRef(weights, 6, 224), r


def test_restatement_matches_oracle_taps(setup):
    ref, r = setup
    T = r["taps"]
    s7 = ref.s7_from_s6(torch.as_tensor(T["s6.bn"])).numpy()
    assert np.abs(s7 - T["s7.bn"]).max() <= 1e-10 * np.abs(T["s7.bn"]).max()
    taps = {}
    ref.logits_from_s7(torch.as_tensor(T["s7.bn"]), taps)
    for k in ("s8.bn", "s9.bn2", "d0.mm", "d1.mm", "d2.mm", "d3.mm"):
        got = taps[k].numpy().reshape(T[k].shape)
        assert np.abs(got - T[k]).max() <= 1e-10 * np.abs(T[k]).max(), k


def _kinks(ref, s6=None, s7=None):
    taps = {}
    if s6 is not None:
        s7 = ref.s7_from_s6(torch.as_tensor(s6), taps)
    z = ref.logits_from_s7(torch.as_tensor(s7), taps)
    masks = [((v > 0) & (v < 6)).numpy() for k, v in sorted(taps.items()) if k.endswith(".pre") or k.endswith(".mm")]
    return z.numpy(), masks


@pytest.mark.parametrize("layer", ["s6.bn", "s7.bn"])
def test_finite_differences(setup, layer):
    ref, r = setup
    T = r["taps"]
    A = T[layer].copy()
    cls = r["ids"]
    out = ref.grad_cam(s6=T["s6.bn"], cls=cls, layer=layer) if layer == "s6.bn" else ref.grad_cam(s7=T["s7.bn"], cls=cls, layer=layer)
    G = out["G"]
    rng = np.random.default_rng(7)
    h = 1e-5
    checked = 0
    for _ in range(24):
        idx = tuple(int(rng.integers(0, s)) for s in A.shape)
        ap, am = A.copy(), A.copy()
        ap[idx] += h
        am[idx] -= h
        kw = "s6" if layer == "s6.bn" else "s7"
        zp, mp = _kinks(ref, **{kw: ap})
        zm, mm = _kinks(ref, **{kw: am})
        if any((a != b).any() for a, b in zip(mp, mm)):
            continue                                      # the step crosses a ReLU6 kink
        i = idx[0]
        fd = (zp[i, cls[i]] - zm[i, cls[i]]) / (2 * h)
        assert abs(fd - G[idx]) <= 1e-6 * max(abs(G).max(), 1e-12), (idx, fd, G[idx])
        checked += 1
    assert checked >= 12


def test_alpha6_identity(setup):
    ref, r = setup
    T = r["taps"]
    out = ref.grad_cam(s6=T["s6.bn"], cls=r["ids"], layer="s6.bn")
    g7, _ = ref.grad_s7(ref.s7_from_s6(torch.as_tensor(T["s6.bn"])).detach(), r["ids"])
    a = ref.alpha6_identity(T["s6.bn"], g7).numpy()
    assert np.abs(a - out["alpha"]).max() <= 1e-10 * np.abs(out["alpha"]).max()


def test_cam_helpers():
    from roomnet_amd import cam
    rng = np.random.default_rng(0)
    m = rng.uniform(0, 3, (46, 46)).astype(np.float32)
    up = cam.upsample(m, 224)
    assert up.shape == (224, 224) and up.dtype == np.float32
    assert up.min() >= 0 and abs(float(up.max()) - 1.0) < 1e-6
    assert cam.upsample(np.stack([m, m]), 100).shape == (2, 100, 100)
    assert not cam.upsample(np.zeros((5, 5)), 20).any()
    im = rng.integers(0, 256, (224, 224, 3), dtype=np.uint8)
    o1 = cam.overlay(im, m, weight=0.4)
    o2 = cam.overlay(im, m.copy(), weight=0.4)
    assert o1.shape == im.shape and o1.dtype == np.uint8 and o1.tobytes() == o2.tobytes()
    assert np.array_equal(cam.overlay(im, m, weight=0.0), im)
    with pytest.raises(ValueError):
        cam.overlay(im, m, weight=2.0)


def test_roomnet_grad_cam_rejects_unknown_layer_without_gpu(weights):
    from roomnet_amd.network import RoomNet
    net = RoomNet(6, im_side=224, compute_bn_mean_var=False)
    with pytest.raises(ValueError, match="layer"):
        net.grad_cam(np.zeros((1, 224, 224, 3), np.uint8), layer="s5.bn2")
    with pytest.raises(ValueError, match="expected"):
        net.grad_cam(np.zeros((224, 224), np.uint8))
    with pytest.raises(ValueError, match="expected"):
        net.grad_cam([np.zeros((224, 224), np.uint8)])
