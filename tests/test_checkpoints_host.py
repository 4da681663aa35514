"""CPU checks of the seeded checkpoint recipes (tests/checkpoints.py) and of the stage-local restatements (tests/stage_ref.py)
that tests/test_hip_other_checkpoints.py builds on.

The GPU tests of the 16-bit kernels' value-range tricks (weights / 6 and the fp16 clamp, fp16 pooling, folded BN tables) are only
worth something if the checkpoint they run really drives values to the upper ReLU6 clamp AND leaves a good share inside (0, 6), in
every stage -- and the shipped checkpoint does not.  That contrast is asserted here on the fp64 oracle."""
import numpy as np
import pytest

import checkpoints as CK
import stage_ref as SR
from oracle import roomnet_ref as R
from parity_bounds import AT_CLAMP_MIN, INSIDE_MIN
from roomnet_amd.graph import build_graph

SHIPPED_AT_CLAMP_MAX = 1e-4                 # shipped checkpoint: no stage 1-9 above 0.01 % at the clamp


@pytest.fixture(scope="module")
def graph():
    return build_graph(6, 224)


@pytest.fixture(scope="module")
def ims(parity_images):
    return parity_images[CK.PARITY_IDX]


@pytest.fixture(scope="module")
def live_ref(graph, ims):
    w = CK.live(graph, 0, CK.LIVE_GAIN)
    return w, R.infer(w, ims, dtype=np.float64, taps=True)


def test_recipes_are_deterministic(graph):
    for make in (lambda: CK.live(graph, 0, CK.LIVE_GAIN), lambda: CK.init_scale(graph, 0)):
        a, b = make(), make()
        assert sorted(a) == sorted(b) == sorted(graph.variable_shapes())
        for name in a:
            assert a[name].dtype == np.float32 and a[name].shape == tuple(graph.variable_shapes()[name])
            np.testing.assert_array_equal(a[name], b[name])
    a, b = CK.live(graph, 0, CK.LIVE_GAIN), CK.live(graph, 1, CK.LIVE_GAIN)
    assert any((a[name] != b[name]).any() for name in a)


def test_live_recipe_makes_every_bn_live_with_both_signs(graph):
    w = CK.live(graph, 0, CK.LIVE_GAIN)
    init = CK.init_scale(graph, 0)
    bns = sorted({n.rsplit("/", 1)[0] for n in w if n.endswith("/gamma")})
    assert len(bns) == 16
    for bn in bns:
        g, b, m, v = (w["%s/%s" % (bn, p)] for p in ("gamma", "beta", "moving_mean", "moving_variance"))
        assert (np.abs(g) >= 0.5).all() and (np.abs(g) <= 1.5).all() and (g < 0).any() and (g > 0).any(), bn
        assert (np.abs(b) <= 0.5).all() and (b != 0).all() and (m > 0).all() and (m < 1).all(), bn
        assert (v >= 0.5).all() and (v <= 2).all(), bn
    for s in graph.stages:
        np.testing.assert_array_equal(w[s.conv_name + "/kernel"], init[s.conv_name + "/kernel"] * np.float32(CK.LIVE_GAIN))
    for d in graph.dense:
        np.testing.assert_array_equal(w[d.name + "/kernel"], init[d.name + "/kernel"])
    assert (w["dense_3/bias"] != 0).all()


@pytest.mark.parametrize("nc", [1, 2, 10, 64])
def test_live_recipe_has_the_same_conv_trunk_at_every_head_width(graph, nc):
    """The head-width cases of the GPU tests run the conv trunk asserted below: only the last dense layer differs."""
    a, b = CK.live(graph, 0, CK.LIVE_GAIN), CK.live(build_graph(nc, 224), 0, CK.LIVE_GAIN)
    for name in a:
        if not name.startswith("dense_3/"):
            np.testing.assert_array_equal(a[name], b[name], err_msg=name)
    assert b["dense_3/kernel"].shape == (8, nc) and b["dense_3/bias"].shape == (nc,)


def test_live_recipe_saturates_relu6_in_every_stage(live_ref):
    _, ref = live_ref
    shares = CK.clamp_shares(ref["taps"])
    print(" ".join("s%d=%.4f/%.3f" % (k, a, b) for k, (a, b) in enumerate(shares)))
    for k in range(1, 10):
        at6, inside = shares[k]
        assert at6 >= AT_CLAMP_MIN and inside >= INSIDE_MIN, (k, shares)
    # the dense head reaches the clamp as well, and the logits of the three images are told apart
    assert (ref["taps"]["d0.relu"] == 6).any() and (ref["taps"]["d1.relu"] == 6).any()
    lg = np.sort(ref["logits"], axis=1)
    assert ((lg[:, -1] - lg[:, -2]) > 0.1).all()


def test_live_recipe_saturates_relu6_at_side_240():
    """The two-image side-240 case of the stage-local GPU test (the clamp image and the textured one: tests/test_seam_cases_host.py
    asserts what each of them is there for), and the clamp image on its own."""
    from conftest import parity_set_of
    g = build_graph(6, 240)
    w = CK.live(g, 0, CK.LIVE_GAIN)
    for idx in (CK.SEAM_IDX, CK.ONE_IMAGE_IDX):
        ref = R.infer(w, parity_set_of(240)[idx], dtype=np.float64, taps=True)
        shares = CK.clamp_shares(ref["taps"])
        for k in range(1, 10):
            assert shares[k][0] >= AT_CLAMP_MIN and shares[k][1] >= INSIDE_MIN, (idx, k, shares)


def test_init_scale_recipe_is_o1_and_does_not_saturate(graph, ims):
    """init(): identity BNs, activations O(1) (the shipped checkpoint's are O(1e-2)), the clamp out of reach."""
    ref = R.infer(CK.init_scale(graph, 0), ims, dtype=np.float64, taps=True)
    shares = CK.clamp_shares(ref["taps"])
    for k, s in enumerate(graph.stages):
        out = ref["taps"][SR.stage_out_name(s)]
        assert shares[k][0] == 0.0 and shares[k][1] >= INSIDE_MIN, (k, shares)
        assert 0.1 <= np.abs(out).max() <= 6.0, (k, float(np.abs(out).max()))


def test_shipped_checkpoint_practically_never_reaches_the_clamp(graph, ims, weights):
    """The contrast that is the reason for the other-checkpoint tests."""
    ref = R.infer(weights, ims, dtype=np.float64, taps=True)
    shares = CK.clamp_shares(ref["taps"])
    print(" ".join("s%d=%.2e" % (k, a) for k, (a, _) in enumerate(shares)))
    for k in range(1, 10):
        assert shares[k][0] <= SHIPPED_AT_CLAMP_MAX, (k, shares)


def test_stage_local_chain_and_head_local_equal_the_oracle(graph, ims, live_ref):
    """stage_local chained over all ten stages, then head_local, IS oracle/roomnet_ref.py's float64 forward pass."""
    w, ref = live_ref
    taps = ref["taps"]
    x = taps["input"]
    outs = []
    for k, s in enumerate(graph.stages):
        assert s.skip_stage == {3: 1, 5: 4, 9: 7}.get(k, -1)
        x = SR.stage_local(graph, w, k, x, outs[s.skip_stage] if s.residual else None)
        outs.append(x)
        assert SR.rel_err(x, taps[SR.stage_out_name(s)]) <= 1e-12, k
    head = SR.head_local(graph, w, x)
    for name in ("d0.mm", "d0.relu", "d0.bn", "d1.bn", "d2.bn", "d3.mm", "d3.relu"):
        assert SR.rel_err(head[name], taps[name]) <= 1e-12, name
    assert SR.rel_err(head["probs"], taps["softmax"]) <= 1e-12
    np.testing.assert_array_equal(head["ids"], ref["ids"])
    # stage 0's exact input differs from the oracle's float32-rounded one by float32 rounding only
    assert np.abs(SR.preprocess64(ims) - taps["input"]).max() <= 2.0 ** -24


def test_emulated_roundings_stay_inside_the_stage_tolerance(graph, live_ref):
    """stage_local_emulated on the oracle's own tensors (rounded to the storage type, as a handle would store them): the
    documented roundings of one stage on exact inputs are visible and stay inside what the project grants ten compounded stages
    (bf16 stage 7, a K = 1152 contraction of weights rounded to 8 bits, comes closest: 0.0069 of 0.0125).  The stage-local GPU
    test takes the larger of that bound and twice this figure.  Both roundings are idempotent and really round."""
    w, ref = live_ref
    taps = ref["taps"]
    x = np.linspace(-7.0, 7.0, 1001)
    for dtype, tol, ulp in (("bf16", 0.0125, 2.0 ** -8), ("f16", 0.006, 2.0 ** -11)):
        r = SR.round_storage(x, dtype)
        np.testing.assert_array_equal(SR.round_storage(r, dtype), r)
        assert 0 < np.abs(r - x).max() <= ulp * 7.0
        for k in (1, 5, 7, 9):                  # fp16 pooling / rounded lerp / plain pooling / the hi + lo resize
            s = graph.stages[k]
            x_in = SR.round_storage(taps[SR.stage_out_name(graph.stages[k - 1])][:1], dtype)
            skip = SR.round_storage(taps[SR.stage_out_name(graph.stages[s.skip_stage])][:1], dtype) if s.residual else None
            want = SR.stage_local(graph, w, k, x_in, skip)
            emu = SR.rel_err(SR.stage_local_emulated(graph, w, k, x_in, skip, dtype), want)
            print(dtype, k, "%.2e" % emu)
            assert 0 < emu <= tol, (dtype, k, emu)
