"""The three backward passes -- the trainers at depth 2 (rn_finetune.hip) and depth 3 (rn_finetune7.hip) and grad-CAM
(rn_gradcam.hip) -- against float64 on ``CK.live(graph, 0, CK.LIVE_GAIN)``: 20-31 % of the pre-activations of conv 7, 8, 9 and d0 at
or above 6, about a quarter strictly inside (0, 6), gammas of both signs in every trained BN.  The other GPU tests of these passes
start from the shipped checkpoint, where the upper end of ``relu6_passes`` and the sign of gamma never matter
(tests/test_backward_live_host.py asserts both, and every condition on the inputs used here).

Inputs (tests/backward_ref.py states the cases once, for this file and the CPU one): at 224 the float32 cast of the float64 oracle's
s7.bn / s6.bn of the four parity images ``CK.PARITY_IDX + [52]``, labels ``arange(n) % nc``, batches above 4 tiling the four; at
side 300 (conv 7 is 63 x 63: its last row and column lie in no pool window) seeded normal features; plus the handle's own features.

Bounds -- the project's: per variable max|d| / max|g_ref| <= GRAD_TOL = 1e-5; exact zeros wherever float64 is exactly zero;
conv2d_7/kernel elementwise |d| <= GRAD_TOL max|g| + Amb / n (finetune_ref.conv7_ambiguity) with conv 7's near-kink share <= 1e-4;
the loss within max(5e-6, 4 x |L32 - L64|) of the same call (on `live` with l2 = 0.06 the loss is 14 to 22 and float32 torch itself
misses it by up to 3.8e-6; 4: another summation order).  DELTA[site] = 4 x max|pre32 - pre64| is computed per call from the float32
torch yardstick; that no float64 pre-activation of conv 8, conv 9, d0 .. d3 lies within DELTA[site] of 0 or 6 is a CONDITION on
the inputs (a flip there would reach every upstream gradient), reported as a failed condition and not as a kernel error.  The
tightest case is side 300 at depth 3: conv 8's nearest pre-activation is 1.84e-5 from a kink, DELTA 1.79e-5.
Grad-CAM: 1e-4 of max|alpha| and of max|cam| as in test_hip_gradcam.py, for layer s6.bn plus the room conv 7's near-kink positions
take (backward_ref.gradcam_room6), at the handle's own s6.bn and s7.bn.  The score is d3.mm BEFORE its ReLU6 (include/roomnet_hip.h),
so a class whose logit ReLU6 clamps to exactly 0 has the reference's map, not a zero one; that class is checked against the
reference like the default one.  On 16-bit handles the figures are recorded and only finiteness and the identity of probs / ids with
forward_u8 are asserted: nobody has measured what 16-bit activations do to the masks at O(1) values.

Every test records the kernel's error beside the yardstick's (``record("backward_live", ...)``; profiles/backward_live_parity.json)
before it asserts.  Measured on an MI355X: gradients within 1.7e-6 of their variable's largest entry (float32 torch: 2.3e-6), losses
within 9.2e-7 (float32 torch: up to 3.8e-6), dW7 at most 0.11 of its room, the five-step drift 1.5e-6 (bound 2e-6), grad-CAM within
5.7e-7.  With ``relu6_passes`` cut to ``v > 0`` at conv 7-9 and d0-d2 (by hand, on a copy of the kernels) 26 of the 32 tests here
fail, by up to 14 x a gradient's largest entry: all but the features, one class, ``eval`` and the recorded 16-bit cases."""
import numpy as np
import pytest
import torch

import backward_ref as BR
import checkpoints as CK
import finetune_harness as H
from conftest import parity_set_of
from finetune_harness import LOSS_TOL, SHARE_CAP
from gradcam_ref import GradCamRef
from oracle import roomnet_ref as R
from parity_bounds import MARGIN, TIE_EDGE, _tol
from roomnet_amd import _capi
from roomnet_amd.graph import build_graph

pytestmark = pytest.mark.gpu

SECTION = "backward_live"
CAM_TOL = 1e-4
LAYERS = ("s6.bn", "s7.bn")


@pytest.fixture(scope="module")
def four(parity_images):
    return np.ascontiguousarray(parity_images[BR.ITEMS])


@pytest.fixture(scope="module")
def taps64(four):
    """The float64 oracle's taps of the four items on `live`, computed once and left unchanged (the conv trunk does not depend on
    the head's width)."""
    return R.infer(BR.live_weights(6, 224), four, dtype=np.float64, taps=True)["taps"]


@pytest.fixture(scope="module")
def handle_feats(four):
    """The f32 handle's own features of the four items: ``{2: s7.bn, 3: s6.bn}``."""
    eng = _capi.Engine(build_graph(6, 224), BR.live_weights(6, 224), device=0, dtype="f32", max_batch=4)
    try:
        return {2: eng.features_u8(four), 3: eng.features_u8(four, depth=3)}
    finally:
        eng.close()


def _trainer(case, w, n, **kw):
    return H.trainer(w, case["side"], max(n, 2), case["depth"], case["nc"], l2_coeff=case["l2"], dropout_rate=case["rate"],
                     dropout_seed=BR.DROP_SEED if case["rate"] else 0, **kw)


def _condition(r, case):
    """The conditions on the inputs, after the figures are on record: a violation is the inputs' failure, not the kernel's."""
    assert not r["violations"], "FAILED CONDITION on the inputs (not a kernel error): pre-activations within DELTA of a ReLU6 " \
        "kink (site, distance, DELTA): %s" % r["violations"]
    if case["depth"] == 3:
        assert r["share"] <= SHARE_CAP, "FAILED CONDITION on the inputs (not a kernel error): conv-7 near-kink share %g" % r["share"]


def _check_one_step(case, w, x, y, idx, record):
    """One step of a trainer on slots ``idx`` of ``x`` against float64: the harness's check with the bounds of the module docstring
    (the loss bound and conv 7's DELTA from the yardstick of this very call) and the kink condition on the inputs."""
    r = BR.reference_of(case, w, x, y, idx)
    return H.check_one_step(w, x, y, idx, case["l2"], record, SECTION, case["key"], case["depth"], case["side"], case["nc"],
                            case["rate"], BR.DROP_SEED, reference=r, loss_bound=r["loss_bound"], delta=r["delta"].get("conv7"),
                            condition=lambda: _condition(r, case),
                            extra={"delta": r["delta"], "kink_distance": {s: d for s, d in r["kink_distance"].items() if s != "conv7"}})


def _ids(kind):
    return dict(argvalues=BR.cases(kind), ids=lambda c: c["key"])


# ---------------------------------------------------------------------------------------------- 1. features
def test_features_equal_the_taps_on_live(four, handle_feats):
    eng = _capi.Engine(build_graph(6, 224), BR.live_weights(6, 224), device=0, dtype="f32", max_batch=4)
    try:
        f2, f3 = eng.features_u8(four), eng.features_u8(four, depth=3)
        eng.forward_u8(four)
        assert f2.shape == (4, 21, 21, 16) and f3.shape == (4, 46, 46, 128)
        assert f2.tobytes() == eng.tap("s7.bn", 4).tobytes() and f3.tobytes() == eng.tap("s6.bn", 4).tobytes()
        assert f2.tobytes() == handle_feats[2].tobytes() and f3.tobytes() == handle_feats[3].tobytes()
        assert (np.abs(f2) > 1).any() and (np.abs(f3) > 1).any()                 # O(1) features, not the shipped 1e-2
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------- 2. + 3. one step
@pytest.mark.parametrize("case", **_ids("one_step"))
def test_one_step_loss_and_gradients(taps64, record, case):
    w, x, y, idx = BR.case_inputs(case, taps64)
    _check_one_step(case, w, x, y, idx, record)


def test_one_step_depth_2_at_the_handles_own_features(handle_feats, record):
    """s7.bn as the f32 handle stored it: the kink condition is recomputed on these features at run time."""
    case = BR._case("own_features", 2, 4, 0.06)
    w = BR.live_weights(6, 224)
    _check_one_step(case, w, handle_feats[2], (np.arange(4) % 6).astype(np.int32), np.arange(4, dtype=np.int32), record)


# ---------------------------------------------------------------------------------------------- 4. head widths
@pytest.mark.parametrize("case", **_ids("width"))
def test_head_widths(taps64, record, case):
    w, x, y, idx = BR.case_inputs(case, taps64)
    r, got, losses = _check_one_step(case, w, x, y, idx, record)
    assert got[BR.W_LAST].shape == (8, case["nc"])
    if case["nc"] == 1:
        # one class: softmax is 1, the CE term and every gradient are exactly zero (l2 = 0)
        assert r["L"] == 0.0 and abs(float(losses[0])) <= r["loss_bound"]
        for name, g in got.items():
            assert not g.any(), name


# ---------------------------------------------------------------------------------------------- 5. side 300
@pytest.mark.parametrize("case", **_ids("side_300"))
def test_side_300_odd_conv7(record, case):
    w, x, y, idx = BR.case_inputs(case, None)
    r, got, _ = _check_one_step(case, w, x, y, idx, record)
    if case["depth"] == 3:
        _, u = r["ref"].conv7_adjoint(r["xin"], y[idx])
        assert u.shape[-2:] == (63, 63) and not u[:, :, -1, :].any() and not u[:, :, :, -1].any() and u[:, :, :-1, :-1].any()


# ---------------------------------------------------------------------------------------------- 6. dropout
@pytest.mark.parametrize("case", **_ids("dropout"))
def test_dropout_against_the_host_masks(taps64, record, case):
    w, x, y, idx = BR.case_inputs(case, taps64)
    r, _, _ = _check_one_step(case, w, x, y, idx, record)
    assert all((~m).any() and m.any() for m in r["masks"].values())


# ---------------------------------------------------------------------------------------------- 7. five Adam steps
def test_five_adam_steps_depth_3(taps64, record):
    case = BR._case("five_steps", 3, 4, 0.06)
    w, x, y, idx = BR.case_inputs(case, taps64)
    lr, ns = 2e-4, 10000
    index = np.tile(idx, (5, 1))
    r0 = BR.reference_of(case, w, x, y, idx)
    ref = BR.make_ref(w, 6, 224, 3)
    Lref = ref.train(x, y, index, lr, ns, case["l2"])
    L32 = ref.twin32.train(x, y, index, lr, ns, case["l2"])
    P, P32 = ref.values(), ref.twin32.values()
    tr = _trainer(case, w, 4, learn_rate=lr, num_steps=ns)
    try:
        losses = tr.run_host(x, y, index)
        got = tr.read()
        assert tr.step_count() == 5
    finally:
        tr.close()
    drift = max(float(np.abs(got[n] - P[n]).max()) for n in P)
    drift32 = max(float(np.abs(P32[n] - P[n]).max()) for n in P)
    moved = max(float(np.abs(P[n] - np.asarray(w[n], np.float64)).max()) for n in P)
    dl, dl32 = np.abs(losses - Lref), np.abs(L32 - Lref)
    lbound = np.maximum(LOSS_TOL, 4.0 * dl32)
    bound = max(0.01 * lr, 4.0 * drift32)
    print("five steps: parameter drift %.3g (float32 torch %.3g, bound %.3g), parameters moved %.3g = %.1f lr; loss errors %s "
          "(float32 torch %s, bounds %s)" % (drift, drift32, bound, moved, moved / lr, dl, dl32, lbound))
    record(SECTION, "five_adam_steps_depth_3", {"param_abs": drift, "param_abs_float32_torch": drift32, "bound_param": bound,
                                                "param_moved": moved, "loss_abs": dl.tolist(), "loss_abs_float32_torch": dl32.tolist(),
                                                "loss_bound": lbound.tolist()})
    _condition(r0, case)
    assert moved > 2 * lr
    assert np.all(dl <= lbound)
    assert drift <= bound


# ---------------------------------------------------------------------------------------------- 8. eval_host
@pytest.mark.parametrize("depth", [2, 3])
def test_eval_host(taps64, record, depth):
    case = BR._case("eval", depth, 4, 0.06)
    w, x, y, idx = BR.case_inputs(case, taps64)
    ref = BR.make_ref(w, 6, 224, depth)
    p64, p32 = ref.probs(x), ref.twin32.probs(x)
    L64, L32 = float(ref.loss(x, y, 0.06).detach()), float(ref.twin32.loss(x, y, 0.06).detach())
    with torch.no_grad():
        lg = ref.logits(x).numpy()
    tr = _trainer(case, w, 4)
    try:
        loss, probs, ids = tr.eval_host(x, y)
    finally:
        tr.close()
    ep, tp = float(np.abs(probs - p64).max()), _tol(p64, p32)
    dl, lbound = abs(loss - L64), max(LOSS_TOL, 4.0 * abs(L32 - L64))
    srt = np.sort(lg, axis=1)
    safe = srt[:, -1] - srt[:, -2] > MARGIN
    print("eval depth %d: probs %.3g (float32 torch %.3g, tol %.3g); loss %.3g (float32 torch %.3g, bound %.3g); ids checked %d of 4"
          % (depth, ep, float(np.abs(p32 - p64).max()), tp, dl, abs(L32 - L64), lbound, int(safe.sum())))
    record(SECTION, "eval_host_depth_%d" % depth, {"probs_abs": ep, "probs_abs_float32_torch": float(np.abs(p32 - p64).max()),
                                                   "probs_tol": tp, "loss_abs": dl, "loss_abs_float32_torch": abs(L32 - L64),
                                                   "loss_bound": lbound, "ids_checked": int(safe.sum())})
    assert probs.shape == (4, 6) and ids.shape == (4,)
    assert ep <= tp and dl <= lbound
    np.testing.assert_array_equal(ids[safe], lg.argmax(1)[safe])


# ---------------------------------------------------------------------------------------------- 9. grad-CAM
def _cos(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(a @ b / max(np.linalg.norm(a) * np.linalg.norm(b), 1e-300))


def _gradcam_check(eng, w, ims, layer, record, key, class_ids=None, assert_bounds=True):
    """test_hip_gradcam._kernel_check on `live`: the kernel against float64 at the handle's own s6.bn and s7.bn, with the kink
    condition recomputed on those tensors and, for s6.bn, the room of conv 7's near-kink positions."""
    g = eng.graph
    nc, side, n = g.num_classes, g.im_side, len(ims)
    cam, ids, probs, alpha = eng.grad_cam(ims, class_ids=class_ids, layer=layer, with_alpha=True)
    s6, s7 = eng.tap("s6.bn", n), eng.tap("s7.bn", n)
    cls = ids if class_ids is None else np.asarray(class_ids)
    gc = GradCamRef(w, nc, side)
    r = gc.grad_cam(s6=s6, s7=s7, cls=cls, layer=layer)
    # the head is linearised at the stored s7.bn; conv 7's masks come from the stored s6.bn
    pre64, pre32 = BR.pre_activations(BR.make_ref(w, nc, side, 2), s7)
    c7 = BR.pre_activations(BR.make_ref(w, nc, side, 3), s6)
    pre64["conv7"], pre32["conv7"] = c7[0]["conv7"], c7[1]["conv7"]
    delta = BR.deltas(pre64, pre32)
    violations = BR.kink_violations(pre64, delta, BR.GRADCAM_KINK_SITES)
    amax, cmax = float(np.abs(r["alpha"]).max()), float(np.abs(r["cam"]).max())
    cscale = max(cmax, 1e-6 * max(amax, 1e-30))
    da, dc = np.abs(alpha - r["alpha"]), np.abs(cam - r["cam"])
    room_a, room_c = CAM_TOL * max(amax, 1e-30), CAM_TOL * cscale
    rec = {"alpha_rel": float(da.max() / max(amax, 1e-30)), "cam_rel": float(dc.max() / cscale), "tol": CAM_TOL,
           "max_abs_alpha": amax, "max_abs_cam": cmax, "cosine": _cos(cam, r["cam"]), "delta": delta,
           "kink_distance": {s: d for s, d in BR.kink_distance(pre64).items() if s in BR.GRADCAM_KINK_SITES}}
    share = 0.0
    if layer == "s6.bn":
        g7, _ = gc.grad_s7(s7, cls)
        share, ra, rc = BR.gradcam_room6(gc, s6, g7, delta["conv7"])
        room_a, room_c = room_a + ra, room_c + rc
        rec.update({"near_kink_share": share, "share_cap": SHARE_CAP, "room_alpha_max_rel": float(ra.max() / max(amax, 1e-30)),
                    "room_cam_max_rel": float(rc.max() / cscale), "alpha_over_room_worst": float((da / room_a).max()),
                    "cam_over_room_worst": float((dc / room_c).max())})
    print(key, " ".join("%s=%.3g" % (k, v) for k, v in rec.items() if not isinstance(v, dict)))
    record(SECTION, key, rec)
    assert np.isfinite(cam).all() and np.isfinite(alpha).all() and np.isfinite(probs).all()
    if assert_bounds:
        assert not violations, "FAILED CONDITION on the handle's own activations (not a kernel error): pre-activations within " \
            "DELTA of a ReLU6 kink (site, distance, DELTA): %s" % violations
        assert share <= SHARE_CAP, "FAILED CONDITION (not a kernel error): conv-7 near-kink share %g" % share
        assert amax > 0 and cmax > 0
        assert np.all(da <= room_a), ("%s: alpha" % layer, BR.locate(alpha, r["alpha"]))
        assert np.all(dc <= room_c), ("%s: cam" % layer, BR.locate(cam, r["cam"]))
        for i in range(n):
            if not r["alpha"][i].any():                        # exactly zero in float64: exactly zero on the GPU
                assert not alpha[i].any() and not cam[i].any(), i
    return cam, ids, probs, alpha, r


@pytest.mark.parametrize("nc", [6, 10])
def test_gradcam_f32_on_live(four, record, nc):
    """Both layers, the default class, and per image a class whose logit ReLU6 clamps to exactly 0 (d3.mm further than TIE_EDGE
    below 0): its score d3.mm still has the reference's gradient."""
    g = build_graph(nc, 224)
    w = BR.live_weights(nc, 224)
    eng = _capi.Engine(g, w, device=0, dtype="f32", max_batch=4)
    try:
        ids_f, probs_f = eng.forward_u8(four)
        for layer in LAYERS:
            cam, ids, probs, alpha, r = _gradcam_check(eng, w, four, layer, record, "gradcam_f32_nc%d_%s_default_class" % (nc, layer))
            assert np.array_equal(ids, ids_f) and probs.tobytes() == probs_f.tobytes()
            z = r["z"]
            clamped = [np.flatnonzero(zi < -TIE_EDGE) for zi in z]
            assert any(len(c) for c in clamped)
            cls = np.array([int(c[0]) if len(c) else int(np.argmin(zi)) for c, zi in zip(clamped, z)], np.int32)
            cam0, _, probs0, _, r0 = _gradcam_check(eng, w, four, layer, record, "gradcam_f32_nc%d_%s_clamped_class" % (nc, layer),
                                                    class_ids=cls)
            assert probs0.tobytes() == probs_f.tobytes()
            assert np.array_equal(r0["cls"], cls) and not np.array_equal(cam0, cam)
    finally:
        eng.close()


def test_gradcam_f32_side_300_on_live(record):
    g = build_graph(6, 300)
    assert g.stages[-3].conv_side % 2 == 1
    w = BR.live_weights(6, 300)
    im = parity_set_of(300)[CK.ONE_IMAGE_IDX]
    eng = _capi.Engine(g, w, device=0, dtype="f32", max_batch=1)
    try:
        for layer in LAYERS:
            _gradcam_check(eng, w, im, layer, record, "gradcam_f32_side_300_%s" % layer)
    finally:
        eng.close()


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_gradcam_16bit_on_live_recorded(four, record, dtype):
    w = BR.live_weights(6, 224)
    eng = _capi.Engine(build_graph(6, 224), w, device=0, dtype=dtype, max_batch=4)
    try:
        ids_f, probs_f = eng.forward_u8(four)
        for layer in LAYERS:
            _, ids, probs, _, _ = _gradcam_check(eng, w, four, layer, record, "gradcam_%s_%s_recorded" % (dtype, layer),
                                                 assert_bounds=False)
            assert np.array_equal(ids, ids_f) and probs.tobytes() == probs_f.tobytes()
    finally:
        eng.close()
