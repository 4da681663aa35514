"""Helpers for the backward-pass tests on a checkpoint that saturates ReLU6 (tests/test_backward_live_host.py on the CPU,
tests/test_hip_backward_live.py on the GPU): what is specific to that checkpoint, on top of the one reference
(tests/finetune_ref.py; ``make_ref`` gives a float64 reference with its float32 twin, the yardstick, as ``ref.twin32``), ``GradCamRef``
and the one-step reference and bounds of tests/finetune_harness.py.

* ``pre_activations``: the pre-activation of every ReLU6 site -- conv 7 (depth 3), conv 8, conv 9, d0 .. d3 -- in float64 and in the
  yardstick; ``deltas``: 4 x max |pre32 - pre64| per site (4: a kernel sums in another order than torch does);
  ``kink_violations``: sites where a float64 pre-activation lies within its delta of 0 or 6.  At conv 8 and behind, a mask flipped
  there reaches every upstream gradient, so the GPU tests take it as a CONDITION on their inputs; at conv 7 a flip reaches dW7 alone
  and ``FineTune7Ref.conv7_ambiguity`` bounds it.
* ``gradcam_room6``: the room conv 7's near-kink positions leave in grad-CAM's alpha and map of layer s6.bn.
* Mutants of the references, for the CPU evidence that a wrong rule is visible on `live` and invisible on the shipped checkpoint:
  ``open_masks`` (the ReLU6 adjoint of the conv stages and of d0 .. d2 passes where x > 0, the upper end dropped) and
  ``abs_gamma_adjoint`` (the BN adjoint towards its input multiplies by |gamma|).  Both leave every forward value bit for bit alone."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

import checkpoints as CK
from finetune_harness import GRAD_TOL, LOSS_TOL, SHARE_CAP, W7, grad_errors, locate, one_step_reference  # noqa: F401  (BR.NAME)
from finetune_ref import FineTune7Ref, make_ref  # noqa: F401
from gradcam_ref import relu6
from roomnet_amd.graph import build_graph

CONV_SITES = ("conv7", "conv8", "conv9")
HEAD_SITES = ("d0", "d1", "d2", "d3")
KINK_SITES = ("conv8", "conv9") + HEAD_SITES      # a flip here reaches every upstream gradient: no room, a condition instead
GRADCAM_KINK_SITES = ("conv8", "conv9", "d0", "d1", "d2")      # grad-CAM's score is d3.mm: the last ReLU6 is not in its path
ITEMS = CK.PARITY_IDX + [52]                      # the four parity images the forward tests on `live` use
W_LAST = "dense_3/kernel"
DROP_RATE, DROP_SEED = 0.35, 2024


# ---------------------------------------------------------------------------------------------- the cases of the GPU file
def _case(kind, depth, batch, l2, nc=6, side=224, rate=0.0):
    key = "%s_depth_%d_nc_%d_side_%d_batch_%d_l2_%g" % (kind, depth, nc, side, batch, l2)
    return {"key": key, "kind": kind, "depth": depth, "batch": batch, "l2": l2, "nc": nc, "side": side, "rate": rate}


ONE_STEP_CASES = (
    [_case("one_step", 2, b, l2) for l2 in (0.06, 0.0) for b in (1, 3, 4, 45)]
    + [_case("one_step", 3, b, l2) for l2 in (0.06, 0.0) for b in (1, 4, 45)]
    + [_case("width", 3, 4, 0.06, nc=nc) for nc in (2, 10, 64)] + [_case("width", 3, 4, 0.0, nc=1)]
    + [_case("side_300", d, 2, 0.06, side=300) for d in (3, 2)]
    + [_case("dropout", d, 3, 0.06, rate=DROP_RATE) for d in (2, 3)])


def cases(kind):
    return [c for c in ONE_STEP_CASES if c["kind"] == kind]


def live_weights(nc, side):
    return CK.live(build_graph(nc, side), 0, CK.LIVE_GAIN)


def features_224(taps64, depth):
    """The float32 cast of the float64 oracle's s7.bn (depth 2) or s6.bn (depth 3) of ``ITEMS``."""
    return np.ascontiguousarray(np.asarray(taps64["s7.bn" if depth == 2 else "s6.bn"]).astype(np.float32))


def features_300(depth):
    """Side 300 without a trunk: conv 7 is 63 x 63, so its last row and column lie in no pool window."""
    shape = (2, 30, 30, 16) if depth == 2 else (2, 65, 65, 128)
    return np.random.default_rng(300).standard_normal(shape).astype(np.float32)


def case_inputs(case, taps64):
    """``(weights, x [items, ...] float32, labels [items] int32, idx [batch] int32)``: batches above the item count tile the items."""
    w = live_weights(case["nc"], case["side"])
    if case["side"] == 300:
        x, y = features_300(case["depth"]), np.array([2, 5], np.int32)
    else:
        x = features_224(taps64, case["depth"])
        y = (np.arange(len(x)) % case["nc"]).astype(np.int32)
    idx = (np.arange(case["batch"]) % len(x)).astype(np.int32)
    return w, x, y, idx


def reference_of(case, w, x, y, idx):
    """Everything the CPU and the GPU test of one case need from the references, computed once: the harness's one-step reference
    (float64 loss and gradients, the yardstick's) and, on top, the pre-activations, DELTA, the kink condition's violations, the loss
    bound and at depth 3 conv 7's near-kink share and Amb at DELTA["conv7"]."""
    r = one_step_reference(w, x, y, idx, case["l2"], case["depth"], case["side"], case["nc"], case["rate"], DROP_SEED)
    pre64, pre32 = pre_activations(r["ref"], r["xin"])
    delta = deltas(pre64, pre32)
    r.update({"pre64": pre64, "delta": delta, "violations": kink_violations(pre64, delta), "kink_distance": kink_distance(pre64),
              "loss_bound": max(LOSS_TOL, 4.0 * abs(r["L32"] - r["L"]))})
    if case["depth"] == 3:
        r["share"], r["amb"] = r["ref"].conv7_ambiguity(r["xin"], y[idx], case["l2"], delta["conv7"])
    return r


def _forward_pre(ref, x):
    """``{site: pre-activation}`` (float64 numpy) of one forward pass of ``ref`` in ITS arithmetic, and the ReLU6'd logits.  A
    restatement of ``ref.logits`` that keeps what feeds each ReLU6; tests/test_backward_live_host.py asserts that its logits are
    ``ref.logits``' bit for bit."""
    g, P = ref.graph, ref.params
    masks = ref.masks
    out = {}
    with torch.no_grad():
        x = ref._t(x) if not torch.is_tensor(x) else x
        if isinstance(ref, FineTune7Ref):
            pre = ref.pre7(x)
            out["conv7"] = pre
            x7 = ref.x7_from_act(relu6(pre))
        else:
            x7 = x
        h = x7
        for site, st in (("conv8", g.stages[-2]), ("conv9", g.stages[-1])):
            c = F.conv2d(h.permute(0, 3, 1, 2), P[st.conv_name + "/kernel"].permute(3, 2, 0, 1))
            out[site] = c
            h = ref._bn(F.avg_pool2d(relu6(c), 4, 2).permute(0, 2, 3, 1), st.bn_name, P)
        s9 = ref._bn(h + ref._resize(x7), g.stages[-1].bn2_name, P)
        h = s9.reshape(s9.shape[0], -1)
        if masks is not None:
            h = h * masks[1]
        for i, d in enumerate(g.dense):
            z = h @ P[d.name + "/kernel"]
            if d.biased:
                z = z + P[d.name + "/bias"]
            out["d%d" % i] = z
            h = relu6(z)
            if d.bn_name:
                h = ref._bn(h, d.bn_name, P)
            if masks is not None:
                h = h * masks[2 + i]
    return {k: v.to(torch.float64).numpy() for k, v in out.items()}, h.to(torch.float64).numpy()


def pre_activations(ref, x):
    """``(pre64, pre32)``: per ReLU6 site the pre-activation tensor on input ``x`` in float64 and in the float32 torch yardstick
    (``ref.twin32``), both as float64 numpy.  Conv sites are [N, C, H, W], head sites [N, width]."""
    return _forward_pre(ref, x)[0], _forward_pre(ref.twin32, x)[0]


def deltas(pre64, pre32):
    """``DELTA[site]`` = 4 x max |pre32 - pre64|: how far a float32 kernel that sums in another order may put a pre-activation."""
    return {s: 4.0 * float(np.abs(pre32[s] - pre64[s]).max()) for s in pre64}


def kink_distance(pre):
    """Per site the smallest distance of a pre-activation from 0 or 6."""
    return {s: float(np.minimum(np.abs(v), np.abs(v - 6.0)).min()) for s, v in pre.items()}


def kink_violations(pre64, delta, sites=KINK_SITES):
    """``[(site, distance, delta)]`` of the sites that break the kink condition (empty: the condition holds)."""
    dist = kink_distance(pre64)
    return [(s, dist[s], delta[s]) for s in sites if s in pre64 and not dist[s] > delta[s]]


def clamp_shares(pre):
    """Per site ``(share at or above 6, share strictly inside (0, 6))``."""
    return {s: (float((v >= 6.0).mean()), float(((v > 0.0) & (v < 6.0)).mean())) for s, v in pre.items()}


# ---------------------------------------------------------------------------------------------- grad-CAM room, layer s6.bn
def gradcam_room6(gc, s6, g7, delta):
    """``(share, room_alpha [N, 128], room_cam [N, S6, S6])`` for a ``GradCamRef`` ``gc`` at stored ``s6`` with ``g7 = dS/ds7.bn``:
    the reduced form of ``GradCamRef.alpha6_identity`` is alpha6[c] = sum_co Gamma[co] wsum[c, co] / S^2 with Gamma[co] the sum over
    conv-7 positions p of gpool[p, co] mask[p, co], and gpool -- the pool adjoint of g7 times the BN factor -- does not depend on
    the mask.  A mask flipped at a position within ``delta`` of a kink moves alpha6[c] by |gpool[p, co]| |wsum[c, co]| / S^2, so
    ``room_alpha[c]`` is the sum of that over the near positions, and the map, 1-Lipschitz in sum_c alpha[c] A[.., c], moves by at
    most ``room_cam = sum_c |A[.., c]| room_alpha[c]``."""
    s6 = torch.as_tensor(np.asarray(s6, np.float64))
    taps = {}
    gc.s7_from_s6(s6, taps)
    pre = taps["s7.pre"].permute(0, 3, 1, 2)                                      # [N, 16, C7, C7]
    _mean, inv, _beta = gc.bn[gc.st7.index]
    gp = (torch.as_tensor(np.asarray(g7, np.float64)) * inv).permute(0, 3, 1, 2)
    pre_c = pre.detach().clone().requires_grad_(True)
    (gpool,) = torch.autograd.grad(F.avg_pool2d(pre_c, 4, 2), pre_c, grad_outputs=gp)
    near = (pre.abs() <= delta) | ((pre - 6.0).abs() <= delta)
    gam = (gpool.abs() * near.to(torch.float64)).sum(dim=(2, 3))                  # [N, 16]
    wsum = gc.w7_hwio.sum(dim=(0, 1)).abs()                                       # [128, 16]
    side = s6.shape[1]
    room_alpha = (gam @ wsum.T) / float(side * side)
    room_cam = torch.einsum("nyxc,nc->nyx", s6.abs(), room_alpha)
    return float(near.to(torch.float64).mean()), room_alpha.numpy(), room_cam.numpy()


# ---------------------------------------------------------------------------------------------- mutants
class _Relu6Open(torch.autograd.Function):
    """ReLU6 whose adjoint passes wherever x > 0: the upper end of the mask dropped.  The forward values are ``relu6``'s."""

    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return relu6(x).detach()

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return torch.where(x > 0, g, torch.zeros_like(g))


def relu6_open(x):
    return _Relu6Open.apply(x)


def open_masks(base):
    """``base`` (the FineTuneRef or FineTune7Ref class) with the mask ``x > 0`` at every ReLU6 whose pre-activation stays below 6
    from the shipped checkpoint: the conv stages and the hidden dense blocks d0 .. d2.  The logits keep 0 < x < 6 (from the shipped
    checkpoint they do reach 6, and the existing tests see that mask)."""
    class OpenMasks(base):
        def _stage(self, x, st, P):
            c = F.conv2d(x.permute(0, 3, 1, 2), P[st.conv_name + "/kernel"].permute(3, 2, 0, 1))
            return self._bn(F.avg_pool2d(relu6_open(c), 4, 2).permute(0, 2, 3, 1), st.bn_name, P)

        def x7(self, x6, P=None):
            return self.x7_from_act(relu6_open(self.pre7(x6, P)), P)

        def logits(self, x, P=None):
            # (FineTuneRef.logits with the other ReLU6 in the hidden blocks)
            P = P or self.params
            g = self.graph
            x = self._t(x) if not torch.is_tensor(x) else x
            x7 = self.x7(x, P) if isinstance(self, FineTune7Ref) else x
            s8 = self._stage(x7, g.stages[-2], P)
            b9 = self._stage(s8, g.stages[-1], P)
            s9 = self._bn(b9 + self._resize(x7), g.stages[-1].bn2_name, P)
            h = s9.reshape(s9.shape[0], -1)
            for d in g.dense:
                z = h @ P[d.name + "/kernel"]
                if d.biased:
                    z = z + P[d.name + "/bias"]
                h = relu6_open(z) if d.bn_name else relu6(z)
                if d.bn_name:
                    h = self._bn(h, d.bn_name, P)
            return h
    return OpenMasks


def abs_gamma_adjoint(base):
    """``base`` with a BN whose adjoint towards its input multiplies by |gamma|; gamma's and beta's own gradients and every forward
    value stay (y = a + (b - b.detach()) with b - b.detach() exactly zero)."""
    class AbsGammaAdjoint(base):
        def _bn(self, x, bn, P):
            mean, rsq = self.frozen[bn]
            xh = (x - mean) * rsq
            b = xh * P[bn + "/gamma"].detach().abs()
            return (xh.detach() * P[bn + "/gamma"] + P[bn + "/beta"]) + (b - b.detach())
    return AbsGammaAdjoint


def grad_change(G, Gm):
    """Per variable max |Gm - G| / max |G| (0 where G is all zero and Gm equals it)."""
    out = {}
    for n in G:
        d = float(np.abs(Gm[n] - G[n]).max())
        out[n] = d / max(float(np.abs(G[n]).max()), 1e-300) if d else 0.0
    return out
