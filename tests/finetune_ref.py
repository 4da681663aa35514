"""CPU reference of the fine-tuning trainers (rn_ft_*, csrc/rn_finetune.hip and csrc/rn_finetune7.hip), the only statement of
their mathematics in the tests: restated in torch with autograd for the gradients and a plain Adam.  ``dtype=torch.float64`` is the
reference; ``dtype=torch.float32`` runs the same code as the yardstick for what float32 arithmetic in another summation order costs.

``FineTuneRef`` (depth 2) starts from a cached ``s7.bn``.  Forward: stage 8 (conv 3x3 VALID -> ReLU6 -> avg-pool 4/2 -> BN), stage 9
(the same + legacy-bilinear resize of s7.bn -> add -> BN), flatten, dense blocks x @ W [+ b] -> ReLU6 -> [BN], the last ReLU6 applied
to the logits too.  Every BN is (x - moving_mean) / sqrt(moving_variance + eps) * gamma + beta with trainable gamma and beta.
Loss: mean CE(softmax(relu6(z)), y) + l2 * sum over the trained variables of sum(v^2) / 2.
Adam: tf.train.AdamOptimizer with lr(step) = learn_rate * 0.068^(step / num_steps).

``FineTune7Ref`` (depth 3) starts one stage further back, from a cached ``s6.bn``: stage 7 is conv 3x3 VALID 128 -> 16 -> ReLU6 ->
avg-pool 4/2 -> BN (moving statistics, trainable gamma and beta); everything behind its output ``s7.bn`` is ``FineTuneRef``'s.  The
L2 term runs over the 22 trained variables.  ``conv7_ambiguity`` measures how much room conv 7's ReLU6 kinks leave in dW7.  A float32
kernel that sums in another order may put a pre-activation within ``delta`` of 0 or 6 on the other side of the kink.  s7.bn is
continuous in the pre-activation and no gradient goes below stage 7, so such a flip reaches conv2d_7/kernel's gradient alone, by
exactly |u[p, co]| |x6[p + k, ci]| at element [ky, kx, ci, co], where u is the adjoint of relu6(pre) and does not depend on the mask.

Dropout (rn_ft_set_dropout): ``set_masks`` hands either class GIVEN masks, applied at sites 1 and 2 + d of include/roomnet_hip.h in
the kernel's order -- site 1 behind the flatten; hidden dense blocks: the ``mask * scale`` factor sits behind the BN; the last block:
behind its ReLU6, so that the softmax and the CE term read the dropped logits.  With no masks set no factor is applied (not even a
multiplication by 1).  Site 0 (depth 3) is not applied here: the caller forms the dropped ``s6.bn`` itself in float32 NumPy
(``dropped_x6``) and hands it in as the input.  The masks come from the product's host statement of the stream,
``finetune.dropout_keep`` (``host_masks``), which tests/test_dropout_host.py pins to the published Philox vectors and the GPU test
compares with the device's masks byte for byte."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from gradcam_ref import _resize_tables, relu6
from roomnet_amd import finetune
from roomnet_amd.graph import BN_EPSILON, build_graph

DECAY_RATE = 0.068


# The two lists below deliberately differ in where a dense block's /bias sits: behind its BN pair in ``trained_names``, in front of it in
# ``trained_names7``.  Each is kept as it was written; the tests compare both with the product's lists.
def trained_names(graph):
    """Written out here, not imported from the product: the list of section 1 of the issue, generalised to a graph."""
    s8, s9 = graph.stages[-2], graph.stages[-1]
    names = [s8.conv_name + "/kernel", s8.bn_name + "/gamma", s8.bn_name + "/beta",
             s9.conv_name + "/kernel", s9.bn_name + "/gamma", s9.bn_name + "/beta", s9.bn2_name + "/gamma", s9.bn2_name + "/beta"]
    for d in graph.dense:
        names.append(d.name + "/kernel")
        if d.bn_name:
            names += [d.bn_name + "/gamma", d.bn_name + "/beta"]
        if d.biased:
            names.append(d.name + "/bias")
    return names


def trained_names7(graph):
    """The 22 names of the issue, written out here (not imported from the product), generalised to a graph: conv 7's kernel and
    its BN's gamma and beta, then the 19 of depth 2 in their order."""
    s7, s8, s9 = graph.stages[-3], graph.stages[-2], graph.stages[-1]
    names = [s7.conv_name + "/kernel", s7.bn_name + "/gamma", s7.bn_name + "/beta",
             s8.conv_name + "/kernel", s8.bn_name + "/gamma", s8.bn_name + "/beta",
             s9.conv_name + "/kernel", s9.bn_name + "/gamma", s9.bn_name + "/beta", s9.bn2_name + "/gamma", s9.bn2_name + "/beta"]
    for d in graph.dense:
        names.append(d.name + "/kernel")
        if d.biased:
            names.append(d.name + "/bias")
        if d.bn_name:
            names += [d.bn_name + "/gamma", d.bn_name + "/beta"]
    return names


def host_masks(graph, depth, seed, step, n_slots, rate):
    """``{site: bool [n_slots, size]}`` for every site of a trainer of ``depth`` at global step ``step``."""
    return {site: np.stack([finetune.dropout_keep(seed, step, b, site, size, rate) for b in range(n_slots)])
            for site, (_name, size) in finetune.dropout_sites(graph, depth).items()}


def dropped_x6(x6, keep, rate):
    """Site 0 as the pre-pass forms it: ``x6 * scale`` as one float32 product where kept, +0 where dropped.  ``x6`` [n, S6, S6, 128]
    float32 (already gathered in slot order), ``keep`` bool [n, S6 * S6 * 128]."""
    x6 = np.asarray(x6, np.float32)
    return np.where(keep.reshape(x6.shape), x6 * finetune.dropout_scale(rate), np.float32(0.0)).astype(np.float32)


class FineTuneRef:
    depth = 2
    masks = None                                   # set_masks: {site: mask * scale}, for the forward passes of ONE batch
    scale = 1.0

    def __init__(self, weights, num_classes=6, im_side=224, dtype=torch.float64):
        self.graph = g = build_graph(num_classes, im_side)
        self.dtype = dtype
        self.names = trained_names(g)
        self.params = {n: self._t(weights[n]).clone().requires_grad_(True) for n in self.names}
        self.frozen = {}
        for bn in [g.stages[-2].bn_name, g.stages[-1].bn_name, g.stages[-1].bn2_name] + [d.bn_name for d in g.dense if d.bn_name]:
            mean, var = self._t(weights[bn + "/moving_mean"]), self._t(weights[bn + "/moving_variance"])
            self.frozen[bn] = (mean, 1.0 / torch.sqrt(var + BN_EPSILON))
        self.rt = _resize_tables(g.stages[-3].out_side, g.stages[-1].out_side)
        self.m = {n: torch.zeros_like(p) for n, p in self.params.items()}
        self.v = {n: torch.zeros_like(p) for n, p in self.params.items()}
        self.t = 0

    def _t(self, x):
        return torch.as_tensor(np.asarray(x, np.float64)).to(self.dtype)

    # ---- forward
    def _bn(self, x, bn, P):
        mean, rsq = self.frozen[bn]
        return (x - mean) * rsq * P[bn + "/gamma"] + P[bn + "/beta"]

    def _stage(self, x, st, P):
        c = F.conv2d(x.permute(0, 3, 1, 2), P[st.conv_name + "/kernel"].permute(3, 2, 0, 1))
        p = F.avg_pool2d(relu6(c), 4, 2)
        return self._bn(p.permute(0, 2, 3, 1), st.bn_name, P)

    def _resize(self, x):
        lo, hi, lerp = self.rt
        yl = self._t(lerp)[None, :, None, None]
        xl = self._t(lerp)[None, None, :, None]
        tl, tr = x[:, lo][:, :, lo], x[:, lo][:, :, hi]
        bl, br = x[:, hi][:, :, lo], x[:, hi][:, :, hi]
        top = tl + (tr - tl) * xl
        bot = bl + (br - bl) * xl
        return top + (bot - top) * yl

    def set_masks(self, masks, rate):
        """Before every forward pass whose batch the masks belong to (``None``: no dropout)."""
        self.scale = float(finetune.dropout_scale(rate)) if masks is not None else 1.0          # the float32 value, exactly
        self.masks = masks and {site: self._t(np.asarray(m, np.float64)) * self.scale for site, m in masks.items()}

    def logits(self, x7, P=None):
        """relu6(z) [N, C] from features [N, S7, S7, 16]."""
        P = P or self.params
        g = self.graph
        x7 = self._t(x7) if not torch.is_tensor(x7) else x7
        s8 = self._stage(x7, g.stages[-2], P)
        b9 = self._stage(s8, g.stages[-1], P)
        s9 = self._bn(b9 + self._resize(x7), g.stages[-1].bn2_name, P)
        x = s9.reshape(s9.shape[0], -1)
        if self.masks is not None:
            x = x * self.masks[1]
        for i, d in enumerate(g.dense):
            z = x @ P[d.name + "/kernel"]
            if d.biased:
                z = z + P[d.name + "/bias"]
            x = relu6(z)
            if d.bn_name:
                x = self._bn(x, d.bn_name, P)
            if self.masks is not None:
                x = x * self.masks[2 + i]
        return x

    def loss(self, x7, y, l2, P=None):
        P = P or self.params
        r = self.logits(x7, P)
        ce = F.cross_entropy(r, torch.as_tensor(np.asarray(y, np.int64)), reduction="mean")
        reg = sum((p * p).sum() for p in P.values()) * 0.5
        return ce + l2 * reg

    def loss_and_grads(self, x7, y, l2):
        """(loss, {name: gradient}) as float64 numpy, whatever dtype the arithmetic ran in."""
        names = self.names
        L = self.loss(x7, y, l2)
        gs = torch.autograd.grad(L, [self.params[n] for n in names])
        return float(L.detach()), {n: g.detach().to(torch.float64).numpy() for n, g in zip(names, gs)}

    def probs(self, x7):
        with torch.no_grad():
            return torch.softmax(self.logits(x7), dim=-1).to(torch.float64).numpy()

    # ---- Adam
    def step(self, x7, y, l2, lr, beta1=0.9, beta2=0.999, eps=1e-8):
        """One Adam step at learning rate ``lr`` (already decayed); returns the loss before the update."""
        L, _ = self.loss_and_grads(x7, y, l2), None
        loss, grads = L
        self.t += 1
        lr_t = lr * np.sqrt(1.0 - beta2 ** self.t) / (1.0 - beta1 ** self.t)
        with torch.no_grad():
            for n in self.names:
                g = self._t(grads[n])
                self.m[n] = beta1 * self.m[n] + (1.0 - beta1) * g
                self.v[n] = beta2 * self.v[n] + (1.0 - beta2) * g * g
                self.params[n] -= lr_t * self.m[n] / (torch.sqrt(self.v[n]) + eps)
        return loss

    def train(self, feats, labels, index, learn_rate, num_steps, l2, start_step=0, seed=0, rate=0.0):
        """Steps over ``index`` [steps, batch]; returns float64 losses [steps] (each before its update).  With ``rate``, each step
        under its masks: slot b of step s drops by ``dropout_keep(seed, start_step + s, b, ...)`` (depth 2: no site 0)."""
        assert not rate or self.depth == 2
        feats = self._t(feats)
        labels = np.asarray(labels)
        losses = []
        for s, idx in enumerate(np.asarray(index)):
            if rate:
                self.set_masks(host_masks(self.graph, 2, seed, start_step + s, len(idx), rate), rate)
            lr = learn_rate * DECAY_RATE ** ((start_step + s) / num_steps)
            losses.append(self.step(feats[idx], labels[idx], l2, lr))
        return np.asarray(losses, np.float64)

    def values(self):
        return {n: p.detach().to(torch.float64).numpy().copy() for n, p in self.params.items()}


class FineTune7Ref(FineTuneRef):
    """``FineTuneRef`` one stage further back: every method that took ``x7`` [N, S7, S7, 16] takes ``x6`` [N, S6, S6, 128]
    (with masks set: the DROPPED ``x6``, ``dropped_x6``)."""
    depth = 3

    def __init__(self, weights, num_classes=6, im_side=224, dtype=torch.float64):
        super().__init__(weights, num_classes, im_side, dtype)
        g = self.graph
        self.st7 = g.stages[-3]
        self.names = trained_names7(g)
        self.params = {n: self._t(weights[n]).clone().requires_grad_(True) for n in self.names}
        bn = self.st7.bn_name
        self.frozen[bn] = (self._t(weights[bn + "/moving_mean"]), 1.0 / torch.sqrt(self._t(weights[bn + "/moving_variance"]) + BN_EPSILON))
        self.m = {n: torch.zeros_like(p) for n, p in self.params.items()}
        self.v = {n: torch.zeros_like(p) for n, p in self.params.items()}

    def pre7(self, x6, P=None):
        """conv 7's pre-activation [N, 16, C7, C7] (channels first)."""
        P = P or self.params
        x6 = self._t(x6) if not torch.is_tensor(x6) else x6
        return F.conv2d(x6.permute(0, 3, 1, 2), P[self.st7.conv_name + "/kernel"].permute(3, 2, 0, 1))

    def x7_from_act(self, act, P=None):
        """s7.bn [N, S7, S7, 16] from relu6(pre) [N, 16, C7, C7]."""
        P = P or self.params
        return self._bn(F.avg_pool2d(act, 4, 2).permute(0, 2, 3, 1), self.st7.bn_name, P)

    def x7(self, x6, P=None):
        return self.x7_from_act(relu6(self.pre7(x6, P)), P)

    def logits(self, x6, P=None):
        P = P or self.params
        return super().logits(self.x7(x6, P), P)

    def conv7_adjoint(self, x6, y):
        """``(pre, u)`` [N, 16, C7, C7]: conv 7's pre-activation and u = d(sum_i CE_i)/d relu6(pre), the adjoint of the batch's SUMMED
        loss as the kernel carries it before its update divides by n.  u is the pool adjoint: it does not depend on the mask.
        The head behind s7.bn is the masked one when masks are set."""
        with torch.no_grad():
            pre = self.pre7(self._t(x6))
        act = relu6(pre).detach().requires_grad_(True)
        r = FineTuneRef.logits(self, self.x7_from_act(act), self.params)
        L = F.cross_entropy(r, torch.as_tensor(np.asarray(y, np.int64)), reduction="sum")
        (u,) = torch.autograd.grad(L, act)
        return pre, u

    def conv7_ambiguity(self, x6, y, l2, delta):
        """``(share, Amb)``: the share of conv 7's pre-activations within ``delta`` of a ReLU6 kink, and per element of
        conv2d_7/kernel ``Amb[ky, kx, ci, co] = sum over those positions p of |u[p, co]| |x6[p + k, ci]|`` (float64 numpy, HWIO),
        with u of ``conv7_adjoint``: of the summed loss, so that ``Amb / n`` is the room in the gradient of the mean (``l2``
        touches no activation and leaves u alone)."""
        x6 = self._t(x6)
        pre, u = self.conv7_adjoint(x6, y)
        near = ((pre.abs() <= delta) | ((pre - 6.0).abs() <= delta))
        w0 = torch.zeros_like(self.params[self.st7.conv_name + "/kernel"].permute(3, 2, 0, 1)).requires_grad_(True)
        out = F.conv2d(x6.abs().permute(0, 3, 1, 2), w0)
        (amb,) = torch.autograd.grad((out * (u.abs() * near.to(u.dtype))).sum(), w0)
        return float(near.to(torch.float64).mean()), amb.permute(2, 3, 1, 0).to(torch.float64).numpy()


def make_ref(weights, nc, side, depth, masks=None, rate=0.0, cls=None):
    """The float64 reference of a trainer of ``depth`` with ``ref.twin32``, the same class in float32 (the yardstick).  ``masks``
    (with ``rate``) are set on both.  ``cls`` overrides the class (a mutant)."""
    cls = cls or (FineTuneRef if depth == 2 else FineTune7Ref)
    ref, ref.twin32 = cls(weights, nc, side), cls(weights, nc, side, dtype=torch.float32)
    ref.set_masks(masks, rate)
    ref.twin32.set_masks(masks, rate)
    return ref
