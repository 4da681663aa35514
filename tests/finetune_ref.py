"""CPU reference of the fine-tuning trainer (rn_ft_*, csrc/rn_finetune.hip): stages 8-9 and the dense head restated in torch
from a cached ``s7.bn``, with autograd for the gradients and a plain Adam.  ``dtype=torch.float64`` is the reference;
``dtype=torch.float32`` runs the same code as the yardstick for what float32 arithmetic in another summation order costs.

Forward: stage 8 (conv 3x3 VALID -> ReLU6 -> avg-pool 4/2 -> BN), stage 9 (the same + legacy-bilinear resize of s7.bn -> add ->
BN), flatten, dense blocks x @ W [+ b] -> ReLU6 -> [BN], the last ReLU6 applied to the logits too.  Every BN is
(x - moving_mean) / sqrt(moving_variance + eps) * gamma + beta with trainable gamma and beta.
Loss: mean CE(softmax(relu6(z)), y) + l2 * sum over the trained variables of sum(v^2) / 2.
Adam: tf.train.AdamOptimizer with lr(step) = learn_rate * 0.068^(step / num_steps)."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from gradcam_ref import _resize_tables, relu6
from roomnet_amd.graph import BN_EPSILON, build_graph

DECAY_RATE = 0.068


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


class FineTuneRef:
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

    def logits(self, x7, P=None):
        """relu6(z) [N, C] from features [N, S7, S7, 16]."""
        P = P or self.params
        g = self.graph
        x7 = self._t(x7) if not torch.is_tensor(x7) else x7
        s8 = self._stage(x7, g.stages[-2], P)
        b9 = self._stage(s8, g.stages[-1], P)
        s9 = self._bn(b9 + self._resize(x7), g.stages[-1].bn2_name, P)
        x = s9.reshape(s9.shape[0], -1)
        for d in g.dense:
            z = x @ P[d.name + "/kernel"]
            if d.biased:
                z = z + P[d.name + "/bias"]
            x = relu6(z)
            if d.bn_name:
                x = self._bn(x, d.bn_name, P)
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

    def train(self, feats, labels, index, learn_rate, num_steps, l2, start_step=0):
        """Steps over ``index`` [steps, batch]; returns float64 losses [steps] (each before its update)."""
        feats = self._t(feats)
        labels = np.asarray(labels)
        losses = []
        for s, idx in enumerate(np.asarray(index)):
            lr = learn_rate * DECAY_RATE ** ((start_step + s) / num_steps)
            losses.append(self.step(feats[idx], labels[idx], l2, lr))
        return np.asarray(losses, np.float64)

    def values(self):
        return {n: p.detach().to(torch.float64).numpy().copy() for n, p in self.params.items()}
