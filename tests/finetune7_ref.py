"""CPU reference of the depth-3 fine-tuning trainer (rn_ft_create_depth, csrc/rn_finetune7.hip + csrc/rn_finetune.hip): the whole
last conv block, stages 7-9, and the dense head restated in torch from a cached ``s6.bn``, with autograd for the gradients and the
plain Adam of ``finetune_ref.FineTuneRef``.  ``dtype=torch.float64`` is the reference; ``dtype=torch.float32`` runs the same code
as the yardstick for what float32 arithmetic in another summation order costs.

Stage 7 is conv 3x3 VALID 128 -> 16 -> ReLU6 -> avg-pool 4/2 -> BN (moving statistics, trainable gamma and beta); everything behind
its output ``s7.bn`` is ``FineTuneRef``'s.  The L2 term runs over the 22 trained variables.

``conv7_ambiguity`` measures how much room conv 7's ReLU6 kinks leave in dW7.  A float32 kernel that sums in another order may put
a pre-activation within ``delta`` of 0 or 6 on the other side of the kink.  s7.bn is continuous in the pre-activation and no
gradient goes below stage 7, so such a flip reaches conv2d_7/kernel's gradient alone, by exactly |u[p, co]| |x6[p + k, ci]| at
element [ky, kx, ci, co], where u is the adjoint of relu6(pre) and does not depend on the mask."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from finetune_ref import FineTuneRef
from gradcam_ref import relu6
from roomnet_amd.graph import BN_EPSILON


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


class FineTune7Ref(FineTuneRef):
    """``FineTuneRef`` one stage further back: every method that took ``x7`` [N, S7, S7, 16] takes ``x6`` [N, S6, S6, 128]."""

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
        loss as the kernel carries it before its update divides by n.  u is the pool adjoint: it does not depend on the mask."""
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
