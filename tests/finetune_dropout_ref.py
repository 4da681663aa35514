"""CPU reference of fine-tuning with dropout (rn_ft_set_dropout): ``FineTuneRef`` and ``FineTune7Ref`` with GIVEN masks applied
at sites 1 and 2 + d of include/roomnet_hip.h, in the kernel's order -- hidden dense blocks: the ``mask * scale`` factor sits behind
the BN; the last block: behind its ReLU6, so that the softmax and the CE term read the dropped logits.  Site 0 (depth 3) is not
applied here: the test forms the dropped ``s6.bn`` itself in float32 NumPy (``dropped_x6``) and hands it in as the input.

The masks come from the product's host statement of the stream, ``finetune.dropout_keep`` (``host_masks``), which
tests/test_dropout_host.py pins to the published Philox vectors and the GPU test compares with the device's masks byte for byte."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from finetune7_ref import FineTune7Ref
from finetune_ref import DECAY_RATE, FineTuneRef
from gradcam_ref import relu6
from roomnet_amd import finetune


def host_masks(graph, depth, seed, step, n_slots, rate):
    """``{site: bool [n_slots, size]}`` for every site of a trainer of ``depth`` at global step ``step``."""
    return {site: np.stack([finetune.dropout_keep(seed, step, b, site, size, rate) for b in range(n_slots)])
            for site, (_name, size) in finetune.dropout_sites(graph, depth).items()}


def dropped_x6(x6, keep, rate):
    """Site 0 as the pre-pass forms it: ``x6 * scale`` as one float32 product where kept, +0 where dropped.  ``x6`` [n, S6, S6, 128]
    float32 (already gathered in slot order), ``keep`` bool [n, S6 * S6 * 128]."""
    x6 = np.asarray(x6, np.float32)
    return np.where(keep.reshape(x6.shape), x6 * finetune.dropout_scale(rate), np.float32(0.0)).astype(np.float32)


class _DropHead:
    """The part behind ``s7.bn`` with masks: ``set_masks`` before every forward pass whose batch they belong to."""
    masks = None
    scale = 1.0

    def set_masks(self, masks, rate):
        self.scale = float(finetune.dropout_scale(rate))          # the float32 value, exactly
        self.masks = {site: self._t(np.asarray(m, np.float64)) * self.scale for site, m in masks.items()}

    def _head(self, x7, P):
        g = self.graph
        x7 = self._t(x7) if not torch.is_tensor(x7) else x7
        s8 = self._stage(x7, g.stages[-2], P)
        b9 = self._stage(s8, g.stages[-1], P)
        s9 = self._bn(b9 + self._resize(x7), g.stages[-1].bn2_name, P)
        x = s9.reshape(s9.shape[0], -1) * self.masks[1]
        for i, d in enumerate(g.dense):
            z = x @ P[d.name + "/kernel"]
            if d.biased:
                z = z + P[d.name + "/bias"]
            x = relu6(z)
            if d.bn_name:
                x = self._bn(x, d.bn_name, P)
            x = x * self.masks[2 + i]
        return x


class FineTuneDropRef(_DropHead, FineTuneRef):
    def logits(self, x7, P=None):
        return self._head(x7, P or self.params)

    def train_dropout(self, feats, labels, index, learn_rate, num_steps, l2, seed, rate, start_step=0):
        """``FineTuneRef.train`` with each step's masks: slot b of step s drops by ``dropout_keep(seed, start_step + s, b, ...)``."""
        feats = self._t(feats)
        labels = np.asarray(labels)
        losses = []
        for s, idx in enumerate(np.asarray(index)):
            self.set_masks(host_masks(self.graph, 2, seed, start_step + s, len(idx), rate), rate)
            lr = learn_rate * DECAY_RATE ** ((start_step + s) / num_steps)
            losses.append(self.step(feats[idx], labels[idx], l2, lr))
        return np.asarray(losses, np.float64)


class FineTune7DropRef(_DropHead, FineTune7Ref):
    """Takes the DROPPED ``x6`` (``dropped_x6``)."""

    def logits(self, x6, P=None):
        P = P or self.params
        return self._head(self.x7(x6, P), P)

    def conv7_adjoint(self, x6, y):
        # (FineTune7Ref.conv7_adjoint with the masked head behind s7.bn)
        with torch.no_grad():
            pre = self.pre7(self._t(x6))
        act = relu6(pre).detach().requires_grad_(True)
        r = self._head(self.x7_from_act(act), self.params)
        L = F.cross_entropy(r, torch.as_tensor(np.asarray(y, np.int64)), reduction="sum")
        (u,) = torch.autograd.grad(L, act)
        return pre, u
