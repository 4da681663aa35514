"""CPU reference of the grad-CAM maps (rn_grad_cam_*, include/roomnet_hip.h): stages 7-9 and the dense head restated in
torch float64 from a stored ``s6.bn`` / ``s7.bn``, with autograd for G = dS/dA.

S = z[c] with z the last dense layer's pre-ReLU6 output (node ``d3.mm``).  ReLU6 passes gradient where 0 < x < 6 only
(TensorFlow's Relu6Grad), which torch.clamp does not do at the ends: ``relu6`` below is written so that it does.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from roomnet_amd.graph import BN_EPSILON, build_graph


def _t(x):
    return torch.as_tensor(np.asarray(x, np.float64))


def relu6(x):
    inside = (x > 0) & (x < 6)
    return torch.where(inside, x, torch.where(x >= 6, torch.full_like(x, 6.0), torch.zeros_like(x)).detach())


def _resize_tables(in_size, out_size):
    scale = np.float32(in_size) / np.float32(out_size)
    src = (np.arange(out_size, dtype=np.float32) * scale).astype(np.float32)
    lo = src.astype(np.int64)
    hi = np.minimum(lo + 1, in_size - 1)
    return lo, hi, (src - lo.astype(np.float32)).astype(np.float32)


class GradCamRef:
    """Stages ns-3 .. ns-1 (s7, s8, s9) and the head of a checkpoint ``weights`` for ``build_graph(num_classes, im_side)``."""

    def __init__(self, weights, num_classes=6, im_side=224):
        g = build_graph(num_classes, im_side)
        self.graph = g
        st = g.stages
        self.st7, self.st8, self.st9 = st[-3], st[-2], st[-1]

        def bn(name):
            gamma, beta = _t(weights[name + "/gamma"]), _t(weights[name + "/beta"])
            mean, var = _t(weights[name + "/moving_mean"]), _t(weights[name + "/moving_variance"])
            return mean, gamma / torch.sqrt(var + BN_EPSILON), beta

        self.w = {s.index: _t(weights[s.conv_name + "/kernel"]).permute(3, 2, 0, 1).contiguous() for s in st[-3:]}   # OIHW
        self.w7_hwio = _t(weights[self.st7.conv_name + "/kernel"])
        self.bn = {s.index: bn(s.bn_name) for s in st[-3:]}
        self.bn2 = bn(self.st9.bn2_name)
        self.rt = _resize_tables(self.st7.out_side, self.st9.out_side)
        self.dense = []
        for d in g.dense:
            k = _t(weights[d.name + "/kernel"])
            b = _t(weights[d.name + "/bias"]) if d.biased else None
            if d.bn_name:
                mean, inv, beta = bn(d.bn_name)
                aff = (inv, beta - mean * inv)
            else:
                aff = None
            self.dense.append((k, b, aff))

    # ---- forward pieces (NHWC float64 tensors)
    def _stage(self, x, idx, taps=None, name=""):
        xc = x.permute(0, 3, 1, 2)
        c = F.conv2d(xc, self.w[idx])
        if taps is not None:
            taps[name + ".pre"] = c.permute(0, 2, 3, 1)
        p = F.avg_pool2d(relu6(c), 4, 2)
        mean, inv, beta = self.bn[idx]
        y = (p.permute(0, 2, 3, 1) - mean) * inv + beta
        return y

    def s7_from_s6(self, s6, taps=None):
        return self._stage(s6, self.st7.index, taps, "s7")

    def _resize(self, x):
        lo, hi, lerp = self.rt
        yl = _t(lerp)[None, :, None, None]
        xl = _t(lerp)[None, None, :, None]
        tl, tr = x[:, lo][:, :, lo], x[:, lo][:, :, hi]
        bl, br = x[:, hi][:, :, lo], x[:, hi][:, :, hi]
        top = tl + (tr - tl) * xl
        bot = bl + (br - bl) * xl
        return top + (bot - top) * yl

    def logits_from_s7(self, s7, taps=None):
        """z = d{last}.mm [N, C]; ``taps`` (dict) collects s8.bn, s9.bn2, d*.mm and every ReLU6 pre-activation."""
        s8 = self._stage(s7, self.st8.index, taps, "s8")
        b9 = self._stage(s8, self.st9.index, taps, "s9")
        mean, inv, beta = self.bn2
        s9 = ((b9 + self._resize(s7)) - mean) * inv + beta
        if taps is not None:
            taps["s8.bn"] = s8
            taps["s9.bn2"] = s9
        x = s9.reshape(s9.shape[0], -1)
        for d, (k, b, aff) in enumerate(self.dense):
            z = x @ k
            if b is not None:
                z = z + b
            if taps is not None:
                taps["d%d.mm" % d] = z
            if d + 1 == len(self.dense):
                return z
            x = relu6(z)
            if aff is not None:
                x = x * aff[0] + aff[1]

    @staticmethod
    def argmax(z):
        r = relu6(z)
        return torch.argmax(torch.softmax(r, dim=-1), dim=-1)

    # ---- gradients
    def grad_s7(self, s7, cls):
        s7 = _t(s7).clone().requires_grad_(True)
        z = self.logits_from_s7(s7)
        S = z.gather(1, torch.as_tensor(np.asarray(cls, np.int64))[:, None]).sum()
        (g,) = torch.autograd.grad(S, s7)
        return g.detach(), z.detach()

    def grad_s6(self, s6, cls, s7=None):
        """dS/ds6.bn.  With ``s7`` (a handle's stored s7.bn) the head is linearised at THAT tensor and only the stage-7 masks
        come from ``s6``; without it s7.bn is recomputed from s6.bn in float64."""
        s6 = _t(s6).clone().requires_grad_(True)
        s7r = self.s7_from_s6(s6)
        if s7 is None:
            z = self.logits_from_s7(s7r)
            S = z.gather(1, torch.as_tensor(np.asarray(cls, np.int64))[:, None]).sum()
            (g,) = torch.autograd.grad(S, s6)
            return g.detach(), z.detach()
        g7, z = self.grad_s7(s7, cls)
        (g,) = torch.autograd.grad(s7r, s6, grad_outputs=g7)
        return g.detach(), z

    def alpha6_identity(self, s6, g7):
        """alpha6 through Gamma[co] = sum_p dS/dconv7[p, co] and the tap sums of W7 (the kernel's reduced form)."""
        s6 = _t(s6)
        taps = {}
        self.s7_from_s6(s6, taps)
        pre = taps["s7.pre"]                                   # [N, C7, C7, 16]
        mean, inv, beta = self.bn[self.st7.index]
        gp = (_t(g7) * inv).permute(0, 3, 1, 2)                # dS/d pool7
        pre_c = pre.permute(0, 3, 1, 2).clone().requires_grad_(True)
        pooled = F.avg_pool2d(pre_c, 4, 2)
        (gpool,) = torch.autograd.grad(pooled, pre_c, grad_outputs=gp)
        mask = ((pre_c > 0) & (pre_c < 6)).to(torch.float64)
        gamma = (gpool * mask).sum(dim=(2, 3))                 # [N, 16]
        wsum = self.w7_hwio.sum(dim=(0, 1))                    # [128, 16]
        s = s6.shape[1]
        return (gamma @ wsum.T) / float(s * s)

    def grad_cam(self, s6=None, s7=None, cls=None, layer="s6.bn"):
        """dict(cam [N,h,w], alpha [N,c], G, z, cls) in float64 numpy."""
        if s7 is None:
            s7t = self.s7_from_s6(_t(s6))
        else:
            s7t = _t(s7)
        if cls is None:
            cls = self.argmax(self.logits_from_s7(s7t)).numpy()
        if layer == "s7.bn":
            G, z = self.grad_s7(s7t, cls)
            A = s7t
        elif layer == "s6.bn":
            G, z = self.grad_s6(s6, cls, s7)
            A = _t(s6)
        else:
            raise ValueError(layer)
        alpha = G.mean(dim=(1, 2))
        cam = torch.clamp(torch.einsum("nyxc,nc->nyx", A, alpha), min=0)
        return {"cam": cam.numpy(), "alpha": alpha.numpy(), "G": G.numpy(), "z": z.numpy(), "cls": np.asarray(cls)}
