"""CPU reference of the batch-statistics forward pass (RN_FLAG_BATCH_STATS, include/roomnet_hip.h): the graph restated in torch
with the moments of the batch at every BN -- tf.layers.batch_normalization(training=True), network.py:193, :202, :217 -- in
float64.  The same code run in float32 is the noise floor the GPU tests scale their tolerance with.

``moments`` replaces the batch moments of every BN by given ones (``"moving"``: the checkpoint's moving statistics, which makes
this the inference graph -- the self-check against tests/golden/parity_224.npz; or a dict ``{bn: (mean, var_biased, ...)}``).

``update`` restates the reference's update ops (network.py:64-67) on the returned moments in plain Python floats / NumPy scalars,
independently of roomnet_amd.bnstats.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from oracle import roomnet_ref as R
from roomnet_amd.graph import BN_EPSILON, build_graph


def forward(weights, im_bgr_u8, dtype=torch.float64, moments=None, num_classes=6):
    """dict: ``bn`` {node name: NHWC array}, ``logits`` (d3.relu), ``raw`` (d3.mm), ``stats`` {bn prefix: (mean, var_biased,
    count)}, ``in_absmax`` {bn prefix: abs-max of the BN's input}, ``bn_nodes`` [(bn prefix, node name)] in variable order."""
    im = np.asarray(im_bgr_u8)
    g = build_graph(num_classes, im.shape[1])
    x = torch.from_numpy(R.preprocess_batch(im)).permute(0, 3, 1, 2).contiguous().to(dtype)
    w = {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(dtype) for k, v in weights.items()}
    out = {"bn": {}, "stats": {}, "in_absmax": {}, "bn_nodes": []}

    def bn(t, name, node):
        rank4 = t.dim() == 4
        dims, shape = ((0, 2, 3), (1, -1, 1, 1)) if rank4 else ((0,), (1, -1))
        if moments is None:
            m = t.mean(dims)
            v = ((t - m.view(shape)) ** 2).mean(dims)
        elif isinstance(moments, str):
            m, v = w[name + "/moving_mean"], w[name + "/moving_variance"]
        else:
            m = torch.from_numpy(np.asarray(moments[name][0])).to(dtype)
            v = torch.from_numpy(np.asarray(moments[name][1])).to(dtype)
        count = t.numel() // t.shape[1]
        out["stats"][name] = (m.double().numpy().copy(), v.double().numpy().copy(), int(count))
        out["in_absmax"][name] = float(t.abs().max())
        out["bn_nodes"].append((name, node))
        inv = (1.0 / torch.sqrt(v + BN_EPSILON)) * w[name + "/gamma"]
        beta = w[name + "/beta"]
        if rank4:
            y = (t - m.view(shape)) * inv.view(shape) + beta.view(shape)            # FusedBatchNorm
            out["bn"][node] = y.permute(0, 2, 3, 1).double().numpy()
        else:
            y = t * inv + (beta - m * inv)                                         # tf.nn.batch_normalization
            out["bn"][node] = y.double().numpy()
        return y

    def resize(t, side):
        _, _, h, wd = t.shape
        ylo, yhi, yl = R.resize_tables(h, side)
        xlo, xhi, xl = R.resize_tables(wd, side)
        yl = torch.from_numpy(yl).to(dtype).view(1, 1, -1, 1)
        xl = torch.from_numpy(xl).to(dtype).view(1, 1, 1, -1)
        r0, r1 = t[:, :, torch.from_numpy(ylo)], t[:, :, torch.from_numpy(yhi)]
        a, b = torch.from_numpy(xlo), torch.from_numpy(xhi)
        top = r0[..., a] + (r0[..., b] - r0[..., a]) * xl
        bot = r1[..., a] + (r1[..., b] - r1[..., a]) * xl
        return top + (bot - top) * yl

    t, outs = x, []
    with torch.no_grad():
        for s in g.stages:
            kern = w[s.conv_name + "/kernel"].permute(3, 2, 0, 1).contiguous()
            t = torch.clamp(F.conv2d(t, kern), 0.0, 6.0)
            if s.pool_k:
                t = F.avg_pool2d(t, s.pool_k, s.pool_s)
            t = bn(t, s.bn_name, "s%d.bn" % s.index)
            outs.append(t)
            if s.residual:
                t = bn(t + resize(outs[s.skip_stage], s.out_side), s.bn2_name, "s%d.bn2" % s.index)
        t = t.permute(0, 2, 3, 1).reshape(t.shape[0], -1)
        for d in g.dense:
            t = t @ w[d.name + "/kernel"]
            if d.biased:
                t = t + w[d.name + "/bias"]
            raw = t
            t = torch.clamp(t, 0.0, 6.0)
            if d.bn_name:
                t = bn(t, d.bn_name, "d%d.bn" % d.index)
    out["raw"] = raw.double().numpy()
    out["logits"] = t.double().numpy()
    return out


def update(moving, value, momentum):
    """assign_moving_average, element by element with NumPy float32 scalars: moving - (moving - value) * float32(1 - momentum)."""
    decay = np.float32(1.0 - momentum)
    return np.array([np.float32(np.float32(m) - np.float32(np.float32(np.float32(m) - np.float32(v)) * decay))
                     for m, v in zip(np.asarray(moving).ravel(), np.asarray(value).ravel())], np.float32)


def update_variance(var_biased, count, dense):
    """The variance the update sees: the biased one behind tf.nn.moments (dense BNs), the fused kernel's Bessel-corrected
    one, var * (float32(N) / float32(N - 1)), on the conv side."""
    v = np.asarray(var_biased, np.float32)
    if dense:
        return v
    adjust = np.float32(count) / np.float32(count - 1 if count > 1 else 1)
    return np.array([np.float32(x * adjust) for x in v], np.float32)
