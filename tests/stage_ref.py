"""Stage-local and head-local float64 restatements (test infrastructure), built from the ops of oracle/roomnet_ref.py.

``stage_local`` computes ONE conv stage from a given input (and, for the residual stages, a given skip tensor): fed the
tensors a handle itself stored, it judges every stage on exact inputs and nothing compounds.  ``head_local`` does the same
for everything behind the last conv stage.  ``stage_local_emulated`` is the same stage with the roundings include/roomnet_hip.h
documents for 16-bit handles applied by NumPy casts: a reference-side number that says how much of an error is rounding."""
import numpy as np

from oracle import roomnet_ref as R

F64 = np.float64


def _colblock_plan_exists(out_side, wo_min, wo_max):
    """csrc/rn_stage.h, rn_colblock_plan: one to four column blocks of wo_min .. wo_max pooled columns each."""
    return any(-(-out_side // nb) <= wo_max and out_side // nb >= wo_min for nb in range(1, 5))


def fp16_pool_stages(graph, tuned=True):
    """Stages whose kernels pool fp16-rounded ReLU6 outputs on the matrix cores and keep their conv weights divided by 6
    (include/roomnet_hip.h): the pool 4 / stride 1 stages 1-3 always; the stride-2 stages 4 and 5 where the row-blocked kernels
    run -- rows that can be cut into column blocks of 194-206 (stage 4) / 66-110 (stage 5) input columns, restated here from
    rn_stage4x_supported / rn_stage5x_supported: at 224 both, at 240 stage 5 only.  The generic kernels (``tuned=False``) pool in
    float32.  On its row-blocked kernel stage 5 also rounds the lerp fraction of its horizontal interpolation, as stage 3 does."""
    if not tuned:
        return ()
    out = [1, 2, 3]
    s4, s5 = graph.stages[4], graph.stages[5]
    if s4.in_side >= 193 and _colblock_plan_exists(s4.out_side, 95, 101):
        out.append(4)
    if s5.in_side >= 66 and s5.in_side - 2 * s5.out_side <= 5 and _colblock_plan_exists(s5.out_side, 31, 53):
        out.append(5)
    return tuple(out)


def stage_out_name(stage):
    return "s%d.%s" % (stage.index, "bn2" if stage.residual else "bn")


def preprocess64(im_bgr_u8):
    """network.py:129 in float64 (no cast to float32): the exact value of stage 0's input."""
    return ((im_bgr_u8[..., [2, 1, 0]] / 255.) * 2) - 1


def _bn(weights, name):
    return tuple(np.asarray(weights["%s/%s" % (name, p)], F64) for p in ("gamma", "beta", "moving_mean", "moving_variance"))


def stage_local(graph, weights, k, x_in, x_skip=None, relu=R.relu6):
    """Conv stage ``k`` alone in float64: conv -> ReLU6 -> [pool] -> BN -> [+ resize(x_skip) -> BN2].  ``x_skip`` is the output
    of stage ``graph.stages[k].skip_stage`` (1, 4 and 7 for the residual stages 3, 5 and 9)."""
    s = graph.stages[k]
    out = relu(R.conv2d_valid(np.asarray(x_in, F64), np.asarray(weights[s.conv_name + "/kernel"], F64)))
    if s.pool_k:
        out = R.avg_pool_valid(out, s.pool_k, s.pool_s)
    out = R.fused_batch_norm_infer(out, *_bn(weights, s.bn_name))
    if s.residual:
        out = out + R.resize_bilinear_legacy(np.asarray(x_skip, F64), out.shape[1])
        out = R.fused_batch_norm_infer(out, *_bn(weights, s.bn2_name))
    return out


def head_local(graph, weights, s_last):
    """Flatten, the dense blocks, softmax and argmax in float64 from the last conv stage's output.  Returns a dict with every
    head node (``d0.mm`` ... ``d3.relu``), ``logits`` (= the last ``dK.relu``), ``probs`` (float64) and ``ids``."""
    out = np.asarray(s_last, F64).reshape(len(s_last), -1)
    res = {"flat": out}
    for d in graph.dense:
        out = out @ np.asarray(weights[d.name + "/kernel"], F64)
        if d.biased:
            out = out + np.asarray(weights[d.name + "/bias"], F64)
        res["d%d.mm" % d.index] = out
        out = R.relu6(out)
        res["d%d.relu" % d.index] = out
        if d.bn_name:
            out = R.batch_norm_2d(out, *_bn(weights, d.bn_name))
            res["d%d.bn" % d.index] = out
    res["logits"] = res["d%d.relu" % graph.dense[-1].index]
    res["probs"] = R.softmax(res["logits"])
    res["ids"] = np.argmax(res["probs"], axis=-1).astype(np.int64)
    return res


def head_local_f32(graph, weights, s_last):
    """``head_local`` in float32 arithmetic (the CPU restatement whose own deviation from float64 scales the head's bound)."""
    out = np.asarray(s_last, np.float32).reshape(len(s_last), -1)
    res = {}
    for d in graph.dense:
        out = out @ np.asarray(weights[d.name + "/kernel"], np.float32)
        if d.biased:
            out = out + np.asarray(weights[d.name + "/bias"], np.float32)
        out = R.relu6(out)
        res["d%d.relu" % d.index] = out
        if d.bn_name:
            out = R.batch_norm_2d(out, *(np.asarray(weights["%s/%s" % (d.bn_name, p)], np.float32)
                                         for p in ("gamma", "beta", "moving_mean", "moving_variance")))
    res["logits"] = out
    res["probs"] = R.softmax(out)
    return res


# ---- the 16-bit roundings of include/roomnet_hip.h, as NumPy casts ----------------------------------------------------------
def round_bf16(x):
    """Round to nearest even onto the bfloat16 grid (values far inside the float32 range)."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).astype(F64)


def round_f16(x):
    return np.asarray(x, F64).astype(np.float16).astype(F64)


def round_storage(x, dtype):
    return round_bf16(x) if dtype == "bf16" else round_f16(x)


def stage_local_emulated(graph, weights, k, x_in, x_skip=None, dtype="bf16", tuned=True, relu=R.relu6):
    """``stage_local`` with the documented 16-bit roundings, everything else float64:
      - the conv kernel of stages 1-9 rounded to nearest in the storage type (after the division by 6 where the stage pools fp16
        values; stage 0's folded weights are hi + lo pairs: not rounded);
      - where pooling is fp16: ReLU6 outputs rounded to fp16 (as clamp(x / 6, 0, 1)) and the vertical pair sums rounded to fp16;
      - stages 3 and 5: the horizontal lerp fraction rounded to 2^-8 (bf16) / 2^-11 (fp16);
      - the stage output rounded to the storage type.
    ``relu`` is the clamp, as in ``stage_local`` (a self-check of the tests swaps both).  ``tuned=False``: the generic kernels (RN_FLAG_GENERIC_KERNELS) -- float32 pooling and interpolation, weights and output rounded."""
    s = graph.stages[k]
    x = np.asarray(x_in, F64)
    w = np.asarray(weights[s.conv_name + "/kernel"], F64)
    fp16_stages = fp16_pool_stages(graph, tuned)
    fp16_pool = bool(s.pool_k) and k in fp16_stages
    if k > 0:
        w = round_storage(w / 6.0, dtype) * 6.0 if fp16_pool else round_storage(w, dtype)
    out = relu(R.conv2d_valid(x, w))
    if fp16_pool:
        out = round_f16(out / 6.0)
        assert s.pool_k == 4
        pairs = round_f16(out[:, 0:-1] + out[:, 1:])           # pairs[y] = rows y + (y + 1), an fp16 add
        n, h, wd, c = out.shape
        ho, wo = (h - 4) // s.pool_s + 1, (wd - 4) // s.pool_s + 1
        acc = np.zeros((n, ho, wo, c), F64)
        for ky in (0, 2):
            for kx in range(4):
                acc += pairs[:, ky:ky + (ho - 1) * s.pool_s + 1:s.pool_s, kx:kx + (wo - 1) * s.pool_s + 1:s.pool_s, :]
        out = acc * (6.0 / 16.0)
    elif s.pool_k:
        out = R.avg_pool_valid(out, s.pool_k, s.pool_s)
    out = R.fused_batch_norm_infer(out, *_bn(weights, s.bn_name))
    if s.residual:
        skip = np.asarray(x_skip, F64)
        side = out.shape[1]
        ylo, yhi, yl = R.resize_tables(skip.shape[1], side)
        xlo, xhi, xl = R.resize_tables(skip.shape[2], side)
        yl, xl = yl.astype(F64), xl.astype(F64)
        if k in fp16_stages:
            q = 2.0 ** (8 if dtype == "bf16" else 11)
            xl = np.round(xl * q) / q
        yl, xl = yl[None, :, None, None], xl[None, None, :, None]
        tl, tr = skip[:, ylo][:, :, xlo], skip[:, ylo][:, :, xhi]
        bl, br = skip[:, yhi][:, :, xlo], skip[:, yhi][:, :, xhi]
        top, bottom = tl + (tr - tl) * xl, bl + (br - bl) * xl
        out = out + (top + (bottom - top) * yl)
        out = R.fused_batch_norm_infer(out, *_bn(weights, s.bn2_name))
    return round_storage(out, dtype)


def rel_err(got, want):
    """max |got - want| relative to the abs-max of the float64 tensor ``want``."""
    want = np.asarray(want, F64)
    return float(np.abs(np.asarray(got, F64) - want).max() / max(float(np.abs(want).max()), 1e-6))
