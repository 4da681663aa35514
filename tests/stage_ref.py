"""Stage-local and head-local float64 restatements (test infrastructure), built from the ops of oracle/roomnet_ref.py.

``stage_local`` computes ONE conv stage from a given input (and, for the residual stages, a given skip tensor): fed the
tensors a handle itself stored, it judges every stage on exact inputs and nothing compounds.  ``head_local`` does the same
for everything behind the last conv stage.  ``stage_local_emulated`` is the same stage with the roundings include/roomnet_hip.h
documents for 16-bit handles applied by NumPy casts: a reference-side number that says how much of an error is rounding.
``check_stage_local``, ``_check_nodes`` and ``check_head_local`` at the end are the checks the GPU test files share (a test module imports from here, never
from another test module)."""
import numpy as np

import block_plans as BP
from oracle import roomnet_ref as R
from parity_bounds import MARGIN, STAGE_TOL, TIE_EDGE, _tol

F64 = np.float64


def fp16_pool_stages(graph, tuned=True):
    """Stages whose kernels pool fp16-rounded ReLU6 outputs on the matrix cores and keep their conv weights divided by 6
    (include/roomnet_hip.h): the pool 4 / stride 1 stages 1-3 always; the stride-2 stages 4 and 5 where the row-blocked kernels
    run -- rows that can be cut into column blocks of 194-206 (stage 4) / 66-110 (stage 5) input columns, restated here from
    rn_stage4x_supported / rn_stage5x_supported: at 224 both, at 240 stage 5 only.  The generic kernels (``tuned=False``) pool in
    float32.  On its row-blocked kernel stage 5 also rounds the lerp fraction of its horizontal interpolation, as stage 3 does.
    The plans themselves are restated in tests/block_plans.py."""
    if not tuned:
        return ()
    return (1, 2, 3) + tuple(k for k in (4, 5) if BP.stage_plan(graph, k))


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


# ---- the checks tests/test_hip_other_checkpoints.py and tests/test_hip_seams_live.py share ----------------------------------
NOTHING_FOLDED = {"pair_channels_not_convolved": 0, "pair_channels_proven_frozen": 0, "residual_stage_folded": -1,
                  "residual_stage_live_quarters": 4}
STAGE_OUT = ["s0.bn", "s1.bn", "s2.bn", "s3.bn2", "s4.bn", "s5.bn2", "s6.bn", "s7.bn", "s8.bn", "s9.bn2"]
SECTION = "other_checkpoints"       # the parity report's section of both files


def _locate(got, want):
    """Where a tensor is wrong: the worst element, its values, whether it sits at a clamp end, the three worst channels."""
    d = np.abs(np.asarray(got, np.float64) - want)
    i = np.unravel_index(int(d.argmax()), d.shape)
    per_c = d.reshape(-1, d.shape[-1]).max(0)
    worst_c = np.argsort(per_c)[::-1][:3]
    return {"at [n, y, x, c]": [int(v) for v in i], "got": float(np.asarray(got)[i]), "want": float(want[i]),
            "want_negative": bool(want[i] < 0), "worst_channels": {int(c): float(per_c[c]) for c in worst_c},
            "elements_above_half_of_worst": int((d > 0.5 * d.max()).sum())}


def check_stage_local(eng, w, ims, dtype, record=None, key="", tuned=True, lazy_emulation=False):
    """Every stage of a handle that materialises all ten stage outputs, judged on the handle's own stored inputs: stage k's
    stored output against ``stage_local`` of the stored output of stage k - 1 (and skip tensor).  Bound per tensor:
    max(STAGE_TOL, 2 x the error of ``stage_local_emulated``).  ``lazy_emulation``: the emulation (as costly as the reference
    itself) is computed only for a stage whose error exceeds STAGE_TOL -- the bound is the same, a passing stage's row then
    carries no emulated error."""
    g, n = eng.graph, len(ims)
    eng.forward_u8(ims)
    taps = [eng.tap(stage_out_name(s), n).astype(np.float64) for s in g.stages]
    rows, bad = {}, []
    for k, s in enumerate(g.stages):
        x_in = preprocess64(ims) if k == 0 else taps[k - 1]
        skip = taps[s.skip_stage] if s.residual else None
        want = stage_local(g, w, k, x_in, skip)
        assert taps[k].shape == want.shape, k
        err = rel_err(taps[k], want)
        bound, emu = STAGE_TOL[dtype], None
        if not (lazy_emulation and err <= bound):
            emu = rel_err(stage_local_emulated(g, w, k, x_in, skip, dtype, tuned=tuned), want)
            bound = max(STAGE_TOL[dtype], 2.0 * emu)
        rows[stage_out_name(s)] = {"rel_err": err, "emulated_rel_err": emu, "bound": bound}
        print("%s %-7s stage-local %.3e   emulated %s   bound %.3e" % (dtype, stage_out_name(s), err,
                                                                      "not needed" if emu is None else "%.3e" % emu, bound))
        if not err <= bound:
            bad.append((stage_out_name(s), err, bound, _locate(taps[k], want)))
    if record:
        record(SECTION, key, rows)
    assert not bad, bad
    return rows


def _check_nodes(eng, names, n, r64, r32, record, key):
    """Float32 handles: the named nodes against the float64 oracle run ``r64``, tolerance _tol with the float32 C oracle run ``r32``."""
    rows, bad = {}, []
    for name in names:
        want = np.asarray(r64["taps"][name], np.float64)
        got = eng.tap(name, n)
        assert got.shape == want.shape, name
        err, tol = float(np.abs(got - want).max()), _tol(want, r32["taps"][name])
        rows[name] = {"err": err, "tol": tol}
        if not err <= tol:
            bad.append((name, err, tol))
    print(key, " ".join("%s=%.2g/%.2g" % (k, v["err"], v["tol"]) for k, v in rows.items()))
    record(SECTION, key, rows)
    assert not bad, bad


def check_head_local(eng, w, n, ids, probs, record=None, key=""):
    """The float32 head (dense chain, softmax, argmax) of any handle against float64 computed from the handle's own s9.bn2."""
    g = eng.graph
    nc = g.num_classes
    s9 = eng.tap("s9.bn2", n)
    h64, h32 = head_local(g, w, s9), head_local_f32(g, w, s9)
    logits = eng.tap("d3.relu", n)
    assert logits.shape == (n, nc) and probs.shape == (n, nc) and ids.shape == (n,)
    el, tl = float(np.abs(logits - h64["logits"]).max()), _tol(h64["logits"], h32["logits"])
    ep, tp = float(np.abs(probs - h64["probs"]).max()), _tol(h64["probs"], h32["probs"])
    # ids: the float64 winner where its margin over the runner-up is clear; an exact float64 tie for the first place (ReLU6 makes
    # exact 0.0 and 6.0 common) must resolve to the lowest index, where the tie is not an accident of a pre-activation that
    # float32 may put on the other side of the clamp's end
    lg, mm = h64["logits"], h64["d%d.mm" % g.dense[-1].index]
    checked = ties = 0
    wrong = []
    for i in range(n):
        tied = np.flatnonzero(lg[i] == lg[i].max())
        rest = np.delete(lg[i], tied)
        clear = rest.size == 0 or lg[i].max() - rest.max() > MARGIN
        solid = len(tied) == 1 or bool((np.minimum(np.abs(mm[i][tied]), np.abs(mm[i][tied] - 6.0)) > TIE_EDGE).all())
        if clear and solid:
            checked += 1
            ties += len(tied) > 1
            if ids[i] != tied[0]:
                wrong.append((i, int(ids[i]), tied.tolist()))
    psum = float(np.abs(probs.sum(1) - 1.0).max())
    row = {"logits_err": el, "logits_tol": tl, "probs_err": ep, "probs_tol": tp, "ids_checked": checked, "of": n,
           "exact_fp64_ties_checked": int(ties), "max_abs_probs_sum_minus_1": psum}
    print("head nc=%d n=%d  logits %.3g / %.3g  probs %.3g / %.3g  ids checked %d (ties %d)  |sum - 1| %.2g" % (
        nc, n, el, tl, ep, tp, checked, ties, psum))
    if record:
        record(SECTION, key, row)
    assert el <= tl and ep <= tp, row
    assert not wrong, wrong
    assert psum <= 1e-5
    # whatever the margins (at 64 classes none of these images has a clear one): the id is the first maximum of the handle's own probs
    np.testing.assert_array_equal(ids, [int(np.flatnonzero(p == p.max())[0]) for p in probs])
    if nc == 1:
        np.testing.assert_array_equal(probs, np.float32(1.0))
        np.testing.assert_array_equal(ids, 0)
    return row
