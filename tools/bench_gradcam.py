"""Grad-CAM cost against the forward pass on the same handle: one JSON line with ms per rn_grad_cam_u8_device call and ms per
rn_forward_u8_device call (device buffers, the caller's stream, CUDA events) for three cases -- batch 256 at 224 x 224 bf16,
batch 1 at 224 bf16, batch 64 at 600 x 600 fp16 -- at layer s6.bn (the default) and s7.bn.

    python tools/bench_gradcam.py [--steps 20] [--warmup 5]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _time(fn, steps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def case(weights, side, dtype, batch, steps, warmup):
    import torch
    from roomnet_amd import _capi
    from roomnet_amd.graph import build_graph
    from roomnet_amd.synth import parity_set
    w = dict(weights)
    if side != 224:
        rng = np.random.default_rng(600)                       # the 600 x 600 variant's seeded first dense kernel
        w["dense/kernel"] = rng.uniform(-0.04, 0.04, (3136, 32)).astype(np.float32)
    fields = np.load(os.path.join(ROOT, "tests", "golden", "class_fields.npz"))["fields_u8"]
    ims = parity_set(side, fields)
    ims = np.concatenate([ims] * (batch // len(ims) + 1))[:batch]
    eng = _capi.Engine(build_graph(6, side), w, device=0, dtype=dtype, max_batch=batch)
    try:
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        d_in = torch.from_numpy(np.ascontiguousarray(ims)).cuda()
        s6 = eng.nodes()["s6.bn"][1]
        d_cam = torch.empty((batch, s6[0], s6[1]), dtype=torch.float32, device="cuda")
        d_probs = torch.empty((batch, 6), dtype=torch.float32, device="cuda")
        d_ids = torch.empty((batch,), dtype=torch.int64, device="cuda")
        fwd = _time(lambda: eng.forward_u8_device(d_in.data_ptr(), batch, d_probs.data_ptr(), d_ids.data_ptr()), steps, warmup)
        out = {"side": side, "dtype": dtype, "batch": batch, "forward_ms": round(fwd, 4)}
        for layer in ("s6.bn", "s7.bn"):
            gc = _time(lambda: eng.grad_cam_u8_device(d_in.data_ptr(), batch, None, layer, d_cam.data_ptr(), None, d_probs.data_ptr(),
                                                      d_ids.data_ptr()), steps, warmup)
            out["grad_cam_%s_ms" % layer] = round(gc, 4)
            out["ratio_%s" % layer] = round(gc / fwd, 3)
        eng.set_stream(None)
        return out
    finally:
        eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    from roomnet_amd.tf_bundle import BundleReader
    weights = BundleReader(os.path.join(ROOT, "roomnet_amd", "final_model", "roomnet")).load_all()
    cases = [case(weights, 224, "bf16", 256, args.steps, args.warmup),
             case(weights, 224, "bf16", 1, args.steps, args.warmup),
             case(weights, 600, "f16", 64, args.steps, args.warmup)]
    print(json.dumps({"what": "ms per grad-CAM call vs ms per forward call on the same handle (device buffers)",
                      "target": "batch 256, 224, bf16: grad-CAM <= 1.3 x forward", "cases": cases}))


if __name__ == "__main__":
    main()
