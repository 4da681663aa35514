"""Cost of batch-statistics BN (RN_FLAG_BATCH_STATS) on the float32 per-node path.

    python tools/bench_bnstats.py [--steps 10] [--warmup 3] [--out profiles/bn_batchstats_timing.json]
        ms per batch-statistics forward and ms per forward of a plain RN_FLAG_TAPS float32 handle (the same launches minus the
        moments) on the same batch, batch 64 and 256 at 224 x 224 (device buffers, the caller's stream, events); one JSON line.

    rocprofv3 --kernel-trace --stats -d DIR -o kt --output-format csv -- python tools/bench_bnstats.py --trace-run [--reps 4]
        the program of the kernel trace (its own run): --reps batch-statistics forwards at batch 64, then at batch 256.

    python tools/bench_bnstats.py --summarise DIR/.../kt_kernel_trace.csv [--reps 4] [--out profiles/bn_batchstats_kernel_stats.txt]
        per BN node: the moments launch (and the finalise launch) next to the bn_f32_kernel launch on the same tensor, median
        over the repetitions but the first.  Yardstick for s0.bn ... s6.bn: moments <= 1.25 x bn_f32_kernel (that kernel
        reads and writes the tensor once each; the one-pass reduction reads it once).
"""
import argparse
import csv
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BATCHES = (64, 256)
CONV_BN_NODES = ["s0.bn", "s1.bn", "s2.bn", "s3.bn", "s3.bn2", "s4.bn", "s5.bn", "s5.bn2", "s6.bn", "s7.bn", "s8.bn", "s9.bn", "s9.bn2"]
YARDSTICK_NODES = ["s0.bn", "s1.bn", "s2.bn", "s3.bn", "s3.bn2", "s4.bn", "s5.bn", "s5.bn2", "s6.bn"]
YARDSTICK = 1.25


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


def _setup(batch):
    from roomnet_amd.synth import parity_set
    from roomnet_amd.tf_bundle import BundleReader
    weights = BundleReader(os.path.join(ROOT, "roomnet_amd", "final_model", "roomnet")).load_all()
    fields = np.load(os.path.join(ROOT, "tests", "golden", "class_fields.npz"))["fields_u8"]
    ims = parity_set(224, fields)
    return weights, np.concatenate([ims] * (batch // len(ims) + 1))[:batch]


def _forward_fn(eng, ims):
    import torch
    batch = len(ims)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    d_in = torch.from_numpy(np.ascontiguousarray(ims)).cuda()
    d_probs = torch.empty((batch, 6), dtype=torch.float32, device="cuda")
    d_ids = torch.empty((batch,), dtype=torch.int64, device="cuda")
    keep = (d_in, d_probs, d_ids)
    return lambda: eng.forward_u8_device(d_in.data_ptr(), batch, d_probs.data_ptr(), d_ids.data_ptr()), keep


def timing(steps, warmup):
    from roomnet_amd import _capi
    from roomnet_amd.graph import build_graph
    cases = []
    for batch in BATCHES:
        weights, ims = _setup(batch)
        row = {"side": 224, "dtype": "f32", "batch": batch}
        for key, kw in (("batch_stats_forward_ms", dict(batch_stats=True)), ("plain_taps_forward_ms", dict(taps=True))):
            eng = _capi.Engine(build_graph(6, 224), weights, device=0, dtype="f32", max_batch=batch, **kw)
            try:
                fn, keep = _forward_fn(eng, ims)
                row[key] = round(_time(fn, steps, warmup), 4)
                eng.set_stream(None)
            finally:
                eng.close()
        row["ratio"] = round(row["batch_stats_forward_ms"] / row["plain_taps_forward_ms"], 4)
        cases.append(row)
    return {"what": "ms per batch-statistics forward (RN_FLAG_BATCH_STATS) vs ms per forward of a plain RN_FLAG_TAPS float32 handle "
                    "on the same batch (device buffers): the same per-node launches minus the moments", "steps": steps, "cases": cases}


def trace_run(reps):
    import torch
    from roomnet_amd import _capi
    from roomnet_amd.graph import build_graph
    for batch in BATCHES:
        weights, ims = _setup(batch)
        eng = _capi.Engine(build_graph(6, 224), weights, device=0, dtype="f32", max_batch=batch, batch_stats=True)
        try:
            fn, keep = _forward_fn(eng, ims)
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            eng.set_stream(None)
        finally:
            eng.close()


def summarise(trace_csv, reps):
    rows = []
    for r in csv.DictReader(open(trace_csv)):
        name = r["Kernel_Name"]
        for key in ("bn_moments_kernel", "bn_finalise_kernel", "bn_f32_kernel"):
            if key in name:
                rows.append((int(r["Start_Timestamp"]), key, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    rows.sort()
    triples, cur = [], {}
    for _t, key, us in rows:
        if key == "bn_moments_kernel":
            cur = {key: us}
        elif cur:
            cur[key] = us
            if key == "bn_f32_kernel":
                triples.append(cur)
                cur = {}
    per = len(CONV_BN_NODES)
    if len(triples) != per * reps * len(BATCHES):
        raise SystemExit("expected %d moments/finalise/bn launch triples (%d nodes x %d reps x %d batches), found %d"
                         % (per * reps * len(BATCHES), per, reps, len(BATCHES), len(triples)))
    lines = ["# rocprofv3 --kernel-trace --stats -- python tools/bench_bnstats.py --trace-run --reps %d (one MI355X, its own run)" % reps,
             "# per BN node of a batch-statistics forward at 224 x 224 float32: median us over the repetitions but the first",
             "# yardstick (s0.bn ... s6.bn): bn_moments_kernel <= %.2f x bn_f32_kernel on the same tensor" % YARDSTICK,
             "%5s  %-7s %12s %12s %12s %9s  %s" % ("batch", "node", "moments_us", "finalise_us", "bn_f32_us", "mom/bn", "yardstick")]
    missed = []
    for bi, batch in enumerate(BATCHES):
        for ni, node in enumerate(CONV_BN_NODES):
            ts = [triples[(bi * reps + rep) * per + ni] for rep in range(1 if reps > 1 else 0, reps)]
            mom, fin, bn = (statistics.median(t[k] for t in ts) for k in ("bn_moments_kernel", "bn_finalise_kernel", "bn_f32_kernel"))
            verdict = ""
            if node in YARDSTICK_NODES:
                verdict = "ok" if mom <= YARDSTICK * bn else "MISSED"
                if verdict == "MISSED":
                    missed.append((batch, node))
            lines.append("%5d  %-7s %12.1f %12.1f %12.1f %9.3f  %s" % (batch, node, mom, fin, bn, mom / bn, verdict))
    lines.append("# nodes over the yardstick: %s" % (missed or "none"))
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--summarise", metavar="KERNEL_TRACE_CSV")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.trace_run:
        trace_run(args.reps)
        return
    if args.summarise:
        text = summarise(args.summarise, args.reps)
        out = args.out or os.path.join(ROOT, "profiles", "bn_batchstats_kernel_stats.txt")
    else:
        text = json.dumps(timing(args.steps, args.warmup)) + "\n"
        out = args.out or os.path.join(ROOT, "profiles", "bn_batchstats_timing.json")
    with open(out, "w") as f:
        f.write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
