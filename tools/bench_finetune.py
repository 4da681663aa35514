"""Fine-tuning cost (rn_ft_*, rn_features_*): one JSON line with
  - us per Adam step at batch 45 and 256 (224 geometry) and batch 45 at the 600 geometry: 200 steps per rn_ft_run, device time of the
    step loop between events on the trainer's stream (rn_ft_last_run_ms), after a warm-up run;
  - features/s of rn_features_u8_device at 256 x 224 x 224 bf16 beside images/s of rn_forward_u8_device on the same handle;
  - ms per step of the float32 torch restatement (tests/finetune_ref.py) on 16 CPU threads, batch 45 at 224: what a user has today.

--depth 3 measures the trainer of the whole last conv block on cached s6.bn (rn_ft_create_depth: four launches per step, 256 resident
items at 224 and 48 at 600 -- an item is 1.08 MB and 10 MB) against the float32 torch restatement tests/finetune_ref.py, and states
each step against its arithmetic floor.  --lib PATH measures another build of the library (depth 2 of the commit before, say).

--dropout RATE measures, at batch 45 / 224 and both depths in one session with the arms alternating run by run, the step with
dropout off beside the step with dropout on (rn_ft_set_dropout) -- and, with --lib PATH, beside the dropout-off step of that other
build, a parent-commit build for instance -- and states whether this build's dropout-off range overlaps the other build's.  With
--trace-run / --summarise it is the five launches of a depth-3 step with dropout (ft7_drop_kernel in front) that are traced.

--val-every K measures what a validation point costs at batch 45 / 224, both depths and validation sets of 256 and 2048 items: inside
the run (rn_ft_run_validated) and the way there was before, K steps of rn_ft_run and an rn_ft_eval from the host in turn.

--views measures training on fresh random views (rn_ft_run_views) at batch 45 / 224 on a bf16 handle, depth 2 and depth 3, in one
session: the cached-feature run (rn_ft_run) and the views run alternate, --runs runs each after a warm-up round; and, between events
on the handle's stream, the view launch alone (rn_views_batch_device) and the trunk's feature pass alone (rn_features_depth_u8_device).
With --lib PATH a third arm runs the views step of that other build (handle and trainer both from it) in the same rotation: the A/B of
the two feature slots against one is --lib of a build with RN_VARIANT_FLAGS=-DFT_VIEW_SLOTS=1 (csrc/build.sh, RN_FILES=rn_finetune).

    python tools/bench_finetune.py [--depth 3] [--steps 200] [--runs 5] [--steps-only] [--lib PATH]
    python tools/bench_finetune.py --views [--lib ONE_SLOT_BUILD.so] [--steps 200] [--runs 3] [--out profiles/finetune_views_timing.json]
    python tools/bench_finetune.py --dropout 0.35 [--lib PARENT_BUILD.so] [--steps 200] [--runs 7]
    python tools/bench_finetune.py --val-every 10 [--steps 200] [--runs 5] [--out profiles/finetune_validate_timing.json]
    rocprofv3 --kernel-trace --stats -d DIR -o kt --output-format csv -- python tools/bench_finetune.py [--depth 3] --trace-run
    python tools/bench_finetune.py [--depth 3] --summarise DIR/.../kt_kernel_trace.csv [--out profiles/finetune_kernel_stats.txt]
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ((224, 45), (224, 256), (600, 45))
N_ITEMS = 512
KERNELS = {2: ("ft_item_kernel", "ft_update_kernel"), 3: ("ft7_fwd_kernel", "ft_item_kernel", "ft7_bwd_kernel", "ft_update_kernel")}
DROP_KERNEL = "ft7_drop_kernel"                  # depth 3 with dropout: the pre-pass in front of the four
DROP_CASES = ((224, 45),)
F32_MFMA_TFLOPS = 155.0                          # float32 MFMA = the float32 vector rate (measured peak of the part)
HBM_TBPS = 6.0


def n_items_of(side, depth):
    return N_ITEMS if depth == 2 else (256 if side == 224 else 48)


def _weights(side):
    from roomnet_amd.graph import build_graph
    from roomnet_amd.tf_bundle import BundleReader
    w = BundleReader(os.path.join(ROOT, "roomnet_amd", "final_model", "roomnet")).load_all()
    g = build_graph(6, side)
    if side != 224:
        w = dict(w)
        w["dense/kernel"] = np.random.default_rng(600).uniform(-0.04, 0.04, (g.flat_len, 32)).astype(np.float32)
    return g, w


def _data(g, n_items=N_ITEMS, depth=2):
    from roomnet_amd import finetune
    rng = np.random.default_rng(7)
    shape = finetune.feature_shape(g, depth) if depth != 2 else finetune.feature_shape(g)
    feats = (rng.standard_normal((n_items,) + shape, dtype=np.float32) * np.float32(0.5)) if depth != 2 else \
        (rng.standard_normal((n_items,) + shape) * 0.5).astype(np.float32)
    labels = rng.integers(0, 6, n_items).astype(np.int32)
    return feats, labels


def step_floor(g, batch):
    """Arithmetic floor of a depth-3 step: conv 7 forward and its weight gradient on the float32 matrix cores, and one read of the
    minibatch's cached features from HBM."""
    s7 = g.stages[-3]
    flop = 2 * 2.0 * batch * s7.conv_side ** 2 * 9 * s7.cin * s7.cout
    cache = 4.0 * batch * g.stages[-4].out_side ** 2 * s7.cin
    return {"conv7_gflop": round(flop / 1e9, 2), "mfma_floor_us": round(flop / F32_MFMA_TFLOPS / 1e6, 1),
            "cache_read_mb": round(cache / 1e6, 1), "hbm_floor_us": round(cache / HBM_TBPS / 1e6, 1)}


def dropout_case(side, batch, steps, runs, depth, rate, lib=None):
    """Dropout off, dropout on and (``lib``) the other build's dropout off on the same data: one trainer per arm, a warm-up run
    each, then ``runs`` rounds in which every arm runs once, in an order that rotates from round to round, so that drift of the
    clocks and whatever an arm inherits from the one before it hit all arms alike."""
    from roomnet_amd import _capi, finetune
    g, w = _weights(side)
    n_items = n_items_of(side, depth)
    feats, labels = _data(g, n_items, depth)
    index = finetune.epoch_indices(n_items, batch, steps, seed=1)
    arms = [("off", None, 0.0), ("on", None, rate)] + ([("other_off", lib, 0.0)] if lib else [])
    trainers, us = {}, {name: [] for name, _, _ in arms}
    try:
        for name, path, r in arms:
            tr = _capi.Trainer(g, w, device=0, max_batch=batch, learn_rate=2e-4, l2_coeff=0.06, lib_path=path, depth=depth)
            trainers[name] = (tr, [tr.upload(feats), tr.upload(labels), tr.upload(index)])
            if r:
                tr.set_dropout(r, 1)
        del feats
        for r in range(runs + 1):                                   # the first round is the warm-up
            k = r % len(arms)                                       # the order rotates, so that no arm always follows the same one
            for name, _, _ in arms[k:] + arms[:k]:
                tr, d = trainers[name]
                tr.run(d[0], d[1], n_items, d[2], batch, steps)
                us[name].append(tr.last_run_ms() * 1e3 / steps)
        out = {"side": side, "batch": batch, "depth": depth, "steps_per_run": steps, "runs": runs, "rate": rate}
        for name in us:
            v = us[name][1:]
            out[name] = {"us_per_step": round(statistics.median(v), 2), "us_per_step_min": round(min(v), 2),
                         "us_per_step_max": round(max(v), 2)}
        if lib:
            a, b = out["off"], out["other_off"]
            out["off_ranges_overlap"] = bool(a["us_per_step_min"] <= b["us_per_step_max"] and b["us_per_step_min"] <= a["us_per_step_max"])
        out["on_inside_off_range"] = bool(out["off"]["us_per_step_min"] <= out["on"]["us_per_step"] <= out["off"]["us_per_step_max"])
        if depth == 3:
            out["ft7_drop_kernel_bytes"] = 2 * batch * g.stages[-4].out_side ** 2 * g.stages[-3].cin * 4
        return out
    finally:
        for tr, _ in trainers.values():
            tr.close()


VAL_SIZES = (256, 2048)
VAL_MAX_BATCH = 256                              # the chunk of an evaluation pass: what RoomNet.fine_tune gives its trainer


def validate_case(side, batch, steps, runs, depth, n_val, val_every):
    """What a validation point costs at ``val_every``: (a) inside the run (rn_ft_run_validated) and (b) the only way there was
    before, ``val_every`` steps of rn_ft_run and an rn_ft_eval from the host in turn -- each as the host's wall time of the whole
    arm minus that of the same steps in one plain rn_ft_run, per point.  One trainer per arm on the same data, a warm-up round,
    then ``runs`` rounds in which every arm runs once, in an order that rotates."""
    from roomnet_amd import _capi, finetune
    steps -= steps % val_every                                      # every run then has steps / val_every points, wherever it starts
    points = steps // val_every
    g, w = _weights(side)
    n_items = n_items_of(side, depth)
    feats, labels = _data(g, n_items, depth)
    index = finetune.epoch_indices(n_items, batch, steps, seed=1)
    reps = -(-n_val // n_items)
    vfeats, vlabels = np.concatenate([feats] * reps)[:n_val], np.concatenate([labels] * reps)[:n_val]
    arms = ("plain", "validated", "alternating")
    trainers, ms, dev = {}, {a: [] for a in arms}, {a: [] for a in ("plain", "validated")}
    try:
        for name in arms:
            tr = _capi.Trainer(g, w, device=0, max_batch=VAL_MAX_BATCH, learn_rate=2e-4, l2_coeff=0.06, depth=depth)
            d = [tr.upload(feats), tr.upload(labels), tr.upload(index)]
            d += [] if name == "plain" else [tr.upload(vfeats), tr.upload(vlabels)]
            trainers[name] = (tr, d)
        del feats, vfeats

        def run(name):
            tr, d = trainers[name]
            t0 = time.perf_counter()
            if name == "plain":
                tr.run(d[0], d[1], n_items, d[2], batch, steps)
            elif name == "validated":
                tr.run_validated(d[0], d[1], n_items, d[2], batch, steps, d[3], d[4], n_val, val_every)
            else:
                for p in range(points):
                    tr.run(d[0], d[1], n_items, d[2] + 4 * batch * val_every * p, batch, val_every)
                    tr.eval(d[3], n_val, d[4])
            ms[name].append((time.perf_counter() - t0) * 1e3)
            if name in dev:
                dev[name].append(tr.last_run_ms())

        for r in range(runs + 1):                                   # the first round is the warm-up
            k = r % len(arms)
            for name in arms[k:] + arms[:k]:
                run(name)
        med = {a: statistics.median(v[1:]) for a, v in ms.items()}
        out = {"side": side, "batch": batch, "depth": depth, "n_val": n_val, "val_every": val_every, "steps_per_run": steps,
               "points_per_run": points, "runs": runs, "eval_chunk": VAL_MAX_BATCH}
        for a in arms:
            out[a + "_wall_ms"] = {"median": round(med[a], 3), "min": round(min(ms[a][1:]), 3), "max": round(max(ms[a][1:]), 3)}
        out["inside_run_us_per_point"] = round((med["validated"] - med["plain"]) * 1e3 / points, 1)
        out["alternating_us_per_point"] = round((med["alternating"] - med["plain"]) * 1e3 / points, 1)
        out["inside_run_device_us_per_point"] = round((statistics.median(dev["validated"][1:]) - statistics.median(dev["plain"][1:]))
                                                      * 1e3 / points, 1)
        out["inside_run_below_alternating"] = bool(out["inside_run_us_per_point"] < out["alternating_us_per_point"])
        return out
    finally:
        for tr, _ in trainers.values():
            tr.close()


VIEW_SHAPES = ((480, 640), (640, 480), (1080, 1920), (224, 224), (448, 448), (600, 800))      # (height, width) of the resident photographs
VIEW_ITEMS = 96


def views_case(depth, steps, runs, batch=45, lib=None):
    """The cached-feature step beside the step on fresh views -- and (``lib``) beside the views step of another build, handle and
    trainer both of that build: a one-slot build, say --, the arms in an order that rotates run by run after a warm-up round; then
    the view launch and the trunk's feature pass of one minibatch alone, between events on the handle's stream."""
    import torch
    from roomnet_amd import _capi, finetune
    g, w = _weights(224)
    rng = np.random.default_rng(11)
    photos = [rng.integers(0, 256, VIEW_SHAPES[k % len(VIEW_SHAPES)] + (3,), dtype=np.uint8) for k in range(VIEW_ITEMS)]
    feats, labels = _data(g, VIEW_ITEMS, depth)
    index = finetune.epoch_indices(VIEW_ITEMS, batch, steps, seed=1)
    eng = _capi.Engine(g, w, device=0, dtype="bf16", max_batch=batch)
    arms = ["cached", "views"] + (["views_other"] if lib else [])
    views, trainers, us, other = None, {}, {a: [] for a in arms}, None
    try:
        views = eng.views_create(photos)
        if lib:
            other_eng = _capi.Engine(g, w, device=0, dtype="bf16", max_batch=batch, lib_path=lib)
            other = (other_eng, other_eng.views_create(photos))
        for name in arms:
            tr = _capi.Trainer(g, w, device=0, max_batch=batch, learn_rate=2e-4, l2_coeff=0.06, depth=depth,
                               lib_path=lib if name == "views_other" else None)
            trainers[name] = (tr, [tr.upload(feats) if name == "cached" else 0, tr.upload(labels), tr.upload(index)])
        del feats
        for r in range(runs + 1):                                   # the first round is the warm-up
            k = r % len(arms)
            for name in arms[k:] + arms[:k]:
                tr, d = trainers[name]
                if name == "cached":
                    tr.run(d[0], d[1], VIEW_ITEMS, d[2], batch, steps)
                elif name == "views":
                    tr.run_views(eng, views, d[1], d[2], batch, steps, seed=1)
                else:
                    tr.run_views(other[0], other[1], d[1], d[2], batch, steps, seed=1)
                us[name].append(tr.last_run_ms() * 1e3 / steps)
        out = {"side": 224, "dtype": "bf16", "batch": batch, "depth": depth, "steps_per_run": steps, "runs": runs,
               "photographs": VIEW_ITEMS, "photograph_shapes": [list(s) for s in VIEW_SHAPES], "resident_bytes": views.nbytes,
               "other_lib": lib}
        for name, v in us.items():
            v = v[1:]
            out[name] = {"us_per_step": round(statistics.median(v), 2), "us_per_step_min": round(min(v), 2),
                         "us_per_step_max": round(max(v), 2)}
        out["views_minus_cached_us"] = round(out["views"]["us_per_step"] - out["cached"]["us_per_step"], 2)
        if lib:
            a, b = out["views"], out["views_other"]
            out["views_ranges_overlap"] = bool(a["us_per_step_min"] <= b["us_per_step_max"] and b["us_per_step_min"] <= a["us_per_step_max"])
        # the two launches in front of a step, alone
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        d_index = torch.from_numpy(index[0].copy()).cuda()
        d_bgr = torch.empty((batch, 224, 224, 3), dtype=torch.uint8, device="cuda")
        d_f = torch.empty((batch,) + finetune.feature_shape(g, depth), dtype=torch.float32, device="cuda")
        import ctypes as C

        def make_views():
            _capi._check(eng.lib, eng.lib.rn_views_batch_device(eng.handle, views.handle, C.c_void_p(d_index.data_ptr()), 0, batch, 1, 0, 3,
                                                                C.c_void_p(d_bgr.data_ptr())), "rn_views_batch_device")

        def timed(fn, reps=50, warmup=5):
            for _ in range(warmup):
                fn()
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            torch.cuda.synchronize()
            return a.elapsed_time(b) * 1e3 / reps

        vl = [timed(make_views) for _ in range(max(runs, 1))]
        fp = [timed(lambda: eng.features_u8_device(d_bgr.data_ptr(), batch, d_f.data_ptr(), depth=depth)) for _ in range(max(runs, 1))]
        eng.set_stream(None)
        out["view_launch_us"] = {"median": round(statistics.median(vl), 2), "min": round(min(vl), 2), "max": round(max(vl), 2)}
        out["feature_pass_us"] = {"median": round(statistics.median(fp), 2), "min": round(min(fp), 2), "max": round(max(fp), 2)}
        return out
    finally:
        for tr, _ in trainers.values():
            tr.close()
        if views is not None:
            views.close()
        if other is not None:
            other[1].close()
            other[0].close()
        eng.close()


def step_case(side, batch, steps, runs, depth=2, lib=None, dropout=0.0):
    from roomnet_amd import _capi, finetune
    g, w = _weights(side)
    n_items = n_items_of(side, depth)
    feats, labels = _data(g, n_items, depth)
    index = finetune.epoch_indices(n_items, batch, steps, seed=1)
    kw = {"depth": depth} if depth != 2 else {}
    tr = _capi.Trainer(g, w, device=0, max_batch=batch, learn_rate=2e-4, l2_coeff=0.06, lib_path=lib, **kw)
    try:
        if dropout:
            tr.set_dropout(dropout, 1)
        d = [tr.upload(feats), tr.upload(labels), tr.upload(index)]
        del feats
        tr.run(d[0], d[1], n_items, d[2], batch, steps)            # warm-up
        us = []
        for _ in range(runs):
            tr.run(d[0], d[1], n_items, d[2], batch, steps)
            us.append(tr.last_run_ms() * 1e3 / steps)
        out = {"side": side, "batch": batch, "depth": depth, "steps_per_run": steps, "us_per_step": round(statistics.median(us), 2),
               "us_per_step_min": round(min(us), 2), "us_per_step_max": round(max(us), 2)}
        if depth == 3:
            out["floor"] = step_floor(g, batch)
        return out
    finally:
        tr.close()


def features_case(steps=20, warmup=5):
    import torch
    from roomnet_amd import _capi
    from roomnet_amd.synth import parity_set
    g, w = _weights(224)
    fields = np.load(os.path.join(ROOT, "tests", "golden", "class_fields.npz"))["fields_u8"]
    ims = parity_set(224, fields)
    ims = np.ascontiguousarray(np.concatenate([ims] * 4)[:256])
    eng = _capi.Engine(g, w, device=0, dtype="bf16", max_batch=256)
    try:
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        d_in = torch.from_numpy(ims).cuda()
        d_f = torch.empty((256, 21, 21, 16), dtype=torch.float32, device="cuda")
        d_probs = torch.empty((256, 6), dtype=torch.float32, device="cuda")
        d_ids = torch.empty((256,), dtype=torch.int64, device="cuda")

        def timed(fn):
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

        fwd = timed(lambda: eng.forward_u8_device(d_in.data_ptr(), 256, d_probs.data_ptr(), d_ids.data_ptr()))
        fea = timed(lambda: eng.features_u8_device(d_in.data_ptr(), 256, d_f.data_ptr()))
        eng.set_stream(None)
        return {"side": 224, "dtype": "bf16", "batch": 256, "forward_ms": round(fwd, 4), "features_ms": round(fea, 4),
                "forward_images_per_s": round(256e3 / fwd, 1), "features_per_s": round(256e3 / fea, 1)}
    finally:
        eng.close()


def torch_case(batch=45, steps=5, threads=16, depth=2):
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from finetune_ref import FineTune7Ref, FineTuneRef
    from roomnet_amd import finetune
    torch.set_num_threads(threads)
    g, w = _weights(224)
    n_items = n_items_of(224, depth)
    feats, labels = _data(g, n_items, depth)
    index = finetune.epoch_indices(n_items, batch, steps + 1, seed=1)
    ref = (FineTuneRef if depth == 2 else FineTune7Ref)(w, 6, 224, dtype=torch.float32)
    ref.train(feats, labels, index[:1], 2e-4, 10000, 0.06)
    t0 = time.perf_counter()
    ref.train(feats, labels, index[1:], 2e-4, 10000, 0.06)
    return {"side": 224, "batch": batch, "threads": threads, "ms_per_step": round((time.perf_counter() - t0) * 1e3 / steps, 2)}


def trace_run(depth=2, dropout=0.0):
    for side, batch in (DROP_CASES if dropout else CASES):
        step_case(side, batch, TRACE_STEPS, 1, depth, dropout=dropout)


TRACE_STEPS = 20                                  # steps per rn_ft_run of --trace-run (a warm-up run and a measured one per case)


def summarise(trace_csv, depth=2, dropout=0.0):
    kernels = ((DROP_KERNEL,) if dropout and depth == 3 else ()) + KERNELS[depth]
    cases = DROP_CASES if dropout else CASES
    rows = []
    for r in csv.DictReader(open(trace_csv)):
        for key in kernels:
            if key in r["Kernel_Name"]:
                wgs = int(r["Grid_Size_X"]) // max(int(r["Workgroup_Size_X"]), 1) * max(int(r.get("Grid_Size_Y") or 1), 1)
                rows.append((int(r["Start_Timestamp"]), key, wgs,
                             (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    rows.sort()
    per_case = 2 * len(kernels) * TRACE_STEPS     # the cases run one after the other: two runs x the launches of a step
    if len(rows) != per_case * len(cases):
        raise SystemExit("expected %d ft_* launches (%d cases), found %d" % (per_case * len(cases), len(cases), len(rows)))
    lines = ["# rocprofv3 --kernel-trace --stats -- python tools/bench_finetune.py%s%s --trace-run (one MI355X, its own run)"
             % (" --depth 3" if depth == 3 else "", " --dropout %g" % dropout if dropout else ""),
             "# the %s launches of an Adam step per case: workgroups, calls, median / max duration in us, and the step's sum"
             % {2: "two", 4: "four", 5: "five"}[len(kernels)],
             "%5s %6s  %-17s %6s %6s %11s %9s" % ("side", "batch", "kernel", "wgs", "calls", "median_us", "max_us")]
    for ci, (side, batch) in enumerate(cases):
        total = 0.0
        for key in kernels:
            sel = [r for r in rows[ci * per_case:(ci + 1) * per_case] if r[1] == key]
            us = [r[3] for r in sel]
            total += statistics.median(us)
            lines.append("%5d %6d  %-17s %6d %6d %11.1f %9.1f" % (side, batch, key, sel[0][2], len(us), statistics.median(us), max(us)))
        lines.append("%5d %6d  %-17s %6s %6s %11.1f" % (side, batch, {2: "both", 4: "all four", 5: "all five"}[len(kernels)], "", "", total))
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps-only", action="store_true", help="only the us-per-step cases")
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--summarise", metavar="KERNEL_TRACE_CSV")
    ap.add_argument("--out")
    ap.add_argument("--depth", type=int, default=2, choices=(2, 3), help="trained conv stages: 2 (features s7.bn) or 3 (s6.bn)")
    ap.add_argument("--lib", help="measure this build of libroomnet_hip.so instead of the package's")
    ap.add_argument("--dropout", type=float, default=0.0, metavar="RATE",
                    help="the dropout-on arm beside the dropout-off arm (and beside --lib's dropout-off arm) at both depths")
    ap.add_argument("--val-every", type=int, default=0, metavar="K",
                    help="what a validation point costs inside the run (rn_ft_run_validated) and from the host (rn_ft_run / rn_ft_eval)")
    ap.add_argument("--views", action="store_true",
                    help="the step on fresh random views (rn_ft_run_views) beside the cached-feature step, both depths, and the view launch alone")
    args = ap.parse_args()
    if not args.summarise:
        import torch  # noqa: F401  (before libroomnet_hip.so is loaded: one HIP runtime in the process, torch's)
    if args.summarise:
        text = summarise(args.summarise, args.depth, args.dropout)
        if args.out:
            open(args.out, "w").write(text)
        print(text, end="")
        return
    if args.trace_run:
        trace_run(args.depth, args.dropout)
        return
    if args.views:
        doc = {"what": "fine-tuning on fresh random views (rn_ft_run_views) at batch 45 / 224 on a bf16 handle, one session on one MI355X: "
                       "us per Adam step (device time of the step loop, rn_ft_last_run_ms) of the cached-feature run and of the views "
                       "run, the arms alternating run by run after a warm-up round; the view launch and the trunk's feature pass of "
                       "one minibatch alone, between events on the handle's stream; views_other: the views run of the build given with "
                       "--lib (handle and trainer both of that build)",
               "cases": [views_case(depth, args.steps, args.runs, lib=args.lib) for depth in (2, 3)]}
        text = json.dumps(doc, indent=1)
        if args.out:
            open(args.out, "w").write(text + "\n")
        print(json.dumps(doc))
        return
    if args.val_every:
        doc = {"what": "validation inside a fine-tuning run at batch 45 / 224, val_every %d, both depths, n_val 256 and 2048, the arms "
                       "alternating run by run in one session: host wall time of (a) rn_ft_run_validated and of (b) rn_ft_run(%d "
                       "steps) and rn_ft_eval in turn from the host, each minus the same steps in one plain rn_ft_run, per point"
                       % (args.val_every, args.val_every),
               "cases": [validate_case(s, b, args.steps, args.runs, depth, n_val, args.val_every)
                         for depth in (2, 3) for s, b in DROP_CASES for n_val in VAL_SIZES]}
        text = json.dumps(doc, indent=1)
        if args.out:
            open(args.out, "w").write(text + "\n")
        print(json.dumps(doc))
        return
    if args.dropout:
        print(json.dumps({"what": "fine-tuning with dropout: us per Adam step at batch 45 / 224, dropout off, dropout on at rate %g and "
                                  "(other_off) dropout off of the build given with --lib, the arms alternating run by run in one "
                                  "session; ft7_drop_kernel moves ft7_drop_kernel_bytes per step (one read and one write of the "
                                  "minibatch's s6.bn)" % args.dropout,
                          "other_lib": args.lib,
                          "cases": [dropout_case(s, b, args.steps, args.runs, depth, args.dropout, args.lib)
                                    for depth in (2, 3) for s, b in DROP_CASES]}))
        return
    if args.steps_only:
        print(json.dumps({"depth": args.depth, "lib": args.lib,
                          "steps": [step_case(s, b, args.steps, args.runs, args.depth, args.lib) for s, b in CASES]}))
        return
    if args.depth == 3:
        print(json.dumps({"what": "fine-tuning the whole last conv block on cached s6.bn features: us per Adam step (four launches, "
                                  "enqueued back to back) against its arithmetic floor, and the float32 torch restatement on the CPU",
                          "steps": [step_case(s, b, args.steps, args.runs, 3, args.lib) for s, b in CASES],
                          "torch_float32_cpu": torch_case(depth=3)}))
        return
    print(json.dumps({"what": "fine-tuning on cached s7.bn features: us per Adam step (two launches, enqueued back to back), feature "
                              "extraction beside the plain forward pass, and the float32 torch restatement on the CPU",
                      "steps": [step_case(s, b, args.steps, args.runs) for s, b in CASES],
                      "features": features_case(), "torch_float32_cpu": torch_case()}))


if __name__ == "__main__":
    main()
