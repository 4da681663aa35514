"""Two builds of the library held to each other on the 16-bit path and the float32 path: every output byte and every launch.

For a refactor of the host side (rn_fused.hip, rn_stage_f32m.hip) that must change neither.  One run per build writes a digest of probs, ids and of
every tensor rn_tap returns, case by case; under rocprofv3 the same run is the build's launch sequence.  --summarise compares the two.

    rocprofv3 --kernel-trace -d DIR_A -o kt --output-format csv -- python tools/fused_plan_ab.py --trace-run --lib A.so --ab-lib A_ab.so --dump a.json
    rocprofv3 --kernel-trace -d DIR_B -o kt --output-format csv -- python tools/fused_plan_ab.py --trace-run --lib B.so --ab-lib B_ab.so --dump b.json
    python tools/fused_plan_ab.py --summarise a.json b.json A_kernel_trace.csv B_kernel_trace.csv [--rename OLD=NEW ...]
        [--rename-re PATTERN=REPLACEMENT ...] [--skip-prefix PREFIX ...] [--out profiles/fused_plan_launches.txt]

--rename: a substring of A's kernel names that build B spells differently (a parameter type that moved to another namespace, say); A's
names are compared under the new spelling and the summary says how many launches that touched.  --rename-re: the same with a regular
expression and its replacement (re.sub; a template list that lost parameters in build B; the option is split at its first `=`, so
the pattern itself cannot contain one: write `\\x3d`).  --skip-prefix: kernels left out of the
launch comparison on both sides, counted in the summary (the HIP runtime's own copy kernels `__amd_rocclr_`, which are the uploads
of rn_create and not launches of the forward pass).  The trace reports a kernel's static LDS only: dynamic LDS is not compared.

Cases: bf16 and f16; sides 190 (no fused pair), 224, 300, 420, 600 at batch 3 and side 224 at ceil(n_cu / 2) images (the back end in
one launch); the default handle, stage_launches, generic_kernels, compute_frozen, no_dither and pair32 (the A/B library); the shipped
checkpoint, and at 224 the `live` recipe of tests/checkpoints.py, which folds nothing.  The fused pair runs in its eight-channel form on the
shipped checkpoint (24 constant channels of stage 2) and in its full form on `live` and compute_frozen; its 16-channel form needs a
checkpoint that freezes 16 to 23: `gammas_other_sets` (17), default handle, both types, sides 224 and 420 (one column block and two).
Float32 cases: the same sides and batches; the default handle (the matrix-core stages of rn_stage_f32m.hip), compute_frozen, taps and
batch_stats (the per-node kernels); the shipped checkpoint, `live`, and at 224 the four `with_gammas` checkpoints of
tests/test_hip_f32.py::test_matrix_core_f32_fold_on_other_checkpoints (folds elsewhere, taken back, none).  The float32 stage
kernels' LDS is all dynamic: tests/test_f32m_plan.py pins it on the CPU.
"""
import argparse
import csv
import functools
import hashlib
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HANDLES = ("default", "stage_launches", "generic_kernels", "compute_frozen", "no_dither", "pair32")
F32_HANDLES = ("default", "compute_frozen", "taps", "batch_stats")
# tests/test_hip_f32.py::test_matrix_core_f32_fold_on_other_checkpoints: frozen channels of stage 2's BN and stage 5's first BN, seed
GAMMAS = {"none": (0, 0, 1), "nine_and_31": (9, 31, 2), "other_sets": (17, 40, 3), "everything": (32, 64, 4)}
SIDES = (190, 224, 300, 420, 600)
BATCH = 3
PAIR16_SIDES = (224, 420)       # the 16-bit cases of gammas_other_sets: one column block and two


def case_list(n_big):
    cases = []
    for dtype in ("bf16", "f16"):
        for handle in HANDLES:
            for side in SIDES:
                cases.append(("shipped", dtype, handle, side, BATCH))
            cases.append(("shipped", dtype, handle, 224, n_big))
            cases.append(("live", dtype, handle, 224, BATCH))
        for side in PAIR16_SIDES:
            cases.append(("gammas_other_sets", dtype, "default", side, BATCH))
    for handle in F32_HANDLES:
        for side in SIDES:
            cases.append(("shipped", "f32", handle, side, BATCH))
        cases.append(("shipped", "f32", handle, 224, n_big))
        for kind in ("live",) + tuple("gammas_" + k for k in GAMMAS):
            cases.append((kind, "f32", handle, 224, BATCH))
    return cases


@functools.lru_cache(maxsize=None)
def _weights(kind, side):
    from roomnet_amd.graph import build_graph
    from roomnet_amd.tf_bundle import BundleReader
    g = build_graph(6, side)
    if kind == "live":
        import checkpoints
        return g, checkpoints.live(g, 1, checkpoints.LIVE_GAIN)
    w = dict(BundleReader(os.path.join(ROOT, "roomnet_amd", "final_model", "roomnet")).load_all())
    if side != 224:
        w["dense/kernel"] = np.random.default_rng(side).uniform(-0.04, 0.04, (g.flat_len, 32)).astype(np.float32)
    if kind.startswith("gammas_"):
        from conftest import with_gammas
        n2, n5, seed = GAMMAS[kind[len("gammas_"):]]
        rng = np.random.default_rng(6)
        bn2 = range(32) if n2 == 32 else rng.choice(32, n2, replace=False) if n2 else []
        return g, with_gammas(w, bn2, range(64) if n5 == 64 else rng.choice(64, n5, replace=False) if n5 else [], seed)
    return g, w


@functools.lru_cache(maxsize=None)
def _parity_images(side):
    from roomnet_amd.synth import parity_set
    return parity_set(side, np.load(os.path.join(ROOT, "tests", "golden", "class_fields.npz"))["fields_u8"])


def _images(side, n):
    ims = _parity_images(side)
    return ims[(np.arange(n) * 3 + 2) % len(ims)]


def _digest(a):
    return hashlib.blake2b(np.ascontiguousarray(a).tobytes(), digest_size=16).hexdigest()


def trace_run(lib, ab_lib, dump):
    import torch
    from roomnet_amd import _capi
    n_big = (torch.cuda.get_device_properties(0).multi_processor_count + 1) // 2
    out = {"n_big": n_big, "cases": {}}
    for kind, dtype, handle, side, n in case_list(n_big):
        g, w = _weights(kind, side)
        flags = {handle: True} if handle != "default" else {}
        e = _capi.Engine(g, w, device=0, dtype=dtype, max_batch=n, lib_path=ab_lib if handle == "pair32" else lib, **flags)
        try:
            ids, probs = e.forward_u8(_images(side, n))
            rec = {"probs": _digest(probs), "ids": _digest(ids), "frozen": e.frozen_info(), "const": e.const_info()}
            for name in sorted(e.nodes()):
                try:
                    rec["tap " + name] = _digest(e.tap(name, n))
                except (ValueError, _capi.RoomNetLibraryError) as err:      # (a tensor this handle never writes: both builds must say so)
                    rec["tap " + name] = "no tensor: " + str(err).split(":")[-1].strip()[:60]
        finally:
            e.close()
        out["cases"]["%s %s %s side %d n %d" % (kind, dtype, handle, side, n)] = rec
    with open(dump, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)


def _launches(trace_csv, rename, skip):
    """(launches in order, how many launches each rename touched, how many were skipped)"""
    rows = list(csv.DictReader(open(trace_csv)))
    rows.sort(key=lambda r: (int(r["Start_Timestamp"]), int(r.get("Dispatch_Id") or 0)))
    out, renamed, skipped = [], [0] * len(rename), 0
    for r in rows:
        name = r["Kernel_Name"]
        if name.startswith(tuple(skip)):
            skipped += 1
            continue
        for k, (old, new) in enumerate(rename):
            new_name = re.sub(old, new, name) if isinstance(old, re.Pattern) else name.replace(old, new)
            renamed[k] += new_name != name
            name = new_name
        grid = tuple(int(r.get("Grid_Size_" + d) or r.get("Grid_Size") or 0) for d in "XYZ")
        wg = tuple(int(r.get("Workgroup_Size_" + d) or r.get("Workgroup_Size") or 0) for d in "XYZ")
        out.append((name, grid, wg, int(r.get("LDS_Block_Size") or r.get("LDS_Block_Size_v") or 0)))
    return out, renamed, skipped


def summarise(dump_a, dump_b, trace_a, trace_b, rename=(), skip=()):
    a, b = json.load(open(dump_a)), json.load(open(dump_b))
    lines = ["# tools/fused_plan_ab.py: parent (A) against this commit (B), one MI355X, one process per build under",
             "# rocprofv3 --kernel-trace (nothing else traced); ceil(n_cu / 2) = %d" % a["n_big"]]
    ok = a["n_big"] == b["n_big"] and sorted(a["cases"]) == sorted(b["cases"])
    same = [c for c in a["cases"] if b["cases"].get(c) == a["cases"][c]]
    n_tensors = sum(len(v) for v in a["cases"].values())
    lines.append("outputs (probs, ids, every rn_tap tensor, frozen / constant channel info; %d digests): %d cases, %d identical"
                 % (n_tensors, len(a["cases"]), len(same)))
    for name, part in (("16-bit", [c for c in a["cases"] if c.split()[1] != "f32"]), ("float32", [c for c in a["cases"] if c.split()[1] == "f32"])):
        lines.append("  %s: %d of %d cases identical" % (name, len([c for c in part if c in same]), len(part)))
    for c in sorted(a["cases"]):
        if c not in same:
            diff = [k for k in a["cases"][c] if b["cases"].get(c, {}).get(k) != a["cases"][c][k]]
            lines.append("  DIFFERENT: %s: %s" % (c, ", ".join(diff)))
    (la, n_renamed, ra), (lb, _, rb) = _launches(trace_a, rename, skip), _launches(trace_b, (), skip)
    first = next((i for i, (x, y) in enumerate(zip(la, lb)) if x != y), None)
    launches_same = first is None and len(la) == len(lb)
    lines.append("launches (kernel name, grid, workgroup size, static LDS bytes), in order: %d against %d, %s" %
                 (len(la), len(lb), "identical line for line" if launches_same else "FIRST DIFFERENCE at line %s" % first))
    lines.append("  (the trace reports static LDS only: the dynamic LDS of a launch is not in this comparison)")
    for (old, new), k in zip(rename, n_renamed):
        lines.append("  (A's kernel names are compared with '%s' spelled '%s', as B spells it: %d launches)"
                     % (getattr(old, "pattern", old), new, k))
    for prefix in skip:
        lines.append("  (not compared: kernels named %s*, %d against %d)" % (prefix, ra, rb))
    if not launches_same and first is not None:
        lines += ["  A: %r" % (la[first],), "  B: %r" % (lb[first],)]
    counts = {}
    for x in lb:
        counts[x] = counts.get(x, 0) + 1
    lines.append("distinct launches of this commit (count, kernel, grid, workgroup, static LDS):")
    for x, k in sorted(counts.items(), key=lambda kv: (kv[0][0], kv[0][1])):
        lines.append("%6d  %s  grid %s  wg %s  lds %d" % (k, x[0], "x".join(map(str, x[1])), "x".join(map(str, x[2])), x[3]))
    ok = ok and len(same) == len(a["cases"]) and launches_same
    lines.append("verdict: %s" % ("PASS" if ok else "FAIL"))
    return "\n".join(lines) + "\n", ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--lib", help="the build of libroomnet_hip.so to run (default: the package's)")
    ap.add_argument("--ab-lib", help="... and of libroomnet_hip_ab.so, for the pair32 handles")
    ap.add_argument("--dump", default="fused_plan_digests.json")
    ap.add_argument("--summarise", nargs=4, metavar=("DUMP_A", "DUMP_B", "TRACE_A", "TRACE_B"))
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW", help="A's kernel names are compared with OLD spelled NEW")
    ap.add_argument("--rename-re", action="append", default=[], metavar="PATTERN=REPLACEMENT",
                    help="the same, by re.sub; split at the first '=', so PATTERN cannot contain one (write \\x3d)")
    ap.add_argument("--skip-prefix", action="append", default=[], metavar="PREFIX", help="kernels left out of the launch comparison")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.summarise:
        rename = [tuple(r.split("=", 1)) for r in args.rename]
        rename += [(re.compile(p), new) for p, new in (r.split("=", 1) for r in args.rename_re)]
        text, ok = summarise(*args.summarise, rename=rename, skip=args.skip_prefix)
        if args.out:
            open(args.out, "w").write(text)
        print(text, end="")
        sys.exit(0 if ok else 1)
    if args.trace_run:
        trace_run(args.lib, args.ab_lib, args.dump)


if __name__ == "__main__":
    main()
