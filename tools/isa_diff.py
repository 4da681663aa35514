"""Two assembly listings of one kernel file (hipcc -S --cuda-device-only) held to each other, kernel by kernel.

    python tools/isa_diff.py PARENT.s COMMIT.s [--diff]

Per kernel symbol and side: instruction count, VGPRs, SGPRs, spilled dwords, scratch bytes and a digest (blake2b-128) of the normalised
body; then the verdict on the pair:
  A  the bodies are identical (and so are the figures);
  B  the figures are equal and no differing line lies in a basic block that holds a v_mfma instruction or inside a loop (between a
     label and a later branch back to it);
  C  anything else.
For B and C the first differing line of each side is printed, with --diff the whole unified diff.  The exit status is 1 if any pair is
C or a kernel exists on one side only.

Normalisation (the method of profiles/pair_pipeline_isa.txt): comment lines and trailing comments dropped, the translation unit's
__hip_cuid_* symbol spelled __hip_cuid_, the function's ordinal taken out of its labels (.LBB12_7 -> .LBB_7, .Lfunc_end12 -> .Lfunc_end).
"""
import argparse
import difflib
import hashlib
import re
import sys

_LABEL = re.compile(r"^([.\w$]+):")
_ORDINAL = re.compile(r"\.(LBB|Lfunc_end|Lfunc_begin|LJTI|Ltmp)\d+")
_CUID = re.compile(r"__hip_cuid_[0-9a-f]+")
_META = {"vgprs": ".vgpr_count", "sgprs": ".sgpr_count", "vgpr_spills": ".vgpr_spill_count", "sgpr_spills": ".sgpr_spill_count",
         "scratch": ".private_segment_fixed_size"}


def _normalise(line):
    line = line.split(";", 1)[0].rstrip()
    line = _CUID.sub("__hip_cuid_", line)
    return _ORDINAL.sub(lambda m: "." + m.group(1), line)


def parse_listing(text):
    """{kernel symbol: {"body": [normalised lines], "instrs", "vgprs", "sgprs", "spills", "scratch", "digest"}}"""
    lines = text.splitlines()
    functions = [m.group(1) for m in (re.match(r"\s*\.type\s+([.\w$]+),@function", l) for l in lines) if m]
    out = {}
    for sym in functions:
        start = next((i for i, l in enumerate(lines) if l.startswith(sym + ":")), None)
        if start is None:
            continue
        end = next((i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end")), len(lines))
        body = [n for n in map(_normalise, lines[start + 1:end]) if n.strip()]
        out[sym] = {"body": body, "instrs": sum(1 for l in body if _is_instruction(l)),
                    "digest": hashlib.blake2b("\n".join(body).encode(), digest_size=16).hexdigest()}
    # the figures: the kernel's entry in the metadata note (amdhsa.kernels: a list, "  - " opens an entry, its keys are indented by four)
    entries, inside = [], False
    for l in lines:
        if l.startswith("amdhsa.kernels:"):
            inside = True
        elif inside and l.startswith("  - "):
            entries.append({})
        elif inside and not l.startswith("  "):
            inside = False
        m = re.match(r"^(?:  - |    )(\.\w+):\s+(\S+)$", l) if inside and entries else None
        if m:
            entries[-1][m.group(1)] = m.group(2)
    for entry in entries:
        rec = out.get(entry.get(".name"))
        if rec is not None:
            for key, field in _META.items():
                rec[key] = int(entry.get(field, 0))
            rec["spills"] = rec.pop("vgpr_spills") + rec.pop("sgpr_spills")
    return {k: v for k, v in out.items() if "vgprs" in v}      # (kernels only: a device function has no entry)


def _is_instruction(line):
    s = line.strip()
    return bool(s) and not s.startswith(".") and not _LABEL.match(s)


def _is_branch(line):
    op = line.split()[0] if line.split() else ""
    return op.startswith(("s_cbranch", "s_branch", "s_endpgm", "s_setpc"))


def hot_lines(body):
    """per line of a body: it lies in a basic block with a v_mfma instruction, or inside a loop"""
    n = len(body)
    hot = [False] * n
    label_at = {m.group(1): i for i, m in ((i, _LABEL.match(l.strip())) for i, l in enumerate(body)) if m}
    # basic blocks: a label opens one, a branch closes one
    start = 0
    for i in range(n + 1):
        opens = i < n and _LABEL.match(body[i].strip())
        closes = i > 0 and i <= n and _is_instruction(body[i - 1]) and _is_branch(body[i - 1])
        if i == n or opens or closes:
            if any("v_mfma" in l for l in body[start:i]):
                hot[start:i] = [True] * (i - start)
            start = i
    for i, l in enumerate(body):
        if _is_instruction(l) and _is_branch(l):
            target = label_at.get(l.split()[-1])
            if target is not None and target <= i:
                hot[target:i + 1] = [True] * (i + 1 - target)
    return hot


def compare(a, b):
    """(verdict 'A' / 'B' / 'C', first differing line of a, of b, its index in a's body, the opcodes of the difference)"""
    figures = ("instrs", "vgprs", "sgprs", "spills", "scratch")
    if a["body"] == b["body"]:
        return ("A" if all(a[f] == b[f] for f in figures) else "C"), None, None, None, []
    ops = [o for o in difflib.SequenceMatcher(None, a["body"], b["body"], autojunk=False).get_opcodes() if o[0] != "equal"]
    cold = all(a[f] == b[f] for f in figures)
    for body, lo, hi in [(a["body"], o[1], o[2]) for o in ops] + [(b["body"], o[3], o[4]) for o in ops]:
        hot = hot_lines(body)
        span = range(lo, hi) if hi > lo else range(min(lo, len(body) - 1), min(lo, len(body) - 1) + 1)      # (an insertion: where it went)
        cold = cold and not any(hot[i] for i in span)
    _, i1, _, j1, _ = ops[0]
    line = lambda body, i: body[i].strip() if i < len(body) else "(end)"
    return ("B" if cold else "C"), line(a["body"], i1), line(b["body"], j1), i1, ops


def report(parent, commit, full_diff=False):
    """(text, every pair is A or B)"""
    cols = "%-70s %-7s %7s %6s %6s %7s %8s  %s"
    out = [cols % ("kernel", "side", "instrs", "VGPRs", "SGPRs", "spills", "scratch", "digest")]
    ok = True
    for sym in sorted(set(parent) | set(commit)):
        for side, table in (("parent", parent), ("commit", commit)):
            if sym in table:
                r = table[sym]
                out.append(cols % (sym, side, r["instrs"], r["vgprs"], r["sgprs"], r["spills"], r["scratch"], r["digest"]))
        if sym not in parent or sym not in commit:
            out.append("  only in the %s listing" % ("parent's" if sym in parent else "commit's"))
            ok = False
            continue
        verdict, la, lb, at, ops = compare(parent[sym], commit[sym])
        if verdict == "A":
            out.append("  A: identical, %d lines" % len(parent[sym]["body"]))
            continue
        ok = ok and verdict == "B"
        if not ops:
            out.append("  C: the bodies are identical, the figures moved")
            continue
        out.append("  %s: %d differing stretches, %s; first at body line %d: parent '%s' against '%s'" %
                   (verdict, len(ops), "all outside MFMA blocks and loops, figures equal" if verdict == "B" else "in matrix code or a loop, or the figures moved",
                    at + 1, la, lb))
        if full_diff:
            out += ["    " + l for l in difflib.unified_diff(parent[sym]["body"], commit[sym]["body"], "parent", "commit", n=2, lineterm="")]
    return "\n".join(out) + "\n", ok


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("parent")
    ap.add_argument("commit")
    ap.add_argument("--diff", action="store_true", help="print the unified diff of every pair that is not identical")
    args = ap.parse_args()
    text, ok = report(parse_listing(open(args.parent).read()), parse_listing(open(args.commit).read()), args.diff)
    print(text, end="")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
