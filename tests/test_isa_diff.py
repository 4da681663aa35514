"""tools/isa_diff.py on two small listings written here (the shape of `hipcc -S --cuda-device-only` output; no compiler).  No GPU."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_diff  # noqa: E402


def kernel(name, ordinal, body, vgprs=24, spills=0, scratch=0):
    text = """\t.globl\t%(n)s ; -- Begin function %(n)s
\t.p2align\t8
\t.type\t%(n)s,@function
%(n)s: ; @%(n)s
; %%bb.0:
%(body)s
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.amdhsa_kernel %(n)s
\t\t.amdhsa_next_free_vgpr %(v)d
\t.end_amdhsa_kernel
\t.text
.Lfunc_end%(o)d:
\t.size\t%(n)s, .Lfunc_end%(o)d-%(n)s
; NumVgprs: %(v)d
""" % dict(n=name, o=ordinal, body=body.replace("@", str(ordinal)), v=vgprs)
    meta = """  - .agpr_count:     0
    .args:
      - .offset:         0
        .size:           272
    .name:           %s
    .private_segment_fixed_size: %d
    .sgpr_count:     18
    .sgpr_spill_count: 0
    .vgpr_count:     %d
    .vgpr_spill_count: %d
    .wavefront_size: 64
""" % (name, scratch, vgprs, spills)
    return text, meta


def listing(kernels, cuid):
    texts, metas = zip(*kernels)
    return ("\t.amdgcn_target \"amdgcn-amd-amdhsa--gfx950\"\n\t.text\n" + "".join(texts) +
            "\t.type\t__hip_cuid_%s,@object\n__hip_cuid_%s:\n\t.byte\t0\n\t.amdgpu_metadata\n---\namdhsa.kernels:\n" % (cuid, cuid) +
            "".join(metas) + "amdhsa.target:   amdgcn-amd-amdhsa--gfx950\n...\n\t.end_amdgpu_metadata\n")


# prologue (one compare and branch) | a loop with an MFMA block | an epilogue block with an MFMA outside any loop | the exit block
BODY = """\ts_load_dword s4, s[0:1], 0x10
\ts_waitcnt lgkmcnt(0)
\t%(cmp)s
\ts_mov_b32 s6, 0
\t%(br)s .LBB@_3
.LBB@_1: ; =>This Inner Loop Header: Depth=1
\tds_read_b128 v[0:3], v8
\ts_waitcnt lgkmcnt(0)
\tv_mfma_f32_16x16x32_bf16 v[4:7], v[0:3], v[10:13], v[4:7]
\t%(loop)s
\ts_cmp_lg_u32 s5, 0
\ts_cbranch_scc1 .LBB@_1
; %%bb.2:
\t%(pool)s
\tv_mfma_f32_16x16x32_f16 v[4:7], v[0:3], v[14:17], v[4:7]
.LBB@_3:
\t%(tail)s
\tglobal_store_dwordx4 v9, v[4:7], s[2:3]"""
PARENT = dict(cmp="s_cmp_gt_i32 s4, 0", br="s_cbranch_scc0", loop="s_add_i32 s5, s5, -1", pool="v_pk_add_f16 v0, v1, v2", tail="v_mov_b32_e32 v9, 0")


def body(**changes):
    return BODY % dict(PARENT, **changes)


@pytest.fixture(scope="module")
def tables():
    parent = listing([kernel("k_same", 0, body()), kernel("k_cold", 1, body()), kernel("k_tail", 2, body()), kernel("k_loop", 3, body()),
                      kernel("k_mfma", 4, body()), kernel("k_regs", 5, body()), kernel("k_spill", 6, body()), kernel("k_gone", 7, body())], "aaaa0001")
    # the commit's listing: another translation-unit id, the kernels in another order (other label ordinals), other comments
    commit = listing([kernel("k_mfma", 0, body(pool="v_pk_add_f16 v0, v2, v1")),
                      kernel("k_loop", 1, body(loop="s_sub_i32 s5, s5, 1")),
                      kernel("k_cold", 2, body(cmp="s_cmp_lt_i32 s4, 1", br="s_cbranch_scc1")),
                      kernel("k_tail", 3, body(tail="v_mov_b32_e32 v9, 0\n\ts_nop 0")),
                      kernel("k_same", 4, body().replace("Inner Loop Header", "Loop Header")),
                      kernel("k_regs", 5, body(), vgprs=25),
                      kernel("k_spill", 6, body(), spills=2, scratch=8),
                      kernel("k_new", 7, body())], "bbbb0002")
    return isa_diff.parse_listing(parent), isa_diff.parse_listing(commit), parent, commit


def test_figures_and_digest(tables):
    parent, commit, _, _ = tables
    assert sorted(parent) == ["k_cold", "k_gone", "k_loop", "k_mfma", "k_regs", "k_same", "k_spill", "k_tail"]
    r = parent["k_same"]
    assert (r["instrs"], r["vgprs"], r["sgprs"], r["spills"], r["scratch"]) == (16, 24, 18, 0, 0)
    assert (commit["k_spill"]["spills"], commit["k_spill"]["scratch"], commit["k_regs"]["vgprs"]) == (2, 8, 25)
    # comment lines, the function's ordinal in its labels and the translation unit's id do not reach the digest
    assert r["digest"] == commit["k_same"]["digest"] and r["body"] == commit["k_same"]["body"]
    assert not any(";" in l or "LBB4" in l for l in commit["k_same"]["body"])
    assert parent["k_cold"]["digest"] != commit["k_cold"]["digest"]


def test_verdicts(tables):
    parent, commit, _, _ = tables
    verdict = {k: isa_diff.compare(parent[k], commit[k])[0] for k in parent if k in commit}
    assert verdict == {"k_same": "A", "k_cold": "B", "k_tail": "C", "k_loop": "C", "k_mfma": "C", "k_regs": "C", "k_spill": "C"}
    # (k_tail: an instruction more is a changed figure; k_regs, k_spill: equal bodies, other register / spill figures)
    v, la, lb, at, ops = isa_diff.compare(parent["k_cold"], commit["k_cold"])
    assert (la, lb, at, len(ops)) == ("s_cmp_gt_i32 s4, 0", "s_cmp_lt_i32 s4, 1", 2, 2)
    assert isa_diff.compare(parent["k_loop"], commit["k_loop"])[1:3] == ("s_add_i32 s5, s5, -1", "s_sub_i32 s5, s5, 1")


def test_hot_lines(tables):
    parent = tables[0]
    lines = parent["k_same"]["body"]
    hot = isa_diff.hot_lines(lines)
    assert [l.strip() for l, h in zip(lines, hot) if not h][:4] == ["s_load_dword s4, s[0:1], 0x10", "s_waitcnt lgkmcnt(0)", "s_cmp_gt_i32 s4, 0",
                                                                     "s_mov_b32 s6, 0"]
    first_hot, last_hot = hot.index(True), len(hot) - 1 - hot[::-1].index(True)
    assert lines[first_hot].startswith(".LBB_1:") and "v_mfma_f32_16x16x32_f16" in lines[last_hot] and all(hot[first_hot:last_hot + 1])


def test_command_line(tables, tmp_path):
    _, _, parent, commit = tables
    a, b = tmp_path / "parent.s", tmp_path / "commit.s"
    a.write_text(parent)
    b.write_text(commit)
    tool = os.path.join(ROOT, "tools", "isa_diff.py")
    p = subprocess.run([sys.executable, tool, str(a), str(b), "--diff"], capture_output=True, text=True)
    assert p.returncode == 1
    out = p.stdout
    assert "  A: identical, " in out and "  B: 2 differing stretches" in out and out.count("  C: ") == 5
    assert "only in the parent's listing" in out and "only in the commit's listing" in out
    assert "-\ts_cmp_gt_i32 s4, 0" in out and "+\ts_cmp_lt_i32 s4, 1" in out
    same = subprocess.run([sys.executable, tool, str(a), str(a)], capture_output=True, text=True)
    assert same.returncode == 0 and same.stdout.count("  A: identical") == 8
