"""The plan of the float32 matrix-core stages, pinned on the CPU.

rn_f32m_plan exports the pure per-stage planner of rn_stage_f32m.hip: kernel kind, variant-table row and launch geometry from a
stage's shape, the input channels it contracts and the couts it does not convolve.  The stage kernels' LDS is all dynamic, which
no kernel trace shows, and a wrong tile count costs speed or -- past the LDS -- the launch.  tests/golden/f32m_plan.json was
recorded from the planning code as it stood inline in rn_f32m_prepare (the commit its header names); the planner must return the
same plan for every row.  The take-back rules the fixture cannot record (no handle reaches them on the shipped checkpoint) are
stated from that code's rules."""
import ctypes as C
import json
import os

import pytest

import checkpoints
from conftest import ROOT
from roomnet_amd import _capi
from roomnet_amd.graph import build_graph

FIXTURE = os.path.join(ROOT, "tests", "golden", "f32m_plan.json")
SIDES = (190, 224, 300, 420, 600)
COLUMNS = ["im_side", "stage", "cin", "cout", "pool_k", "pool_s", "residual", "in_side", "out_side", "live_cin", "frozen_couts", "kind",
           "variant", "live_cin_contracted", "npt", "ringcols", "lds", "n_colblocks", "n_ctg", "threads"]


def _rows():
    with open(FIXTURE) as f:
        fx = json.load(f)
    assert fx["columns"] == COLUMNS
    assert "commit" in fx["recorded_from"]
    return [dict(zip(COLUMNS, r)) for r in fx["rows"]]


def _plan_of_stage(s, **kw):
    return _capi.f32m_plan(s.cin, s.cout, s.pool_k, s.pool_s, s.skip_stage >= 0, s.in_side, s.out_side, **kw)


def test_fixture_covers_stages_1_to_8_at_every_side_and_the_two_fold_rows():
    rows = _rows()
    plain = {(r["im_side"], r["stage"]) for r in rows if r["live_cin"] == r["cin"] and r["frozen_couts"] == 0}
    assert plain == {(side, stage) for side in SIDES for stage in range(1, 9)}
    # every row is a stage of the graph at that side
    for r in rows:
        s = build_graph(6, r["im_side"]).stages[r["stage"]]
        assert (s.cin, s.cout, s.pool_k, s.pool_s, int(s.skip_stage >= 0), s.in_side, s.out_side) == tuple(
            r[k] for k in ("cin", "cout", "pool_k", "pool_s", "residual", "in_side", "out_side")), r
    assert any(r["stage"] == 3 and r["live_cin"] == 16 and r["kind"] == "wide" and r["im_side"] == 224 for r in rows)
    assert any(r["stage"] == 2 and r["frozen_couts"] == 16 and r["kind"] == "m16" and r["im_side"] == 224 for r in rows)


def test_plan_matches_the_recorded_stages():
    wrong = []
    for r in _rows():
        got = _capi.f32m_plan(r["cin"], r["cout"], r["pool_k"], r["pool_s"], bool(r["residual"]), r["in_side"], r["out_side"],
                              live_cin=r["live_cin"], frozen_couts=r["frozen_couts"])
        want = {k: r[k] for k in ("kind", "variant", "frozen_couts", "npt", "ringcols", "lds", "n_colblocks", "n_ctg", "threads")}
        want["live_cin"] = r["live_cin_contracted"]
        if got != want:
            wrong.append((r, got))
    assert not wrong, "%d rows differ, the first: %s" % (len(wrong), wrong[:2])


def test_lds_and_workgroup_stay_inside_the_chip():
    for side in SIDES + (186, 1000):
        for s in build_graph(6, side).stages[1:]:
            p = _plan_of_stage(s)
            if p["kind"] != "off":
                assert 0 < p["lds"] <= 160 * 1024 and 64 <= p["threads"] <= 1024 and p["npt"] * p["n_colblocks"] >= 1, (side, s.index, p)


def test_residual_fold_drops_the_frozen_cout_tile_only():
    s5 = build_graph(6, 224).stages[5]
    full, fold = _plan_of_stage(s5), _plan_of_stage(s5, frozen_couts=32)
    assert full["n_ctg"] == 2 and fold["n_ctg"] == 1 and fold["frozen_couts"] == 32
    assert {k: v for k, v in fold.items() if k not in ("n_ctg", "frozen_couts")} == {k: v for k, v in full.items() if k not in ("n_ctg", "frozen_couts")}
    # (a count that leaves no whole 32-cout tile is not folded)
    assert _plan_of_stage(s5, frozen_couts=24) == full


def test_input_channel_fold_is_taken_back_where_no_variant_contracts_that_count():
    g = build_graph(6, 224)
    s3, s9 = g.stages[3], g.stages[9]
    full = _plan_of_stage(s3)
    assert _plan_of_stage(s3, live_cin=16)["live_cin"] == 16
    for live in (8, 24):                       # residual consumer, a count no variant contracts: every channel is contracted
        assert _plan_of_stage(s3, live_cin=live) == full and full["live_cin"] == 32
    # a consumer no variant exists for at all is not covered, whatever its live channels
    assert _plan_of_stage(s9)["kind"] == "off" and _plan_of_stage(s9, live_cin=8)["kind"] == "off"
    # residual stage 5 with 56 live input channels (8 frozen ones in stage 4): no variant either
    assert _plan_of_stage(g.stages[5], live_cin=56) == _plan_of_stage(g.stages[5])


def test_producer_without_a_16_cout_variant_convolves_every_channel():
    g = build_graph(6, 224)
    assert _plan_of_stage(g.stages[2], frozen_couts=16)["kind"] == "m16"
    for s in (g.stages[1], g.stages[4]):       # 8 -> 32 and 32 -> 64: no 16-cout variant with frozen couts
        assert _plan_of_stage(s, frozen_couts=16) == _plan_of_stage(s)
    assert _plan_of_stage(g.stages[2], frozen_couts=8) == _plan_of_stage(g.stages[2])


def test_take_back_checkpoint_lands_the_fold_on_stage_9(weights):
    """The checkpoint of the GPU take-back case (tests/test_hip_f32.py): by the planner's inequality stages 2, 4 and 5 freeze
    nothing and stage 8 freezes 11 channels, so the input-channel fold is proposed for stage 9 with 8 live channels -- which no
    kernel covers.  (Stage 4's frozen channels can never fold: its output is stage 5's skip tensor.)"""
    g = build_graph(6, 224)
    w = checkpoints.take_back_stage9(g, weights)
    frozen = [len(checkpoints.f32_frozen_channels(w, s.bn_name)) for s in g.stages]
    assert frozen[2] == 0 and frozen[4] == 0 and frozen[5] == 0 and frozen[8] == 11, frozen
    # producers in front of stage 8 that could take the fold: a pooled stage without a skip whose output nobody's residual reads
    skip_sources = {s.skip_stage for s in g.stages}
    for s in g.stages[:8]:
        takes = s.skip_stage < 0 and s.pool_k == 4 and s.index not in skip_sources and 8 <= frozen[s.index] // 8 * 8 < s.cout
        assert not takes, s.index
    assert g.stages[8].skip_stage < 0 and g.stages[8].pool_k == 4 and 8 not in skip_sources
    assert _plan_of_stage(g.stages[9], live_cin=16 - frozen[8] // 8 * 8)["kind"] == "off"


def test_plan_rejects_bad_arguments():
    lib = _capi.load_library()
    p = _capi.rn_f32m_stage_plan()
    assert lib.rn_f32m_plan(32, 32, 4, 1, 0, 215, 210, 32, 0, None) == -1
    assert lib.rn_f32m_plan(30, 32, 4, 1, 0, 215, 210, 30, 0, C.byref(p)) == -1          # channels in eights
    assert lib.rn_f32m_plan(32, 32, 4, 1, 0, 215, 210, 40, 0, C.byref(p)) == -1          # live_cin above cin
    assert lib.rn_f32m_plan(32, 32, 4, 1, 0, 215, 210, 32, 32, C.byref(p)) == -1         # every cout frozen
    assert b"rn_f32m_plan" in lib.rn_last_error()
    with pytest.raises(ValueError):
        _capi.f32m_plan(32, 32, 4, 0, False, 215, 210)
