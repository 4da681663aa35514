"""profiles/finetune_views_timing.json (tools/bench_finetune.py --views) is the measurement README.md and DESIGN.md section 21 quote."""
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_views_timing_is_the_one_the_documents_quote():
    doc = json.load(open(os.path.join(ROOT, "profiles", "finetune_views_timing.json")))
    cases = {c["depth"]: c for c in doc["cases"]}
    assert sorted(cases) == [2, 3]
    readme = open(os.path.join(ROOT, "README.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for depth, c in cases.items():
        assert (c["side"], c["dtype"], c["batch"], c["runs"]) == (224, "bf16", 45, 3)
        for arm in ("cached", "views", "views_other"):            # views_other: the one-slot build of the A/B
            a = c[arm]
            assert 0 < a["us_per_step_min"] <= a["us_per_step"] <= a["us_per_step_max"]
            for text in (readme, design):
                assert "%d us" % round(a["us_per_step"]) in text, (depth, arm, a["us_per_step"])
        assert c["views"]["us_per_step"] > c["cached"]["us_per_step"]
        assert 0 < c["view_launch_us"]["median"] < c["feature_pass_us"]["median"]
        # the second feature slot ships because it is not slower, and faster outside the spread where the ranges do not overlap
        assert c["views"]["us_per_step_min"] <= c["views_other"]["us_per_step_max"]
        assert c["views_ranges_overlap"] == (c["views"]["us_per_step_max"] >= c["views_other"]["us_per_step_min"]
                                             and c["views_other"]["us_per_step_max"] >= c["views"]["us_per_step_min"])
    assert not cases[2]["views_ranges_overlap"] and cases[2]["views"]["us_per_step"] < cases[2]["views_other"]["us_per_step"]
