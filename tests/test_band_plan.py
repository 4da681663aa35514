"""The launch geometry of the forward pass, pinned on the CPU.

Bands cut the rows of an image into workgroups and change no output bit, so no result test notices a slip in the band
picker (roomnet_amd/csrc/rn_bands.h): it would only cost speed.  tests/golden/band_plan.json was recorded from the searches
as they stood inline in rn_fused_forward and rn_f32m_launch (the commit its header names), with every stage's real
out_side, column blocks, workgroups per CU and pooling at image sides 224, 300 and 600; rn_band_plan -- the export of the
functions the forward pass calls -- must return the same rows_per_band and n_bands for every row."""
import json
import os

from conftest import ROOT
from roomnet_amd import _capi

FIXTURE = os.path.join(ROOT, "tests", "golden", "band_plan.json")
BATCHES = (1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128, 160, 192, 256, 384, 512)
SIDES = (224, 300, 600)
# n_cu plays no part in the two closed forms: recorded at 256 only
CLOSED_FORMS = ("stage0", "generic")


def _rows():
    with open(FIXTURE) as f:
        fx = json.load(f)
    assert fx["columns"] == ["family", "im_side", "n", "n_cu", "out_side", "n_colblocks", "wgs_per_cu", "pool_k", "pool_s",
                             "rows_per_band", "n_bands"]
    return fx["rows"]


def test_fixture_covers_every_family_side_batch_and_chip():
    rows = _rows()
    have = {(r[0], r[1], r[2], r[3]) for r in rows}
    for family in _capi.BAND_FAMILIES:
        for side in SIDES:
            for n in BATCHES:
                for n_cu in (256,) if family in CLOSED_FORMS else (256, 128):
                    assert (family, side, n, n_cu) in have, "no fixture row for %s at side %d, n %d, n_cu %d" % (family, side, n, n_cu)
    # the variants the issue names: register-weights workgroups one and four per CU, rn_conv16p's 3-wave (two per CU) and 5-wave (one) forms
    assert {r[6] for r in rows if r[0] == "rw"} == {1, 4}
    assert {r[6] for r in rows if r[0] == "conv16p"} == {1, 2}
    assert {r[7] for r in rows if r[0] == "rw"} == {0, 4}                  # ... and the un-pooled stage with its 4-row floor


def test_band_plan_matches_the_recorded_geometry():
    rows = _rows()
    assert len(rows) > 2000
    wrong = []
    for family, _side, n, n_cu, out_side, n_colblocks, wgs_per_cu, pool_k, pool_s, rows_per_band, n_bands in rows:
        got = _capi.band_plan(family, n, n_cu, out_side, n_colblocks, wgs_per_cu, pool_k, pool_s)
        if got != (rows_per_band, n_bands):
            wrong.append((family, n, n_cu, out_side, n_colblocks, wgs_per_cu, pool_k, pool_s, (rows_per_band, n_bands), got))
    assert not wrong, "%d of %d rows differ, the first: %s" % (len(wrong), len(rows), wrong[:5])


def test_band_plan_rejects_bad_arguments():
    lib = _capi.load_library()
    import ctypes as C
    r, b = C.c_int(0), C.c_int(0)
    assert lib.rn_band_plan(99, 1, 256, 100, 1, 1, 0, 1, C.byref(r), C.byref(b)) == -1           # unknown family
    assert lib.rn_band_plan(_capi.BAND_FAMILIES["pair"], 0, 256, 100, 1, 1, 0, 1, C.byref(r), C.byref(b)) == -1
    assert lib.rn_band_plan(_capi.BAND_FAMILIES["pair"], 1, 256, 100, 1, 1, 0, 1, None, C.byref(b)) == -1
    assert b"rn_band_plan" in lib.rn_last_error()
