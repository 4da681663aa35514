"""Host side of validation inside a fine-tuning run: the point schedule, fine_tune's argument checks (raised before any library
call) and the writer of the reference's all_train_stats.json format.  No GPU."""
import json

import numpy as np
import pytest

from roomnet_amd import _capi, finetune, infer, metrics
from roomnet_amd.network import RoomNet


def test_validation_steps():
    assert finetune.validation_steps(0, 7, 3) == [3, 6, 7]
    assert finetune.validation_steps(7, 5, 2) == [8, 10, 12]
    assert finetune.validation_steps(0, 6, 3) == [3, 6]
    assert finetune.validation_steps(5, 1, 10) == [6]
    for bad in (0, -1):
        with pytest.raises(ValueError, match="val_every"):
            finetune.validation_steps(0, 5, bad)
    with pytest.raises(ValueError):
        finetune.validation_steps(0, 0, 2)


def test_the_binding_knows_the_new_symbols():
    assert _capi.RN_FT_BEST == 4
    for name in ("rn_ft_val_points", "rn_ft_run_validated", "rn_ft_best"):
        assert name in _capi.EXPORTED_SYMBOLS


@pytest.fixture()
def no_library(monkeypatch):
    """Any attempt to load the library or to build a trainer fails the test."""
    def refuse(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_capi, "load_library", refuse)
    monkeypatch.setattr(_capi, "Trainer", refuse)


def test_fine_tune_argument_errors_come_before_any_library_call(no_library):
    net = RoomNet(6, im_side=224, compute_bn_mean_var=False, dtype="f32", max_batch=8)
    feats, labels = np.zeros((2, 21, 21, 16), np.float32), [0, 1]
    with pytest.raises(ValueError, match="val_every"):
        net.fine_tune(feats, labels, steps=1, val_every=2)                              # no val
    with pytest.raises(ValueError, match="keep"):
        net.fine_tune(feats, labels, steps=1, val=(feats, labels), val_every=2, keep="first")
    with pytest.raises(ValueError, match="keep"):
        net.fine_tune(feats, labels, steps=1, keep=None)
    with pytest.raises(ValueError, match="val_every"):
        net.fine_tune(feats, labels, steps=1, val=(feats, labels), val_every=0)
    with pytest.raises(ValueError, match="val_every"):
        net.fine_tune(feats, labels, steps=1, val=(feats, labels), val_every=-3)


def _history():
    out = []
    for step, cm in ((10, [[3, 1, 0], [0, 2, 0], [1, 0, 0]]), (20, [[4, 0, 0], [0, 2, 0], [0, 0, 1]])):
        e = {"step": step, "loss": 1.5, "confusion": np.asarray(cm, np.int32)}
        e.update((k, v) for k, v in metrics.stats_from_confusion(cm).items() if k != "support")
        out.append(e)
    return out


def test_append_stats_keeps_the_reference_keys_and_appends(tmp_path):
    path = tmp_path / "all_train_stats.json"
    earlier = [{"step": 5, "accuracy": 0.25, "precisions": [0.5], "recalls": [0.5], "f-scores": [0.5]}]
    path.write_text(json.dumps(earlier))
    everything = metrics.append_stats(str(path), _history())
    on_disk = json.loads(path.read_text())
    assert on_disk == everything and len(on_disk) == 3 and on_disk[0] == earlier[0]
    for entry in on_disk:
        assert sorted(entry) == sorted(metrics.REFERENCE_KEYS) == ["accuracy", "f-scores", "precisions", "recalls", "step"]
    assert [e["step"] for e in on_disk] == [5, 10, 20]
    assert on_disk[2]["accuracy"] == 1.0 and on_disk[1]["accuracy"] == pytest.approx(5 / 7)
    # the reference's format: indent 4, sorted keys
    assert path.read_text() == json.dumps(on_disk, indent=4, sort_keys=True)
    fresh = tmp_path / "new.json"
    assert len(metrics.append_stats(str(fresh), _history()[:1])) == 1 and len(json.loads(fresh.read_text())) == 1


def test_fine_tune_from_list_passes_the_arguments_and_writes_the_stats(tmp_path, monkeypatch):
    history = _history()
    seen = {}

    class Net:
        def fine_tune(self, feats, labels, steps, **kw):
            seen.update(kw, steps=steps)
            return {"losses": np.zeros(steps, np.float32), "val_history": history, "best_step": 20}

        def extract_features(self, ims, depth=2):
            return np.zeros((len(ims), 21, 21, 16), np.float32)

    lst = tmp_path / "list.txt"
    lst.write_text("a.jpg 0\nb.jpg 1\n")
    monkeypatch.setattr(infer, "_decode_files", lambda fpaths, n: ((i, f, np.zeros((4, 4, 3), np.uint8)) for i, f in enumerate(fpaths)))
    stats = tmp_path / "stats.json"
    out = infer.fine_tune_from_list(Net(), str(lst), 3, val_list_fpath=str(lst), val_every=10, keep="best", stats_fpath=str(stats))
    assert out["best_step"] == 20
    assert seen["val_every"] == 10 and seen["keep"] == "best" and seen["steps"] == 3 and seen["val"] is not None
    assert [e["step"] for e in json.loads(stats.read_text())] == [10, 20]
    with pytest.raises(ValueError, match="val_every"):
        infer.fine_tune_from_list(Net(), str(lst), 3, stats_fpath=str(stats))
