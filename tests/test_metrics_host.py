"""roomnet_amd.metrics against scikit-learn, whose accuracy_score and precision_recall_fscore_support the reference's training loop
records at every validation point (train.py:146-147).  Every figure is a ratio of small integers in [0, 1]; the two sides may order a
division and a product differently, which costs a few ulps of 1.1e-16: the bound is 1e-12."""
import numpy as np
import pytest

from roomnet_amd import metrics

pytest.importorskip("sklearn")
sklearn_metrics = pytest.importorskip("sklearn.metrics")

TOL = 1e-12


def _vectors(case):
    """``(y_true, y_pred, num_classes, per-class list length)`` of a seeded case."""
    rng = np.random.default_rng(20)
    if case == "six":
        return rng.integers(0, 6, 200), rng.integers(0, 6, 200), 6, 6
    if case == "three":
        return rng.integers(0, 3, 41), rng.integers(0, 3, 41), 3, 3
    if case == "absent_from_labels":                     # class 4 is predicted and never a label: recall 0, support 0
        y = rng.integers(0, 4, 120)
        p = rng.integers(0, 5, 120)
        p[:3] = 4
        return y, p, 6, 5
    if case == "never_predicted":                        # class 2 is a label and never predicted: precision 0
        y = rng.integers(0, 3, 90)
        y[:4] = 2
        p = rng.integers(0, 2, 90)
        return y, p, 3, 3
    if case == "absent_from_both":                       # class 3 of six occurs nowhere: its list entry vanishes
        y = rng.choice([0, 1, 2, 4, 5], 150)
        p = rng.choice([0, 1, 2, 4, 5], 150)
        return y, p, 6, 5
    raise AssertionError(case)


CASES = ("six", "three", "absent_from_labels", "never_predicted", "absent_from_both")


@pytest.mark.parametrize("case", CASES)
def test_confusion_matrix_is_sklearns(case):
    y, p, nc, _ = _vectors(case)
    cm = metrics.confusion_matrix(y, p, nc)
    want = sklearn_metrics.confusion_matrix(y, p, labels=list(range(nc)))
    assert cm.shape == (nc, nc) and np.array_equal(cm, want) and cm.sum() == len(y)


@pytest.mark.parametrize("case", CASES)
def test_stats_from_confusion_are_sklearns(case):
    y, p, nc, length = _vectors(case)
    got = metrics.stats_from_confusion(metrics.confusion_matrix(y, p, nc))
    assert sorted(got) == ["accuracy", "f-scores", "precisions", "recalls", "support"]
    acc = sklearn_metrics.accuracy_score(y, p)
    prec, rec, fsc, supp = sklearn_metrics.precision_recall_fscore_support(y, p, zero_division=0)
    assert len(prec) == length
    assert abs(got["accuracy"] - acc) <= TOL
    for key, want in (("precisions", prec), ("recalls", rec), ("f-scores", fsc)):
        assert len(got[key]) == length, key
        assert np.abs(np.asarray(got[key]) - want).max() <= TOL, key
        assert all(isinstance(v, float) for v in got[key])
    assert got["support"] == [int(v) for v in supp]


def test_the_special_classes_give_the_zeros_they_should():
    y, p, nc, _ = _vectors("absent_from_labels")
    s = metrics.stats_from_confusion(metrics.confusion_matrix(y, p, nc))
    assert s["recalls"][4] == 0.0 and s["support"][4] == 0 and s["f-scores"][4] == 0.0
    y, p, nc, _ = _vectors("never_predicted")
    s = metrics.stats_from_confusion(metrics.confusion_matrix(y, p, nc))
    assert s["precisions"][2] == 0.0 and s["support"][2] >= 4 and s["f-scores"][2] == 0.0


def test_bad_arguments_raise():
    with pytest.raises(ValueError):
        metrics.confusion_matrix([0, 1], [0], 3)
    with pytest.raises(ValueError):
        metrics.confusion_matrix([0, 3], [0, 1], 3)
    with pytest.raises(ValueError):
        metrics.stats_from_confusion(np.zeros((3, 3), np.int64))
    with pytest.raises(ValueError):
        metrics.stats_from_confusion(np.zeros((2, 3), np.int64))
