"""Classification figures from a confusion matrix: what the reference's training loop records at every validation point
(train.py:146-152: ``sklearn.metrics.accuracy_score`` and ``precision_recall_fscore_support``), stated in NumPy so that the
confusion matrices ``rn_ft_run_validated`` reduces on the GPU become the reference's ``all_train_stats.json`` entries.  Pure host
code; scikit-learn is not needed."""
from __future__ import annotations

import numpy as np

# the keys of one entry of the reference's all_train_stats.json (train.py:149-152), which plotter.py reads
REFERENCE_KEYS = ("step", "accuracy", "precisions", "recalls", "f-scores")


def confusion_matrix(y_true, y_pred, num_classes) -> np.ndarray:
    """int64 ``[num_classes, num_classes]``: entry ``[t, p]`` counts the items of label ``t`` predicted as ``p`` (row = label,
    column = predicted class, as ``sklearn.metrics.confusion_matrix(..., labels=range(num_classes))``)."""
    nc = int(num_classes)
    t = np.asarray(y_true).reshape(-1).astype(np.int64)
    p = np.asarray(y_pred).reshape(-1).astype(np.int64)
    if t.shape != p.shape:
        raise ValueError("confusion_matrix: %d labels and %d predictions" % (t.size, p.size))
    if nc < 1 or (t.size and (min(t.min(), p.min()) < 0 or max(t.max(), p.max()) >= nc)):
        raise ValueError("confusion_matrix: a class outside [0, %d)" % nc)
    return np.bincount(t * nc + p, minlength=nc * nc).reshape(nc, nc)


def _ratio(num, den):
    """``num / den`` with 0 where ``den`` is 0 (sklearn's ``zero_division=0``)."""
    num = num.astype(np.float64)
    den = den.astype(np.float64)
    return np.where(den > 0, num / np.where(den > 0, den, 1.0), 0.0)


def stats_from_confusion(cm) -> dict:
    """``{'accuracy', 'precisions', 'recalls', 'f-scores', 'support'}`` of a confusion matrix (row = label, column = predicted):
    the numbers ``sklearn.metrics.accuracy_score`` and ``precision_recall_fscore_support(..., zero_division=0)`` give for the same
    predictions.  The per-class lists cover the classes that occur in the labels or in the predictions, in ascending order
    (sklearn's ``labels=None``); precision is TP / predicted, recall TP / support, F-score 2 TP / (predicted + support), each 0
    where its denominator is."""
    cm = np.asarray(cm)
    if cm.ndim != 2 or cm.shape[0] != cm.shape[1] or cm.size == 0 or (cm < 0).any():
        raise ValueError("stats_from_confusion: expected a square matrix of counts, got shape %s" % (cm.shape,))
    cm = cm.astype(np.int64)
    total = int(cm.sum())
    if total < 1:
        raise ValueError("stats_from_confusion: the matrix counts no item")
    tp, support, predicted = np.diagonal(cm), cm.sum(1), cm.sum(0)
    present = (support + predicted) > 0
    tp, support, predicted = tp[present], support[present], predicted[present]
    return {"accuracy": float(np.diagonal(cm).sum()) / float(total),
            "precisions": [float(v) for v in _ratio(tp, predicted)],
            "recalls": [float(v) for v in _ratio(tp, support)],
            "f-scores": [float(v) for v in _ratio(2 * tp, predicted + support)],
            "support": [int(v) for v in support]}


def append_stats(stats_fpath, entries) -> list:
    """Append ``entries`` (dicts; only ``REFERENCE_KEYS`` are kept) to the JSON list in ``stats_fpath`` the way train.py:129-155
    keeps ``all_train_stats.json``: the list is loaded if the file exists, extended, and dumped with ``indent=4, sort_keys=True``.
    Returns the whole list."""
    import json
    import os
    if os.path.isfile(stats_fpath):
        with open(stats_fpath, "r") as f:
            everything = json.load(f)
        if not isinstance(everything, list):
            raise ValueError("append_stats: %r does not hold a JSON list" % (stats_fpath,))
    else:
        everything = []
    for e in entries:
        everything.append({"step": int(e["step"]), "accuracy": float(e["accuracy"]),
                           "precisions": [float(v) for v in e["precisions"]], "recalls": [float(v) for v in e["recalls"]],
                           "f-scores": [float(v) for v in e["f-scores"]]})
    with open(stats_fpath, "w") as f:
        json.dump(everything, f, indent=4, sort_keys=True)
    return everything
