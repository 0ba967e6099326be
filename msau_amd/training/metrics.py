"""Evaluation metrics from a confusion matrix (rows = labels, columns = predictions), e.g. `MSAUWrapper.confusion_matrix`.

The reference keeps every labelled pixel's (label, prediction) pair on the host and calls sklearn
(train_chargrid_funsd_msau.py:147-161).  A confusion matrix holds the same information, so the numbers and the printed report
follow from it without the pairs:

  scores(cm)                               {"prec", "recall", "acc"}: micro precision = micro recall = accuracy (sklearn's
                                           semantics for single-label multi-class data), as `evaluate` returns them
  classification_report(cm, target_names)  the text of sklearn.metrics.classification_report(labels, preds, target_names=...)

One deviation: sklearn raises ValueError when the number of classes present in labels or predictions differs from the number
of `target_names`.  In the reference that can happen (the classes come from the data, and a remapped "other" may add or hide
one); here the report is printed with class indices instead, after one line that says so, and training goes on.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np


def _as_counts(cm) -> np.ndarray:
    if hasattr(cm, "detach"):
        cm = cm.detach().cpu().numpy()
    cm = np.asarray(cm)
    if cm.ndim != 2 or cm.shape[0] != cm.shape[1]:
        raise ValueError(f"a confusion matrix is square, got shape {cm.shape}")
    if cm.dtype.kind not in "iu" or (cm < 0).any():
        raise ValueError("a confusion matrix holds non-negative integer counts")
    return cm.astype(np.int64)


def scores(cm) -> Dict[str, float]:
    """{"prec", "recall", "acc"} of the counted pixels; 0.0 each when nothing was counted"""
    cm = _as_counts(cm)
    total = int(cm.sum())
    acc = int(np.trace(cm)) / total if total else 0.0
    return {"prec": acc, "recall": acc, "acc": acc}


def _divide(num: np.ndarray, den: np.ndarray) -> np.ndarray:
    """num / den with 0.0 where den == 0 (sklearn's zero_division default, without the warning)"""
    out = np.zeros(num.shape, dtype=np.float64)
    np.divide(num, den, out=out, where=den != 0)
    return out


def classification_report(cm, target_names: Optional[Sequence[str]] = None, digits: int = 2) -> str:
    """sklearn.metrics.classification_report's text for the (label, prediction) pairs that `cm` counts: one row per class that
    occurs in the labels or the predictions, then accuracy, macro avg and weighted avg; 0.00 where a ratio divides by zero."""
    cm = _as_counts(cm)
    true_all, pred_all = cm.sum(axis=1), cm.sum(axis=0)
    classes = np.flatnonzero((true_all > 0) | (pred_all > 0))
    if classes.size == 0:
        return "no labelled pixels were counted\n"
    note = ""
    if target_names is None:
        names = [str(int(c)) for c in classes]
    elif len(target_names) != classes.size:
        note = (f"classification_report: {classes.size} classes occur in labels or predictions but {len(target_names)} "
                f"target names were given: printing class indices\n")
        names = [str(int(c)) for c in classes]
    else:
        names = [str(n) for n in target_names]
    sub = cm[np.ix_(classes, classes)]
    tp = np.diag(sub).astype(np.int64)
    true_sum, pred_sum = true_all[classes], pred_all[classes]
    precision = _divide(tp, pred_sum)
    recall = _divide(tp, true_sum)
    f1 = _divide(2.0 * tp, true_sum.astype(np.float64) + pred_sum.astype(np.float64))
    support = int(true_sum.sum())
    # sklearn's supports come out of multilabel_confusion_matrix, whose counts are float64 when no pixel is a true positive:
    # then its report prints them as "1.0"
    num = float if int(tp.sum()) == 0 else int

    headers = ["precision", "recall", "f1-score", "support"]
    width = max(max(len(n) for n in names), len("weighted avg"), digits)
    head_fmt = "{:>{width}s} " + " {:>9}" * len(headers)
    report = head_fmt.format("", *headers, width=width) + "\n\n"
    row_fmt = "{:>{width}s} " + " {:>9.{digits}f}" * 3 + " {:>9}\n"
    for i, name in enumerate(names):
        report += row_fmt.format(name, precision[i], recall[i], f1[i], num(true_sum[i]), width=width, digits=digits)
    report += "\n"
    acc = float(tp.sum()) / float(cm.sum())
    acc_fmt = "{:>{width}s} " + " {:>9.{digits}}" * 2 + " {:>9.{digits}f}" + " {:>9}\n"
    report += acc_fmt.format("accuracy", "", "", acc, num(support), width=width, digits=digits)
    report += row_fmt.format("macro avg", float(np.average(precision)), float(np.average(recall)), float(np.average(f1)),
                             num(support), width=width, digits=digits)
    if support > 0:
        w = [float(np.average(v, weights=true_sum)) for v in (precision, recall, f1)]
    else:
        w = [0.0, 0.0, 0.0]
    report += row_fmt.format("weighted avg", *w, num(support), width=width, digits=digits)
    return note + report
