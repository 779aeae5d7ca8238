"""Binary classification metrics of the classification entry points — the reference's MetricAccumulator(type="cls") (src/utils/tools.py:208-226 of the
reference: torchmetrics Accuracy / Precision / Recall / F1Score / AUROC, task="binary", on p1 = softmax(logits)[:, 1]), kept in a class of its own so that
MetricAccumulator(type="cls") keeps raising.

update() keeps copies of the logits and labels on the device (the loop's batches live in the prefetcher's reused slots).  compute() concatenates them,
runs the criterion over the whole split, takes p1 and hands it to `uia_binary_cls_stats` (TP / FP / TN / FN at p1 > 0.5, exact tie-aware AUROC, fp64); the loss and that record come to the host in ONE copy.  Zero
denominators give 0, as torchmetrics does; AUROC is 0.0 when a class is absent (torchmetrics' binary ROC then has an all-zero axis)."""
import logging

import torch


def metrics_from_counts(tp, fp, tn, fn):
    """acc / pre / rec / f1 of the binary task from the four counts; a zero denominator gives 0."""
    n = tp + fp + tn + fn
    acc = (tp + tn) / n if n else 0.0
    pre = tp / (tp + fp) if tp + fp else 0.0
    rec = tp / (tp + fn) if tp + fn else 0.0
    f1 = 2 * tp / (2 * tp + fp + fn) if 2 * tp + fp + fn else 0.0
    return {"acc": acc, "pre": pre, "rec": rec, "f1": f1}


class ClassificationMetrics:
    KEYS = ("acc", "rec", "pre", "f1", "auc", "loss")

    def __init__(self, criterion=None, num_classes=2):
        if num_classes != 2:
            raise NotImplementedError(f"ClassificationMetrics: num_classes={num_classes}; the reference's metrics are torchmetrics' binary task")
        self.criterion, self.num_classes = criterion, num_classes
        self.reset()

    def reset(self):
        self._logits, self._labels = [], []

    def update(self, preds, labels):
        """Copies both: the loop's batches are views of engine.DevicePrefetcher's ring slots, which later batches overwrite before compute() runs."""
        self._logits.append(preds.detach().clone())
        self._labels.append(labels.detach().reshape(-1).clone())

    def compute(self):
        if not self._logits:
            return {k: float("nan") for k in self.KEYS}
        from uia_hip import ops
        logits = torch.cat(self._logits).float()
        labels = torch.cat(self._labels).to(torch.int64)
        loss = self.criterion(logits, labels).detach().double().reshape(1)
        p1 = torch.softmax(logits, dim=1)[:, 1]
        rec = ops.binary_cls_stats(p1, labels)
        host = torch.cat([loss, rec]).cpu().tolist()           # one device-to-host copy
        loss_v, (tp, fp, tn, fn, auc) = host[0], host[1:]
        if any(v != v for v in (tp, fp, tn, fn)):
            raise ValueError("ClassificationMetrics: labels outside {0, 1}")
        out = metrics_from_counts(tp, fp, tn, fn)
        out.update(auc=auc, loss=loss_v)
        return out

    def roc(self):
        """(fpr fp64, tpr fp64, thresholds fp32) of what was accumulated, device tensors: the exact curve of torchmetrics ROC(task="binary") on
        p1 = softmax(logits)[:, 1] (`uia_binary_roc_curve`: point 0 is (0, 0, 1.0), then one point per distinct score, descending).  One host read: the
        number of points."""
        if not self._logits:
            raise ValueError("ClassificationMetrics.roc: nothing accumulated")
        from uia_hip import ops
        logits = torch.cat(self._logits).float()
        labels = torch.cat(self._labels).to(torch.int64)
        count, fpr, tpr, thr = ops.binary_roc_curve(torch.softmax(logits, dim=1)[:, 1], labels)
        n = int(count.item())
        if n < 0:
            raise ValueError("ClassificationMetrics.roc: labels outside {0, 1} or a NaN score")
        return fpr[:n], tpr[:n], thr[:n]


def report_cls_test(args, stats, saved_best, rank=0):
    """The tail of the classification entry points' test() (reference biomedclip/classification.py:329-363): the Metric / Mean table (percent, %.2f) to
    the log, then runs/<exp>/<dataset>/test/<time>_acc=<acc>/ with results.csv, a copy of the checkpoint, the viz folder and the log."""
    from src.utils.tools import backup_test_run
    rows = [("Acc", stats["acc"] * 100), ("Rec", stats["rec"] * 100), ("Pre", stats["pre"] * 100), ("F1", stats["f1"] * 100), ("AUC", stats["auc"] * 100)]
    table = f"{'Metric':>6} {'Mean':>6}\n" + "".join(f"{m:>6} {a:6.2f}\n" for m, a in rows)
    logging.info(f"\n{'=' * 50}\n" + table + f"{'=' * 50}\n")
    if rank != 0:
        return None
    lines = ["Metric,Mean"] + [f"{m},{a:.2f}" for m, a in rows]
    return backup_test_run(args, f"acc={stats['acc'] * 100:.2f}", lines, saved_best)
