"""Per-class classification metrics of the downstream loop on the host: torchmetrics' MulticlassAccuracy and MulticlassAUROC
with average=None (engine_downstream.py:287-296), which the reference computes on softmax probabilities.  A class with no
sample in the targets scores 0.0 for accuracy, a class without a positive or without a negative sample 0.0 for AUROC, as
torchmetrics does.  `MultilabelMetrics` (an addition of this build) scores the sigmoid outputs of multi-label fine-tuning per
label, on the entries whose label is known."""
from __future__ import annotations

import numpy as np
import torch


def _np(t) -> np.ndarray:
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def multiclass_accuracy(probs, target, num_classes: int) -> np.ndarray:
    """Per-class accuracy (recall): share of the samples of class c whose arg-max prediction is c."""
    pred, tgt = _np(probs).argmax(axis=1), _np(target).astype(np.int64)
    out = np.zeros(num_classes, dtype=np.float32)
    for c in range(num_classes):
        n = int((tgt == c).sum())
        out[c] = float(((pred == c) & (tgt == c)).sum()) / n if n else 0.0
    return out


def binary_auroc(score: np.ndarray, positive: np.ndarray) -> float:
    """Area under the ROC curve (Mann-Whitney U with tied scores sharing their mean rank = the trapezoidal ROC area)."""
    score = np.asarray(score, dtype=np.float64)
    positive = np.asarray(positive, dtype=bool)
    n_pos, n_neg = int(positive.sum()), int((~positive).sum())
    if n_pos == 0 or n_neg == 0:
        return 0.0
    order = np.argsort(score, kind="mergesort")
    s = score[order]
    ranks = np.empty(len(s), dtype=np.float64)
    i = 0
    while i < len(s):
        j = i
        while j + 1 < len(s) and s[j + 1] == s[i]:
            j += 1
        ranks[i:j + 1] = 0.5 * (i + j) + 1.0
        i = j + 1
    r = np.empty_like(ranks)
    r[order] = ranks
    return float((r[positive].sum() - n_pos * (n_pos + 1) / 2.0) / (n_pos * n_neg))


def multiclass_auroc(probs, target, num_classes: int) -> np.ndarray:
    """One-vs-rest AUROC per class on the class probabilities."""
    p, tgt = _np(probs), _np(target).astype(np.int64)
    return np.array([binary_auroc(p[:, c], tgt == c) for c in range(num_classes)], dtype=np.float32)


class ClassificationMetrics:
    """MetricCollection([MulticlassAccuracy(average=None), MulticlassAUROC(average=None)]): update with (probs, target) batches,
    compute() -> {"MulticlassAccuracy": [C], "MulticlassAUROC": [C]}, reset()."""

    def __init__(self, num_classes: int):
        self.num_classes = num_classes
        self.reset()

    def reset(self) -> None:
        self._p, self._t = [], []

    def __call__(self, probs, target) -> None:
        self.update(probs, target)

    def update(self, probs, target) -> None:
        self._p.append(_np(probs).astype(np.float32))
        self._t.append(_np(target).astype(np.int64))

    def compute(self):
        p = np.concatenate(self._p) if self._p else np.zeros((0, self.num_classes), np.float32)
        t = np.concatenate(self._t) if self._t else np.zeros(0, np.int64)
        return {"MulticlassAccuracy": multiclass_accuracy(p, t, self.num_classes),
                "MulticlassAUROC": multiclass_auroc(p, t, self.num_classes)}


def binary_average_precision(score: np.ndarray, positive: np.ndarray) -> float:
    """Average precision: the step-wise sum over the distinct thresholds, from the highest score down, of (R_k - R_{k-1}) P_k,
    tied scores forming one threshold (sklearn's average_precision_score).  0.0 without a positive or without a negative."""
    score = np.asarray(score, dtype=np.float64)
    positive = np.asarray(positive, dtype=bool)
    n_pos, n_neg = int(positive.sum()), int((~positive).sum())
    if n_pos == 0 or n_neg == 0:
        return 0.0
    order = np.argsort(-score, kind="mergesort")
    s, p = score[order], positive[order]
    last = np.r_[np.flatnonzero(s[1:] != s[:-1]), len(s) - 1]  # the last sample of every run of equal scores
    tp = np.cumsum(p)[last].astype(np.float64)
    precision, recall = tp / (last + 1.0), tp / n_pos
    return float(np.sum(np.diff(np.r_[0.0, recall]) * precision))


class MultilabelMetrics:
    """Per-label metrics of multi-label fine-tuning (TRAIN.LABEL_NAMES; an addition of this build) with the interface of
    ClassificationMetrics: update with (sigmoid probabilities [B, T], target [B, T]) batches, a negative target marking a missing
    entry that no metric counts.  compute() -> {"MultilabelAccuracy", "MultilabelAUROC", "MultilabelAveragePrecision"}, each
    [T] fp32: the share of a label's valid entries on the right side of 0.5, `binary_auroc` and `binary_average_precision` on
    them.  A label without a positive or without a negative valid entry scores 0.0 everywhere, the convention above."""

    def __init__(self, label_names):
        self.label_names = list(label_names)
        self.num_labels = len(self.label_names)
        self.reset()

    def reset(self) -> None:
        self._p, self._t = [], []

    def __call__(self, probs, target) -> None:
        self.update(probs, target)

    def update(self, probs, target) -> None:
        p, t = _np(probs).astype(np.float32), _np(target).astype(np.float32)
        if p.ndim != 2 or p.shape[1] != self.num_labels or t.shape != p.shape:
            raise ValueError(f"MultilabelMetrics: probabilities {p.shape} and targets {t.shape} must both be [B, {self.num_labels}]")
        self._p.append(p)
        self._t.append(t)

    def _tables(self):
        T = self.num_labels
        p = np.concatenate(self._p) if self._p else np.zeros((0, T), np.float32)
        t = np.concatenate(self._t) if self._t else np.zeros((0, T), np.float32)
        return p, t

    def has_both_values(self) -> np.ndarray:
        """bool [T]: the labels with a positive and a negative valid entry so far, the ones compute() scores."""
        _, t = self._tables()
        return ((t >= 0.5).any(axis=0)) & (((t >= 0) & (t < 0.5)).any(axis=0))

    def compute(self):
        T = self.num_labels
        p, t = self._tables()
        scored = self.has_both_values()
        acc, auroc, ap = (np.zeros(T, dtype=np.float32) for _ in range(3))
        for c in range(T):
            valid = t[:, c] >= 0
            score, positive = p[valid, c], t[valid, c] >= 0.5
            if not scored[c]:
                continue
            acc[c] = float(((score >= 0.5) == positive).mean())
            auroc[c] = binary_auroc(score, positive)
            ap[c] = binary_average_precision(score, positive)
        return {"MultilabelAccuracy": acc, "MultilabelAUROC": auroc, "MultilabelAveragePrecision": ap}


class SegmentationMetrics:
    """Per-class overlap metrics of segmentation fine-tuning (an addition of this build) from the confusion counts
    `hct_seg_predict` gives: update with int64 [B, K, 3] = TP, FP, FN per scan and class over the valid voxels.  compute() ->
    {"DiceGlobal", "IoUGlobal"}: [K] from the counts summed over every scan (and, after `all_reduce`, every rank) -- the
    dataset-level figures; {"DiceScan"}: [K], the mean of the per-scan Dice over the scans where the class is present
    (TP + FN > 0); {"ScansPresent"}: [K] how many those are.  A class that is neither present nor predicted anywhere has
    Dice and IoU nan; a class present in no scan has DiceScan nan."""

    def __init__(self, num_classes: int):
        self.num_classes = int(num_classes)
        self.reset()

    def reset(self) -> None:
        self._total = np.zeros((self.num_classes, 3), dtype=np.int64)
        self._scan_sum = np.zeros(self.num_classes, dtype=np.float64)
        self._scan_n = np.zeros(self.num_classes, dtype=np.int64)

    def __call__(self, counts) -> None:
        self.update(counts)

    def update(self, counts) -> None:
        c = _np(counts).astype(np.int64)
        if c.ndim != 3 or c.shape[1:] != (self.num_classes, 3):
            raise ValueError(f"SegmentationMetrics: counts {c.shape} must be [B, {self.num_classes}, 3]")
        self._total += c.sum(axis=0)
        tp, fp, fn = (c[:, :, i].astype(np.float64) for i in range(3))
        present = (tp + fn) > 0
        dice = 2 * tp / np.where(present, 2 * tp + fp + fn, 1.0)
        self._scan_sum += np.where(present, dice, 0.0).sum(axis=0)
        self._scan_n += present.sum(axis=0)

    def all_reduce(self) -> None:
        """Sum the accumulators over the ranks (a no-op in a world of one)."""
        import torch
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
            return
        dev = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
        for name in ("_total", "_scan_sum", "_scan_n"):
            t = torch.from_numpy(getattr(self, name).astype(np.float64)).to(dev)
            dist.all_reduce(t)
            setattr(self, name, t.cpu().numpy().astype(getattr(self, name).dtype))

    def compute(self):
        tp, fp, fn = (self._total[:, i].astype(np.float64) for i in range(3))
        with np.errstate(invalid="ignore", divide="ignore"):
            dice = 2 * tp / (2 * tp + fp + fn)
            iou = tp / (tp + fp + fn)
            scan = self._scan_sum / self._scan_n
        return {"DiceGlobal": dice, "IoUGlobal": iou, "DiceScan": scan, "ScansPresent": self._scan_n.copy()}


class SurfaceMetrics:
    """Per-class surface-distance figures over the scans of a test pass (headct_foundation_amd/surface.py): update with what
    `surface_metrics` returns for one scan.  A scan is scored for a class unless both masks are empty there (NSD NaN); a scan with
    exactly one of them empty (NSD 0, the distances NaN) counts under `OneEmpty`, enters the NSD mean and not the distance means.
    compute() -> {"HD95", "ASSD", "NSD", "HD"}: float64 [K], the mean over the scored scans (NaN where there is none, and at the
    background's index 0); {"ScansScored", "OneEmpty"}: lists of K integers."""

    DIST = ("HD95", "ASSD", "HD")

    def __init__(self, num_classes: int):
        self.num_classes = int(num_classes)
        self.reset()

    def reset(self) -> None:
        K = self.num_classes
        self._sum = {k: np.zeros(K, dtype=np.float64) for k in self.DIST + ("NSD",)}
        self._n_dist = np.zeros(K, dtype=np.int64)
        self._n_scored = np.zeros(K, dtype=np.int64)
        self._n_one_empty = np.zeros(K, dtype=np.int64)

    def __call__(self, scan) -> None:
        self.update(scan)

    def update(self, scan) -> None:
        v = {k: np.asarray(scan[k], dtype=np.float64) for k in self.DIST + ("NSD",)}
        if any(a.shape != (self.num_classes,) for a in v.values()):
            raise ValueError(f"SurfaceMetrics: every figure must be [{self.num_classes}]")
        scored = ~np.isnan(v["NSD"])
        scored[0] = False
        both = scored & ~np.isnan(v["HD"])
        for k in self.DIST:
            self._sum[k] += np.where(both, v[k], 0.0)
        self._sum["NSD"] += np.where(scored, v["NSD"], 0.0)
        self._n_dist += both
        self._n_scored += scored
        self._n_one_empty += scored & ~both

    def all_reduce(self) -> None:
        """Sum the accumulators over the ranks (a no-op in a world of one)."""
        import torch
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
            return
        dev = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
        for name in ("_n_dist", "_n_scored", "_n_one_empty"):
            t = torch.from_numpy(getattr(self, name).astype(np.float64)).to(dev)
            dist.all_reduce(t)
            setattr(self, name, t.cpu().numpy().astype(np.int64))
        for k in self._sum:
            t = torch.from_numpy(self._sum[k]).to(dev)
            dist.all_reduce(t)
            self._sum[k] = t.cpu().numpy()

    def merge(self, other: "SurfaceMetrics") -> None:
        """Add another rank's accumulators: what `all_reduce` does over a process group."""
        for k in self._sum:
            self._sum[k] = self._sum[k] + other._sum[k]
        for name in ("_n_dist", "_n_scored", "_n_one_empty"):
            setattr(self, name, getattr(self, name) + getattr(other, name))

    def compute(self):
        with np.errstate(invalid="ignore", divide="ignore"):
            out = {k: self._sum[k] / self._n_dist for k in self.DIST}
            out["NSD"] = self._sum["NSD"] / self._n_scored
        out["ScansScored"] = [int(v) for v in self._n_scored]
        out["OneEmpty"] = [int(v) for v in self._n_one_empty]
        return out


class LesionMetrics:
    """Lesion-wise detection over the scans of a test pass (headct_foundation_amd/components.py): update with what `lesion_metrics`
    returns for one scan.  The four counts are summed over the scans (and, after `all_reduce` or `merge`, the ranks), so the
    figures are micro-averages over the dataset.  compute() -> {"LesionRecall" = gt_detected / n_gt, "LesionPrecision" =
    pred_matched / n_pred, "LesionF1" = 2 P R / (P + R)}: float64 [K], NaN where a denominator is 0 and at the background's
    index 0; {"n_gt", "n_pred", "gt_detected", "pred_matched"}: lists of K integers."""

    KEYS = ("n_gt", "n_pred", "gt_detected", "pred_matched")

    def __init__(self, num_classes: int):
        self.num_classes = int(num_classes)
        self.reset()

    def reset(self) -> None:
        self._total = np.zeros((4, self.num_classes), dtype=np.int64)

    def __call__(self, scan) -> None:
        self.update(scan)

    def update(self, scan) -> None:
        v = np.stack([np.asarray(scan[k]) for k in self.KEYS])
        if v.shape != (4, self.num_classes) or not np.issubdtype(v.dtype, np.integer):
            raise ValueError(f"LesionMetrics: every count must be an integer array [{self.num_classes}]")
        v = v.astype(np.int64)
        if (v < 0).any() or (v[2] > v[0]).any() or (v[3] > v[1]).any() or v[:, 0].any():
            raise ValueError("LesionMetrics: counts must be >= 0, detected <= n_gt, matched <= n_pred, and 0 at the background's index")
        self._total += v

    def all_reduce(self) -> None:
        """Sum the accumulators over the ranks (a no-op in a world of one)."""
        import torch
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
            return
        dev = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
        t = torch.from_numpy(self._total).to(dev)  # int64: lesion counts add exactly
        dist.all_reduce(t)
        self._total = t.cpu().numpy().astype(np.int64)

    def merge(self, other: "LesionMetrics") -> None:
        """Add another rank's accumulators: what `all_reduce` does over a process group."""
        self._total = self._total + other._total

    def compute(self):
        n_gt, n_pred, det, mat = (self._total[i].astype(np.float64) for i in range(4))
        with np.errstate(invalid="ignore", divide="ignore"):
            recall, precision = det / n_gt, mat / n_pred
            f1 = 2 * precision * recall / (precision + recall)
        for a in (recall, precision, f1):
            a[0] = np.nan
        out = {"LesionRecall": recall, "LesionPrecision": precision, "LesionF1": f1}
        out.update({k: [int(x) for x in self._total[i]] for i, k in enumerate(self.KEYS)})
        return out
