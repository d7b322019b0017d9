"""Downstream fine-tuning / probing loop on the HIP path: the reference's engine_downstream.py (train_one_epoch :23-132,
val_one_epoch :135-226, trainer :229-380, tester :383-447) with the same signatures.

Backbone (`ViTBackbone`) and head (`LinearClassifier` on the class token / `AttentionClassifier` on every token) run their
forward and backward in the HIP kernels; the loss is `cross_entropy` (or `bce_with_logits`, below), the clip `clip_grad_norm_` (one norm per module, head and
backbone separately, engine_downstream.py:107-111), the optimizers `HipAdamW`.  With TRAIN.LOCK the backbone runs under no_grad
and only the head trains.  Metrics are per-class accuracy and one-vs-rest AUROC on the softmax probabilities (host side,
headct_foundation_amd/metrics.py).  The best model is kept as a device snapshot of the flat parameter buffers and BatchNorm
statistics (the reference deep-copies the modules); `trainer` puts it back into the modules before it returns them, so the
returned model / classifier are the best ones, as the reference's are.  Out of scope: AMP (the
compute dtype is MAE.COMPUTE_DTYPE), wandb, the PR-curve plot.

Multi-label mode (TRAIN.LABEL_NAMES non-empty; an addition of this build): the head has one output per name, the targets are
fp32 [B, T] with negative entries missing, the criterion is `bce_with_logits`, the probabilities are sigmoids, the metrics
`MultilabelMetrics`, the best checkpoint the one with the highest mean AUROC over the labels that have both values in the
validation set, and the predictions pickle holds `preds` / `targets` [N, T] and `label_names`.  `_probabilities` and `_metrics`
are the two places that tell the modes apart.

Mixup, CutMix and label smoothing (TRAIN.MIXUP / CUTMIX / LABEL_SMOOTHING; additions of this build): when the criterion is a
`MixedCriterion`, `train_one_epoch` mixes each batch on the device and takes the loss from `train_loss`; `val_one_epoch` and
`tester` call the criterion as they call any other and so compute the plain loss.
The mix works IN PLACE on the tensor the loader yields.  That is the contract with loaders: a training batch belongs to the
engine once it is yielded (`LabelledVolumes` makes a fresh fp32 tensor per batch on both of its paths).  A loader that hands out
the same tensors again -- the synthetic loaders keep theirs for every epoch -- must say so with the class attribute
`reuses_batches = True`; the engine then mixes a copy.  Without the attribute such a loader's data would be mixed over and over.
"""
import math
import os
import pickle
import sys
import time
from typing import Any, Iterable, List, Optional

import numpy as np
import torch

from headct_foundation_amd.classifier import bce_with_logits, cross_entropy
from headct_foundation_amd.metrics import ClassificationMetrics, MultilabelMetrics
from headct_foundation_amd.mixup import MixedCriterion
from headct_foundation_amd.misc import MetricLogger, all_reduce_mean, get_rank, save_checkpoint
from headct_foundation_amd.optim import clip_grad_norm_


def _softmax(logits: torch.Tensor) -> np.ndarray:
    """Class probabilities on the host (metrics and the predictions pickle only; the training path never reads them)."""
    z = logits.detach().float().cpu().numpy().astype(np.float64)
    z = np.exp(z - z.max(axis=1, keepdims=True))
    return z / z.sum(axis=1, keepdims=True)


def _label_names(config) -> list:
    return list(config.TRAIN.LABEL_NAMES)


def _probabilities(config, logits: torch.Tensor) -> np.ndarray:
    """Probabilities of the logits on the host: softmax over the classes, or one sigmoid per label in multi-label mode."""
    if not _label_names(config):
        return _softmax(logits)
    z = logits.detach().float().cpu().numpy().astype(np.float64)
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def _metrics(config):
    """The metrics collection of the mode the config asks for."""
    names = _label_names(config)
    return MultilabelMetrics(names) if names else ClassificationMetrics(config.DATA.NUM_CLASSES)


def _features(config, model, data, lock: bool):
    if config.MODEL.NAME != 'vit':
        raise NotImplementedError(f"Unknown model: {config.MODEL.NAME}")
    if lock:
        with torch.no_grad():
            out, _ = model(data)
    else:
        out, _ = model(data)
    # the linear head takes the [B, T, D] tokens and classifies the class token (the reference's out[:, :1, :].squeeze()),
    # so its feature gradient lands in the class-token row without a scatter
    return out


def train_one_epoch(config: Any, model, classifier, loader: Iterable, optimizers: List, schedulers: List, criterion, epoch: int,
                    max_epoch: int, train_metric_collection, logger=None, device=None, use_amp: bool = False, scaler=None,
                    wandb_run=None) -> dict:
    """With a `MixedCriterion` the batch is mixed in place on the device (a loader that hands out the same tensors every epoch,
    `reuses_batches`, gets a copy mixed instead) and the loss is the criterion's `train_loss`.  The training metrics are still
    computed against the un-mixed labels: they then describe predictions on mixed inputs, not the model's accuracy."""
    model.train()
    classifier.train()
    lock = bool(config.TRAIN.LOCK)
    mixed = isinstance(criterion, MixedCriterion)
    metric_logger = MetricLogger(delimiter="  ", logger=logger)
    n = len(loader) if hasattr(loader, "__len__") else -1
    for idx, (data, target, _) in enumerate(loader):
        for optimizer in optimizers:
            optimizer.zero_grad()
        data, target = data.to(device), target.to(device)
        if mixed:
            if criterion.mixup is not None and getattr(loader, "reuses_batches", False):
                data = data.clone()
            data, mix_state = criterion.mix(data, target)
        logits = classifier(_features(config, model, data, lock))
        loss = criterion.train_loss(logits, target, mix_state) if mixed else criterion(logits, target)
        train_metric_collection(_probabilities(config, logits), target)
        loss.backward()
        if config.TRAIN.GRAD_CLIP:
            clip_grad_norm_(classifier, config.TRAIN.GRAD_CLIP)
            if not lock:
                clip_grad_norm_(model, config.TRAIN.GRAD_CLIP)
        for optimizer in optimizers:
            optimizer.step()
        for scheduler in schedulers:
            scheduler.step()
        loss_value = float(all_reduce_mean(loss.detach()))
        if not math.isfinite(loss_value):
            if logger is not None:
                logger.info(f"Loss is {loss_value}, stopping training")
            sys.exit(1)
        metric_logger.update(loss=loss_value)
        lr = optimizers[0].param_groups[0]["lr"]
        metric_logger.update(lr=lr)
        if logger is not None:
            logger.info(f"Epoch {epoch+1}/{max_epoch} [{idx+1}/{n}]  Loss: {loss_value:.4f}")
    metric_logger.synchronize_between_processes()
    if logger is not None:
        logger.info(f"Averaged stats: {metric_logger}")
    return {k: meter.global_avg for k, meter in metric_logger.meters.items()}


def val_one_epoch(config: Any, model, classifier, loader: Iterable, epoch: int, max_epoch: int, val_metric_collection, criterion,
                  logger=None, device=None, use_amp: bool = False, save_preds: bool = False, scaler=None) -> dict:
    """As the reference: the backbone in eval mode, the classifier left in the mode the caller set (training mode during
    training: batch statistics, as engine_downstream.py:168-170 runs it)."""
    model.eval()
    metric_logger = MetricLogger(delimiter="  ", logger=logger)
    fnames, probs, targets = [], [], []
    n = len(loader) if hasattr(loader, "__len__") else -1
    with torch.no_grad():
        for idx, (data, target, fname) in enumerate(loader):
            data, target = data.to(device), target.to(device)
            if save_preds:
                fnames += list(fname)
            logits = classifier(_features(config, model, data, True))
            loss = criterion(logits, target)
            p = _probabilities(config, logits)
            probs.append(p)
            targets.append(target.detach().cpu().numpy())
            val_metric_collection(p, target)
            loss_value = float(all_reduce_mean(loss))
            metric_logger.update(loss=loss_value)
            if logger is not None:
                logger.info(f"Epoch {epoch+1}/{max_epoch} [{idx+1}/{n}]  Loss: {loss_value:.4f}")
    if save_preds:
        out_dir = config.MODEL.DIR
        os.makedirs(out_dir, exist_ok=True)
        if _label_names(config):
            save_dict = {'fnames': fnames, 'preds': np.concatenate(probs).astype(np.float32), 'targets': np.concatenate(targets),
                         'label_names': _label_names(config)}
        else:
            save_dict = {'fnames': fnames, 'preds': np.concatenate(probs)[:, 1].astype(np.float32), 'targets': np.concatenate(targets)}
        with open(os.path.join(out_dir, f"{config.PREDS_SAVE_NAME}_preds.pkl"), "wb") as f:
            pickle.dump(save_dict, f)
    metric_logger.synchronize_between_processes()
    if logger is not None:
        logger.info(f"Averaged stats: {metric_logger}")
    return {k: meter.global_avg for k, meter in metric_logger.meters.items()}


def snapshot(module) -> dict:
    """Device copy of a flat-buffer module's parameters and buffers (running statistics)."""
    return {"flat": module._flat.detach().clone(), "buffers": {k: b.detach().clone() for k, b in module.named_buffers()}}


def restore(module, snap: dict) -> None:
    with torch.no_grad():
        module._flat.copy_(snap["flat"])
        for k, b in module.named_buffers():
            b.copy_(snap["buffers"][k])
    module.mark_weights_updated()


def _log_metrics(logger, out, label_names=()) -> None:
    if logger is None:
        return
    if "MultilabelAUROC" in out:
        logger.info(f"Labels: {list(label_names)}, MultilabelAccuracy: {out['MultilabelAccuracy']}, MultilabelAUROC: {out['MultilabelAUROC']}, "
                    f"MultilabelAveragePrecision: {out['MultilabelAveragePrecision']}")
    else:
        logger.info(f"MulticlassAccuracy: {out['MulticlassAccuracy']}, MulticlassAUROC:{out['MulticlassAUROC']}")


def _mean_auroc(out, metrics) -> float:
    """The figure the best checkpoint is chosen by: the mean one-vs-rest AUROC over the classes, or in multi-label mode the mean
    over the labels that have both values in the set (the others score 0.0 by convention and would pull the mean down)."""
    if "MultilabelAUROC" in out:
        scored = metrics.has_both_values()
        return float(out["MultilabelAUROC"][scored].mean()) if scored.any() else 0.0
    auroc = out["MulticlassAUROC"]
    return float(sum(auroc) / len(auroc))


def trainer(config: Any, model, classifier, train_loader: Iterable, val_loader: Iterable, optimizers: List, schedulers: List,
            criterion, start_epoch: int = 0, max_epochs: int = 100, val_every: int = 10, logger=None, device=None, wandb_run=None):
    """Returns (best mean validation AUROC, best model, best classifier).  The best weights and BatchNorm statistics are kept as
    device snapshots while training runs and restored into `model` / `classifier` before they are returned (the reference
    returns deep copies; with no validation run, the weights the training started from, as there)."""
    if config.DATA.NUM_CLASSES == 1:
        raise NotImplementedError(f"Unknown number of classes: {config.DATA.NUM_CLASSES}")
    lock = bool(config.TRAIN.LOCK)
    best = {"model": None if lock else snapshot(model), "classifier": snapshot(classifier)}
    val_auroc_max = -1
    train_metrics, val_metrics = _metrics(config), _metrics(config)
    names = _label_names(config)
    for epoch in range(start_epoch, max_epochs):
        if logger is not None:
            logger.info(f"Epoch: {epoch+1}")
        t0 = time.time()
        train_stats = train_one_epoch(config, model, classifier, train_loader, optimizers, schedulers, criterion, epoch, max_epochs,
                                      train_metrics, logger=logger, device=device, wandb_run=wandb_run)
        if logger is not None:
            logger.info(f"Final training  {epoch+1}/{max_epochs}, loss: {train_stats['loss']}, time {time.time() - t0}s")
        _log_metrics(logger, train_metrics.compute(), names)
        train_metrics.reset()
        if (epoch + 1) % val_every == 0 and (val_every == 1 or epoch != 0):
            t0 = time.time()
            val_stats = val_one_epoch(config, model, classifier, val_loader, epoch, max_epochs, val_metrics, criterion, logger=logger,
                                      device=device)
            if logger is not None:
                logger.info(f"Final validation {epoch+1}/{max_epochs} loss: {val_stats['loss']}, time {time.time() - t0}s")
            out = val_metrics.compute()
            _log_metrics(logger, out, names)
            val_auroc = _mean_auroc(out, val_metrics)
            val_metrics.reset()
            if val_auroc > val_auroc_max:
                if logger is not None:
                    logger.info(f"new best AUROC ({val_auroc_max} --> {val_auroc}). ")
                val_auroc_max = val_auroc
                if get_rank() == 0:
                    save_checkpoint(model, None, epoch, optimizers[0], schedulers[0], best_loss=val_auroc, dir_add=config.MODEL.DIR,
                                    filename=config.MODEL.SAVE_NAME, logger=logger)
                    name = config.MODEL.SAVE_NAME.split('.')[0] + '_classifier' + '.pt'
                    save_checkpoint(classifier, None, epoch, optimizers[0], schedulers[0], best_loss=val_auroc, dir_add=config.MODEL.DIR,
                                    filename=name, logger=logger)
                best["classifier"] = snapshot(classifier)
                if not lock:
                    best["model"] = snapshot(model)
    if logger is not None:
        logger.info(f"Training Finished !, Best AUROC: {val_auroc_max}")
    if best["model"] is not None:
        restore(model, best["model"])
    restore(classifier, best["classifier"])
    return val_auroc_max, model, classifier


def tester(config: Any, model, classifier, test_loader: Iterable, criterion, logger=None, device=None, wandb_run=None) -> float:
    t0 = time.time()
    metrics = _metrics(config)
    stats = val_one_epoch(config, model, classifier, test_loader, 0, 1, metrics, criterion, logger=logger, device=device,
                          save_preds=True)
    if logger is not None:
        logger.info(f"Final test loss: {stats['loss']}, time {time.time() - t0}s")
    _log_metrics(logger, metrics.compute(), _label_names(config))
    return stats['loss']


__all__ = ["train_one_epoch", "val_one_epoch", "trainer", "tester", "snapshot", "restore", "cross_entropy", "bce_with_logits"]
