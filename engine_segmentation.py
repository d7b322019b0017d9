"""Segmentation fine-tuning loop on the HIP path (an addition of this build), shaped like engine_downstream.py.

Backbone (`ViTBackbone`, every one of its 1 + R + L normalised tokens) and head (`SegmentationHead`, one Linear per token) run their
forward and backward in the HIP kernels; the loss is `seg_loss` (SEG.CE_WEIGHT * cross-entropy + SEG.DICE_WEIGHT * Dice over the
voxels, read from the logits in token layout; its gradient overwrites the logits), the clip `clip_grad_norm_` (one norm per module),
the optimizers the fused ones.  With TRAIN.LOCK the backbone runs under no_grad and only the head trains.  Validation and test take
the arg-max and its confusion counts from `seg_predict` (one pass over the logits) and report `SegmentationMetrics`: per-class Dice
and IoU from the counts summed over all scans and ranks, and the mean per-scan Dice over the scans where the class is present.  The
best model is the one with the highest mean foreground dataset-level Dice on the validation set, kept as a device snapshot and put
back before `trainer` returns.  With SEG.SAVE_PREDS the test pass writes the arg-max volumes in model space as int16 NIfTI files
under MODEL.DIR/<PREDS_SAVE_NAME>_preds/.  With SEG.NATIVE_PREDS the test pass also carries every scan's logits back onto its own file
grid (`NativePass`: headct_foundation_amd/native.py, hct_seg_to_native): <name>_native.nii.gz with the image's affine, one row of
native_volumes.csv (mL per class) and a second SegmentationMetrics against the mask file itself, reported as NativeDiceGlobal,
NativeIoUGlobal and NativeDiceScan.  With SEG.SURFACE_METRICS on top of that, every scan's boundary metrics in millimetres
(headct_foundation_amd/surface.py: HD, HD95, ASSD and NSD at SEG.SURFACE_TOLERANCE_MM, under the spacing of the file's affine) go into
native_surface.csv and, as means over the scored scans, into NativeHD95, NativeASSD, NativeNSD and NativeHD.  With
SEG.MIN_COMPONENT_ML > 0 the predicted connected components below that volume (headct_foundation_amd/components.py, at
SEG.COMPONENT_CONNECTIVITY) become background before any of that is written or scored; with SEG.LESION_METRICS every scan's lesion
counts go into native_lesion_counts.csv, every lesion into native_lesions.csv, and the dataset's lesion-wise recall, precision and F1
into NativeLesionRecall, NativeLesionPrecision and NativeLesionF1.
"""
import csv
import math
import os
import re
import sys
import time
from typing import Any, Iterable, List

import numpy as np
import torch

from engine_downstream import restore, snapshot
from headct_foundation_amd.components import lesion_metrics, min_voxels_for, remove_small_components
from headct_foundation_amd.metrics import LesionMetrics, SegmentationMetrics, SurfaceMetrics
from headct_foundation_amd.misc import MetricLogger, all_reduce_mean, get_rank
from headct_foundation_amd.native import GeometryCache, class_volumes_ml, read_native_labels, seg_to_native
from headct_foundation_amd.nifti import write_nifti
from headct_foundation_amd.optim import clip_grad_norm_
from headct_foundation_amd.segmentation import seg_loss, seg_predict
from headct_foundation_amd.surface import surface_metrics, voxel_spacing


def _class_weight(config, device):
    cw = list(config.SEG.CLASS_WEIGHT)
    return torch.tensor(cw, dtype=torch.float32, device=device) if cw else None


def _first(model) -> int:
    """Leading rows of a sample's tokens that are no patches: the class token and the registers."""
    return 1 + int(model.num_register_tokens)


def _tokens(config, model, data, lock: bool):
    if config.MODEL.NAME != 'vit':
        raise NotImplementedError(f"Unknown model: {config.MODEL.NAME}")
    if lock:
        with torch.no_grad():
            out, _ = model(data)
    else:
        out, _ = model(data)
    return out


def _loss(config, head, logits, labels, first, class_weight, inplace_grad, parts=None):
    return seg_loss(logits, labels, head.patch_size, head.num_classes, first, config.SEG.CE_WEIGHT, config.SEG.DICE_WEIGHT, class_weight,
                    inplace_grad=inplace_grad, parts=parts)


def train_one_epoch(config: Any, model, head, loader: Iterable, optimizers: List, schedulers: List, epoch: int, max_epoch: int, logger=None,
                    device=None) -> dict:
    model.train()
    head.train()
    lock = bool(config.TRAIN.LOCK)
    cw, first = _class_weight(config, device), _first(model)
    metric_logger = MetricLogger(delimiter="  ", logger=logger)
    n = len(loader) if hasattr(loader, "__len__") else -1
    for idx, (data, labels, _) in enumerate(loader):
        for optimizer in optimizers:
            optimizer.zero_grad()
        data, labels = data.to(device), labels.to(device)
        parts = {}
        logits = head(_tokens(config, model, data, lock))
        loss = _loss(config, head, logits, labels, first, cw, True, parts)  # the gradient takes the logits' place
        loss.backward()
        if config.TRAIN.GRAD_CLIP:
            clip_grad_norm_(head, config.TRAIN.GRAD_CLIP)
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
        metric_logger.update(loss=loss_value, ce=float(parts["ce"]), dice=float(parts["dice"]))
        metric_logger.update(lr=optimizers[0].param_groups[0]["lr"])
        if logger is not None:
            logger.info(f"Epoch {epoch+1}/{max_epoch} [{idx+1}/{n}]  Loss: {loss_value:.4f}  CE: {float(parts['ce']):.4f}  Dice: {float(parts['dice']):.4f}")
    metric_logger.synchronize_between_processes()
    if logger is not None:
        logger.info(f"Averaged stats: {metric_logger}")
    return {k: meter.global_avg for k, meter in metric_logger.meters.items()}


def _pred_file(out_dir: str, name, tag: str = "pred") -> str:
    base = os.path.basename(str(name))
    for ext in (".nii.gz", ".nii"):
        if base.endswith(ext):
            base = base[:-len(ext)]
    return os.path.join(out_dir, re.sub(r"[^A-Za-z0-9_.-]", "_", base) + f"_{tag}.nii.gz")


class NativePass:
    """The test pass on each scan's own grid (SEG.NATIVE_PREDS).  Per scan: its geometry through GeometryCache (DATA.CACHE_DIR), the
    raw mask file as labels, seg_to_native, <name>_native.nii.gz (int16, the image's own affine), one row of native_volumes.csv
    (name, then mL per class) and the native TP / FP / FN into `metrics`.  Mask paths come from `loader.pairs`.  With
    SEG.SURFACE_METRICS also one row of native_surface.csv (name, then HD, HD95, ASSD, NSD in mm per foreground class) and the scan's
    figures into `surface`.  With SEG.MIN_COMPONENT_ML > 0 the prediction is filtered (remove_small_components) before all of these, so
    that they describe the mask that is written; with SEG.LESION_METRICS one row of native_lesion_counts.csv per scan, one row of
    native_lesions.csv per lesion, and the scan's counts into `lesions`."""

    def __init__(self, config, loader, out_dir: str):
        if config.DATA.SYNTHETIC or not hasattr(loader, "pairs"):
            raise ValueError("SEG.NATIVE_PREDS needs image / mask files: synthetic volumes have no file grid")
        self.num_classes, self.interp, self.out_dir = int(config.SEG.NUM_CLASSES), str(config.SEG.NATIVE_INTERP), out_dir
        self.geometry = GeometryCache(config.DATA.CACHE_DIR, [int(r) for r in config.MODEL.ROI], config.VIT.IN_CHANS)
        self.seg_of = {img: seg for img, seg in loader.pairs}
        self.metrics = SegmentationMetrics(self.num_classes)
        os.makedirs(out_dir, exist_ok=True)
        rank = get_rank()
        self.csv_path = os.path.join(out_dir, "native_volumes.csv" if rank == 0 else f"native_volumes_rank{rank}.csv")
        with open(self.csv_path, "w", newline="") as f:
            csv.writer(f).writerow(["name"] + [f"class_{c}_ml" for c in range(self.num_classes)])
        self.surface = None
        if config.SEG.SURFACE_METRICS:
            self.surface, self.tolerance = SurfaceMetrics(self.num_classes), float(config.SEG.SURFACE_TOLERANCE_MM)
            self.surface_csv = os.path.join(out_dir, "native_surface.csv" if rank == 0 else f"native_surface_rank{rank}.csv")
            with open(self.surface_csv, "w", newline="") as f:
                csv.writer(f).writerow(["name"] + [f"class_{c}_{k}" for c in range(1, self.num_classes) for k in ("hd_mm", "hd95_mm", "assd_mm", "nsd")])
        self.min_ml, self.connectivity = float(config.SEG.MIN_COMPONENT_ML), int(config.SEG.COMPONENT_CONNECTIVITY)
        self.lesions = None
        if config.SEG.LESION_METRICS:
            self.lesions = LesionMetrics(self.num_classes)
            tag = "" if rank == 0 else f"_rank{rank}"
            self.lesion_counts_csv, self.lesions_csv = (os.path.join(out_dir, f"{stem}{tag}.csv") for stem in ("native_lesion_counts", "native_lesions"))
            with open(self.lesion_counts_csv, "w", newline="") as f:
                csv.writer(f).writerow(["name"] + [f"class_{c}_{k}" for c in range(1, self.num_classes) for k in LesionMetrics.KEYS])
            with open(self.lesions_csv, "w", newline="") as f:
                csv.writer(f).writerow(["name", "class", "side", "index", "voxels", "ml", "overlap_voxels"])

    def scan(self, name, logits_b, patch_size: int, first: int, device) -> None:
        geom = self.geometry.get(name, device)
        labels = read_native_labels(self.seg_of[name], geom, name)
        out = seg_to_native(logits_b, patch_size, self.num_classes, first, geom, self.interp, labels=labels)
        labels_d = None  # the mask on the device, uploaded once for whichever of the filter, the surface and the lesion metrics run
        if self.min_ml > 0.0 or self.surface is not None or self.lesions is not None:
            labels_d = torch.from_numpy(labels).to(out["pred"].device)
        if self.min_ml > 0.0:  # before anything is written or scored: every figure below describes the filtered mask
            # a threshold of at most one voxel removes nothing: the call then hands back the figures it is given
            kept = remove_small_components(out["pred"], self.num_classes, min_voxels_for(self.min_ml, geom.affine), self.connectivity, labels=labels_d,
                                           class_voxels=out["class_voxels"], counts=out["counts"])
            out = {**out, "pred": kept["pred"], "class_voxels": kept["class_voxels"], "counts": kept["counts"]}
        write_nifti(_pred_file(self.out_dir, name, "native"), out["pred"].cpu().numpy(), affine=np.asarray(geom.affine), dtype="i2")
        ml = class_volumes_ml(out["class_voxels"], geom.affine)
        with open(self.csv_path, "a", newline="") as f:
            csv.writer(f).writerow([name] + [f"{v:.6f}" for v in ml])
        self.metrics(out["counts"].unsqueeze(0))
        if self.surface is not None:
            scan = surface_metrics(out["pred"], labels_d, self.num_classes, voxel_spacing(geom.affine), self.tolerance)
            with open(self.surface_csv, "a", newline="") as f:
                csv.writer(f).writerow([name] + [f"{scan[k][c]:.6f}" for c in range(1, self.num_classes) for k in ("HD", "HD95", "ASSD", "NSD")])
            self.surface(scan)
        if self.lesions is not None:
            scan = lesion_metrics(out["pred"], labels_d, self.num_classes, self.connectivity)
            voxel_ml = float(class_volumes_ml(np.ones(1), geom.affine)[0])
            with open(self.lesion_counts_csv, "a", newline="") as f:
                csv.writer(f).writerow([name] + [int(scan[k][c]) for c in range(1, self.num_classes) for k in LesionMetrics.KEYS])
            with open(self.lesions_csv, "a", newline="") as f:
                csv.writer(f).writerows([name, c, side, m, voxels, f"{voxels * voxel_ml:.6f}", overlap] for c, side, m, voxels, overlap in scan["lesions"])
            self.lesions(scan)


def val_one_epoch(config: Any, model, head, loader: Iterable, epoch: int, max_epoch: int, metrics: SegmentationMetrics, logger=None, device=None,
                  save_preds: bool = False, native: NativePass = None) -> dict:
    model.eval()
    head.eval()
    cw, first = _class_weight(config, device), _first(model)
    metric_logger = MetricLogger(delimiter="  ", logger=logger)
    n = len(loader) if hasattr(loader, "__len__") else -1
    out_dir = os.path.join(config.MODEL.DIR, f"{config.PREDS_SAVE_NAME}_preds")
    if save_preds:
        os.makedirs(out_dir, exist_ok=True)
    with torch.no_grad():
        for idx, (data, labels, names) in enumerate(loader):
            data, labels = data.to(device), labels.to(device)
            logits = head(_tokens(config, model, data, True))
            loss = _loss(config, head, logits, labels, first, cw, False)
            out = seg_predict(logits, head.patch_size, head.num_classes, first, labels=labels, want_pred=save_preds)
            metrics(out["counts"])
            if save_preds:
                pred = out["pred"].cpu().numpy()
                for b, name in enumerate(names):
                    write_nifti(_pred_file(out_dir, name), pred[b].astype(np.int16), dtype="i2")
            if native is not None:
                for b, name in enumerate(names):
                    if name != "None":  # a scan that failed to load
                        native.scan(name, logits[b], head.patch_size, first, device)
            loss_value = float(all_reduce_mean(loss))
            metric_logger.update(loss=loss_value)
            if logger is not None:
                logger.info(f"Epoch {epoch+1}/{max_epoch} [{idx+1}/{n}]  Loss: {loss_value:.4f}")
    metrics.all_reduce()
    if native is not None:
        native.metrics.all_reduce()
        if native.surface is not None:
            native.surface.all_reduce()
        if native.lesions is not None:
            native.lesions.all_reduce()
    metric_logger.synchronize_between_processes()
    if logger is not None:
        logger.info(f"Averaged stats: {metric_logger}")
    return {k: meter.global_avg for k, meter in metric_logger.meters.items()}


def _fmt(a) -> str:
    return "[" + ", ".join(f"{float(v):.4f}" for v in a) + "]"


def _log_metrics(logger, out) -> None:
    if logger is not None:
        logger.info(f"SegDiceGlobal: {_fmt(out['DiceGlobal'])}, SegIoUGlobal: {_fmt(out['IoUGlobal'])}, SegDiceScan: {_fmt(out['DiceScan'])}, "
                    f"ScansPresent: {[int(v) for v in out['ScansPresent']]}")


def mean_foreground_dice(out) -> float:
    """The figure the best checkpoint is chosen by: the mean dataset-level Dice over the foreground classes (an undefined one counts 0)."""
    return float(np.nan_to_num(np.asarray(out["DiceGlobal"], dtype=np.float64)[1:]).mean())


def save_seg_checkpoint(config, model, head, epoch, optimizer, scheduler, best, logger=None) -> str:
    """One file: the backbone under `state_dict` (what `load_model` reads), the head under `seg_head_state_dict`, and what the head
    was built with."""
    os.makedirs(config.MODEL.DIR, exist_ok=True)
    path = os.path.join(config.MODEL.DIR, config.MODEL.SAVE_NAME)
    torch.save({"epoch": epoch, "best_loss": best, "state_dict": model.state_dict(), "seg_head_state_dict": head.state_dict(),
                "seg": {"num_classes": head.num_classes, "patch_size": head.patch_size, "dim": head.dim},
                "optimizer": optimizer.state_dict(), "scheduler": scheduler.state_dict()}, path)
    if logger is not None:
        logger.info(f"Saving checkpoint {path}")
    return path


def trainer(config: Any, model, head, train_loader: Iterable, val_loader: Iterable, optimizers: List, schedulers: List, start_epoch: int = 0,
            max_epochs: int = 100, val_every: int = 10, logger=None, device=None):
    """Returns (best mean foreground validation Dice, best model, best head)."""
    lock = bool(config.TRAIN.LOCK)
    best = {"model": None if lock else snapshot(model), "head": snapshot(head)}
    best_dice = -1.0
    val_metrics = SegmentationMetrics(config.SEG.NUM_CLASSES)
    for epoch in range(start_epoch, max_epochs):
        if logger is not None:
            logger.info(f"Epoch: {epoch+1}")
        t0 = time.time()
        stats = train_one_epoch(config, model, head, train_loader, optimizers, schedulers, epoch, max_epochs, logger=logger, device=device)
        if logger is not None:
            logger.info(f"Final training  {epoch+1}/{max_epochs}, loss: {stats['loss']}, time {time.time() - t0}s")
        if (epoch + 1) % val_every == 0 and (val_every == 1 or epoch != 0):
            t0 = time.time()
            val_stats = val_one_epoch(config, model, head, val_loader, epoch, max_epochs, val_metrics, logger=logger, device=device)
            if logger is not None:
                logger.info(f"Final validation {epoch+1}/{max_epochs} loss: {val_stats['loss']}, time {time.time() - t0}s")
            out = val_metrics.compute()
            _log_metrics(logger, out)
            val_metrics.reset()
            dice = mean_foreground_dice(out)
            if dice > best_dice:
                if logger is not None:
                    logger.info(f"new best Dice ({best_dice} --> {dice}). ")
                best_dice = dice
                if get_rank() == 0:
                    save_seg_checkpoint(config, model, head, epoch, optimizers[0], schedulers[0], dice, logger)
                best["head"] = snapshot(head)
                if not lock:
                    best["model"] = snapshot(model)
    if logger is not None:
        logger.info(f"Training Finished !, Best Dice: {best_dice}")
    if best["model"] is not None:
        restore(model, best["model"])
    restore(head, best["head"])
    return best_dice, model, head


def tester(config: Any, model, head, test_loader: Iterable, logger=None, device=None) -> dict:
    t0 = time.time()
    metrics = SegmentationMetrics(config.SEG.NUM_CLASSES)
    native = None
    if config.SEG.NATIVE_PREDS:
        native = NativePass(config, test_loader, os.path.join(config.MODEL.DIR, f"{config.PREDS_SAVE_NAME}_preds"))
    stats = val_one_epoch(config, model, head, test_loader, 0, 1, metrics, logger=logger, device=device, save_preds=bool(config.SEG.SAVE_PREDS),
                          native=native)
    if logger is not None:
        logger.info(f"Final test loss: {stats['loss']}, time {time.time() - t0}s")
    out = metrics.compute()
    _log_metrics(logger, out)
    if native is not None:
        nat = native.metrics.compute()
        if logger is not None:
            logger.info(f"NativeDiceGlobal: {_fmt(nat['DiceGlobal'])}, NativeIoUGlobal: {_fmt(nat['IoUGlobal'])}, NativeDiceScan: {_fmt(nat['DiceScan'])}, "
                        f"NativeScansPresent: {[int(v) for v in nat['ScansPresent']]}")
        out = {**out, "NativeDiceGlobal": nat["DiceGlobal"], "NativeIoUGlobal": nat["IoUGlobal"], "NativeDiceScan": nat["DiceScan"]}
        if native.surface is not None:
            sur = native.surface.compute()
            if logger is not None:
                logger.info(f"NativeHD95: {_fmt(sur['HD95'])}, NativeASSD: {_fmt(sur['ASSD'])}, NativeNSD: {_fmt(sur['NSD'])}, NativeHD: {_fmt(sur['HD'])}, "
                            f"NativeSurfaceScored: {sur['ScansScored']}, NativeSurfaceOneEmpty: {sur['OneEmpty']}")
            out = {**out, "NativeHD95": sur["HD95"], "NativeASSD": sur["ASSD"], "NativeNSD": sur["NSD"], "NativeHD": sur["HD"]}
        if native.lesions is not None:
            les = native.lesions.compute()
            if logger is not None:
                logger.info(f"NativeLesionRecall: {_fmt(les['LesionRecall'])}, NativeLesionPrecision: {_fmt(les['LesionPrecision'])}, "
                            f"NativeLesionF1: {_fmt(les['LesionF1'])}, NativeLesionsGT: {les['n_gt']}, NativeLesionsPred: {les['n_pred']}, "
                            f"NativeLesionsDetected: {les['gt_detected']}, NativeLesionsMatched: {les['pred_matched']}")
            out = {**out, "NativeLesionRecall": les["LesionRecall"], "NativeLesionPrecision": les["LesionPrecision"], "NativeLesionF1": les["LesionF1"]}
    return {"loss": stats["loss"], **out}


__all__ = ["NativePass", "train_one_epoch", "val_one_epoch", "trainer", "tester", "save_seg_checkpoint", "mean_foreground_dice"]
