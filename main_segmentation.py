"""Segmentation fine-tuning entry point on the HIP path (an addition of this build; shaped like main_downstream.py).

  torchrun --nnodes 1 --nproc_per_node 1 main_segmentation.py --local_rank 0 --model_name vit --cfg CFG.yaml \
      --model_load_path PRETRAINED.pt --seg_classes 3 --grad_clip 1.0 --batch_size 8 [--lock] [--save_preds]

Backbone: `ViTBackbone` from VIT.* in MAE.COMPUTE_DTYPE, loaded and position-interpolated as main_downstream.py does; head:
`SegmentationHead`, one Linear VIT.HIDDEN_SIZE -> SEG.NUM_CLASSES * VIT.PATCH_SIZE^3 per patch token.  Loss: SEG.CE_WEIGHT *
cross-entropy + SEG.DICE_WEIGHT * Dice over the voxels (`--ce_weight`, `--dice_weight`; SEG.CLASS_WEIGHT weighs the classes of the
cross-entropy), labels uint8 with 255 = ignore.  Two fused optimizers of the TRAIN.OPTIMIZER kind (backbone at BASE_LR, head at
100 x BASE_LR) with TRAIN.SCHEDULER warm-up schedules, only the head's with TRAIN.LOCK; layer decay, TRAIN.WD_EXCLUDE_1D, drop path,
dropout, LoRA, RMSNorm and register tokens work as in main_downstream.py.  Refused: TRAIN.AFFINE_PROB, TRAIN.MIXUP / CUTMIX and
VIT.PATCH_DROPOUT above 0 (config.check_segmentation_mode).  `--seg_affine_prob P` (SEG.AFFINE_PROB) is this mode's random 3-D affine:
a training sample is rotated, zoomed and translated with probability P, the scan trilinear and the mask nearest neighbour through the
same matrix (`--affine_rotate`, `--affine_scale`, `--affine_translate` give the magnitudes; `--seg_affine_outside background|ignore`
the label where the scan is zero-padded); validation and test are never touched.  Data: synthetic boxes (DATA.SYNTHETIC) or the image / mask pairs of
DATA.TRAIN / VAL / TEST_CSV_PATH (columns img_path, seg_path).  Validation and test report per-class Dice and IoU; `--save_preds`
writes the test pass's arg-max volumes as NIfTI files.  `--native_preds` (real data only) carries the test pass's logits back onto
each scan's own file grid (`--native_interp linear|nearest`): <name>_native.nii.gz with the image's affine, native_volumes.csv with
the volume of every class in mL, and NativeDiceGlobal / NativeIoUGlobal / NativeDiceScan against the mask files themselves.
`--surface_metrics` (with `--native_preds`) adds the boundary metrics in millimetres: native_surface.csv with HD, HD95, ASSD and the
surface Dice at `--surface_tolerance_mm` per scan and class, and NativeHD95 / NativeASSD / NativeNSD / NativeHD over the scans.
`--min_component_ml X` (with `--native_preds`) turns every predicted connected component smaller than X mL into background before the
native file, the volumes, the Dice and the surface metrics are taken, so all of them describe the mask that is written;
`--lesion_metrics` counts lesions: native_lesion_counts.csv (per scan and class: lesions annotated, predicted, detected, matched),
native_lesions.csv (one row per lesion with its volume in mL and its overlap) and NativeLesionRecall / NativeLesionPrecision /
NativeLesionF1 over the dataset.  `--component_connectivity 6|18|26` chooses the neighbourhood of both (26 by default).
"""
import argparse
import json
import os
import random

import numpy as np
import torch
import torch.distributed as dist
import torch.nn as nn

from config import check_segmentation_mode, get_config
from engine_segmentation import tester, trainer
from headct_foundation_amd.data import AugmentedSegmented, DeviceAugment, SyntheticSegmented, segmentation_affine
from headct_foundation_amd.dino_model import ViTBackbone
from headct_foundation_amd.layers import RMSNorm
from headct_foundation_amd.lr_sched import get_lr_scheduler
from headct_foundation_amd.misc import cleanup, init_distributed_mode, load_model, set_requires_grad_false
from headct_foundation_amd.optim import get_optimizer
from headct_foundation_amd.param_scales import describe_scales, layer_decay_scales, no_decay_scales
from headct_foundation_amd.segmentation import SegmentationHead
from logger import create_logger
from main_downstream import learning_rates


def parse_option():
    parser = argparse.ArgumentParser('HIP segmentation fine-tuning and evaluation script', add_help=False)
    parser.add_argument('--cfg', type=str, required=True, metavar="FILE", help='path to config file')
    parser.add_argument("--opts", help="Modify config options using the command-line", default=None, nargs='+')
    parser.add_argument("--preds_save_name", type=str, help='save name tag for predictions')
    parser.add_argument("--local_rank", type=int, default=int(os.environ.get("LOCAL_RANK", 0)), help='local rank')
    parser.add_argument('--dist-backend', default='nccl', help='parsed and ignored, like the reference')
    parser.add_argument('--dist-url', default='env://', help='parsed and ignored, like the reference')
    parser.add_argument("--seed", type=int, help='seed')
    parser.add_argument("--filename", type=str, default="monai-test")
    # model parameters
    parser.add_argument("--model_name", type=str, help='model name')
    parser.add_argument("--model_load_path", type=str, help='path to trained model')
    parser.add_argument("--seg_classes", type=int, help='number of classes, background included (SEG.NUM_CLASSES)')
    parser.add_argument("--ce_weight", type=float, help='weight of the cross-entropy term (SEG.CE_WEIGHT), >= 0')
    parser.add_argument("--dice_weight", type=float, help='weight of the Dice term (SEG.DICE_WEIGHT), >= 0')
    parser.add_argument("--save_preds", action='store_true', help='write the arg-max volumes of the test pass as NIfTI files (SEG.SAVE_PREDS)')
    parser.add_argument("--native_preds", action='store_true',
                        help='test pass on each scan\'s own grid: <name>_native.nii.gz, native_volumes.csv (mL), Dice against the mask file (SEG.NATIVE_PREDS)')
    parser.add_argument("--native_interp", type=str, choices=['linear', 'nearest'], help='how the logits reach the file grid (SEG.NATIVE_INTERP)')
    parser.add_argument("--surface_metrics", action='store_true',
                        help='with --native_preds: HD, HD95, ASSD and surface Dice in mm per scan, native_surface.csv (SEG.SURFACE_METRICS)')
    parser.add_argument("--surface_tolerance_mm", type=float, help='tolerance of the surface Dice in mm, >= 0 (SEG.SURFACE_TOLERANCE_MM)')
    parser.add_argument("--min_component_ml", type=float,
                        help='with --native_preds: predicted components below this volume in mL become background before anything is written or scored (SEG.MIN_COMPONENT_ML)')
    parser.add_argument("--lesion_metrics", action='store_true',
                        help='with --native_preds: lesion-wise recall, precision and F1, native_lesion_counts.csv and native_lesions.csv (SEG.LESION_METRICS)')
    parser.add_argument("--component_connectivity", type=int, help='neighbourhood of a connected component: 6, 18 or 26 (SEG.COMPONENT_CONNECTIVITY)')
    parser.add_argument("--seg_affine_prob", type=float,
                        help='probability of a random 3-D affine per training sample, scan and mask alike (SEG.AFFINE_PROB), in [0, 1]; 0 = off')
    parser.add_argument("--seg_affine_outside", type=str, choices=['background', 'ignore'],
                        help='label where the resampled scan is zero-padded: class 0 or the ignore index (SEG.AFFINE_OUTSIDE)')
    parser.add_argument("--affine_rotate", type=float, nargs='+', help='largest rotation about each axis in degrees: one value or three (TRAIN.AFFINE_ROTATE)')
    parser.add_argument("--affine_scale", type=float, help='zoom factor drawn from [1 - s, 1 + s] (TRAIN.AFFINE_SCALE)')
    parser.add_argument("--affine_translate", type=float, help='largest translation per axis as a fraction of the side (TRAIN.AFFINE_TRANSLATE)')
    parser.add_argument("--optimizer", type=str, help='training optimizer')
    parser.add_argument("--scheduler", type=str, help='learning rate scheduler')
    parser.add_argument("--base_lr", type=float, help='base learning rate')
    parser.add_argument("--min_lr", type=float, help='minimum learning rate')
    parser.add_argument("--weight_decay", type=float, help='weight decay')
    parser.add_argument("--grad_clip", type=float, help='gradient clipping')
    parser.add_argument("--batch_size", type=int, help='batch size')
    parser.add_argument("--num_workers", type=int, help='number of workers for dataloader')
    parser.add_argument("--max_epochs", type=int, help='max epoch')
    parser.add_argument("--lock", action='store_true')
    parser.add_argument("--layer_decay", type=float, help='layer-wise learning-rate decay of the backbone, in (0, 1]; 1 = off')
    parser.add_argument("--wd_exclude_1d", action='store_true', help='no weight decay on biases, norm scales, tokens and the position table')
    parser.add_argument("--drop_path", type=float, help='stochastic depth rate of the backbone (VIT.DROP_PATH_RATE), in [0, 1); 0 = off')
    # dataset parameters
    parser.add_argument('--dataset', type=str, help='dataset name')
    parser.add_argument('--train_csv_path', type=str, help='path to train csv file')
    parser.add_argument('--val_csv_path', type=str, help='path to val csv file')
    parser.add_argument('--test_csv_path', type=str, help='path to test csv file')
    args, _ = parser.parse_known_args()
    return args, get_config(args)


def build_model(config, device):
    v = config.VIT
    if config.MAE.NORM_LAYER == 'layernorm':
        norm_layer = nn.LayerNorm
    elif config.MAE.NORM_LAYER == 'rmsnorm':
        norm_layer = RMSNorm
    else:
        raise ValueError(f"Normalization layer {config.MAE.NORM_LAYER} not supported")
    model = ViTBackbone(in_chans=v.IN_CHANS, img_size=v.INPUT_SIZE, patch_size=v.PATCH_SIZE, hidden_size=v.HIDDEN_SIZE, mlp_dim=v.MLP_DIM,
                        num_layers=v.NUM_LAYERS, num_heads=v.NUM_HEADS, patch_embed=v.PATCH_EMBED, pos_embed=v.POS_EMBED,
                        classification=v.CLASSIFICATION, num_classes=config.DATA.NUM_CLASSES, dropout_rate=v.DROPOUT_RATE,
                        spatial_dims=v.SPATIAL_DIMS, num_register_tokens=v.NUM_REGISTER_TOKENS, qkv_bias=v.USE_BIAS,
                        lora=config.TRAIN.LORA, norm_layer=norm_layer, compute_dtype=config.MAE.COMPUTE_DTYPE,
                        drop_path_rate=v.DROP_PATH_RATE, patch_dropout=0.0)
    head = SegmentationHead(dim=v.HIDDEN_SIZE, patch_size=v.PATCH_SIZE, num_classes=config.SEG.NUM_CLASSES)
    return model.to(device), head.to(device)


def main(config, logger):
    if config.MODEL.NAME != "vit":
        raise ValueError(f"Backbone {config.MODEL.NAME} not supported")
    check_segmentation_mode(config)
    if not torch.cuda.is_available():
        raise SystemExit("main_segmentation.py (HIP) needs an MI355X: the path has no CPU fallback")
    device = torch.device("cuda", torch.cuda.current_device())
    bs, v, g = config.DATA.BATCH_SIZE, config.VIT, config.SEG
    logger.info(f"Segmentation: {g.NUM_CLASSES} classes, loss {g.CE_WEIGHT} * CE + {g.DICE_WEIGHT} * Dice, class weights "
                f"{list(g.CLASS_WEIGHT) or None}, ignore index {g.IGNORE_INDEX}")
    if g.AFFINE_PROB > 0:
        t = config.TRAIN
        logger.info(f"Random affine of scans and masks: SEG.AFFINE_PROB {g.AFFINE_PROB}, SEG.AFFINE_OUTSIDE {g.AFFINE_OUTSIDE}, TRAIN.AFFINE_ROTATE "
                    f"{list(t.AFFINE_ROTATE)} degrees, TRAIN.AFFINE_SCALE {t.AFFINE_SCALE}, TRAIN.AFFINE_TRANSLATE {t.AFFINE_TRANSLATE}")
    if config.DATA.SYNTHETIC:
        nb = max(1, config.DATA.SYNTHETIC_SAMPLES // bs)
        mk = lambda k, salt: SyntheticSegmented(k, bs, v.IN_CHANS, v.INPUT_SIZE, g.NUM_CLASSES, device, config.SEED + salt)
        train_loader, val_loader, test_loader = mk(nb, 0), mk(max(1, nb // 4), 1000), mk(max(1, nb // 4), 2000)
        affine, outside = segmentation_affine(config, config.SEED + dist.get_rank())
        if affine is not None:  # the fixed batches resampled anew every epoch: the affine alone, no flips and no shift
            train_loader = AugmentedSegmented(train_loader, DeviceAugment(flip_prob=0.0, shift_offsets=0.0, shift_prob=0.0, affine=affine), outside)
    else:
        from headct_foundation_amd.data import get_segmentation_dataloaders
        train_loader, val_loader, test_loader = get_segmentation_dataloaders(config, device, dist.get_rank(), dist.get_world_size())

    model, head = build_model(config, device)
    load_model(config, model, None, logger)
    if config.TRAIN.LOCK:
        for p in model.parameters():
            p.requires_grad_(False)
    if config.TRAIN.LORA:
        set_requires_grad_false(model, lora=config.TRAIN.LORA)
    logger.info(f"Total trainable parameters: {sum(p.numel() for p in model.parameters() if p.requires_grad)} (backbone), "
                f"{sum(p.numel() for p in head.parameters())} (head)")

    total = len(train_loader) * config.TRAIN.MAX_EPOCHS
    warmup = int(config.TRAIN.PER_WARMUP * total)
    lr_m, min_m, lr_c, min_c = learning_rates(config)
    config.defrost()
    config.TRAIN.MIN_LR = min_m
    config.freeze()
    logger.info(f"Effective Learning Rate: {config.TRAIN.BASE_LR}, Effective Batch Size: {bs * dist.get_world_size()}, "
                f"Max Epochs: {config.TRAIN.MAX_EPOCHS}")
    logger.info(f"Number of Warmup Steps: {warmup}, Total Steps: {total}")
    opt_c = get_optimizer(config, lr_c, [head])
    sch_c = get_lr_scheduler(config, opt_c, warmup, total, min_c)
    if config.TRAIN.LOCK:
        optimizers, schedulers = [opt_c], [sch_c]
    else:
        opt_m = get_optimizer(config, lr_m, [model])
        if config.TRAIN.LAYER_DECAY != 1.0:
            opt_m.set_scales(layer_decay_scales(model, config.TRAIN.LAYER_DECAY), no_decay_scales(model) if config.TRAIN.WD_EXCLUDE_1D else None)
        optimizers, schedulers = [opt_m, opt_c], [get_lr_scheduler(config, opt_m, warmup, total, min_m), sch_c]
    if config.TRAIN.LAYER_DECAY != 1.0 and config.TRAIN.LOCK:
        logger.info(f"TRAIN.LAYER_DECAY {config.TRAIN.LAYER_DECAY} is ignored: TRAIN.LOCK freezes the backbone")
    if config.TRAIN.WD_EXCLUDE_1D or (config.TRAIN.LAYER_DECAY != 1.0 and not config.TRAIN.LOCK):
        for what, opt in zip(("backbone", "head") if len(optimizers) == 2 else ("head",), optimizers):
            logger.info(f"{what} {describe_scales(opt.scales())}")
    best_dice, best_model, best_head = trainer(config=config, model=model, head=head, train_loader=train_loader, val_loader=val_loader,
                                               optimizers=optimizers, schedulers=schedulers, start_epoch=0, max_epochs=config.TRAIN.MAX_EPOCHS,
                                               val_every=config.TRAIN.VAL_EVERY, logger=logger, device=device)
    logger.info(f"train completed, best validation Dice: {best_dice:.4f} ")
    out = tester(config=config, model=best_model, head=best_head, test_loader=test_loader, logger=logger, device=device)
    logger.info(f"test completed, test loss: {out['loss']:.4f} ")
    cleanup()


if __name__ == "__main__":
    args, config = parse_option()
    init_distributed_mode(args)
    rank = dist.get_rank()
    seed = config.SEED + rank
    random.seed(seed); np.random.seed(seed); torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)
    logger = create_logger(output_dir=config.LOG.OUTPUT_DIR, dist_rank=rank, name=config.LOG.FILENAME)
    if rank == 0 and config.OUTPUT:
        os.makedirs(config.OUTPUT, exist_ok=True)
        with open(os.path.join(config.OUTPUT, f"{config.LOG.FILENAME}.json"), "w") as f:
            f.write(config.dump())
    logger.info(config.dump())
    logger.info(json.dumps(vars(args)))
    main(config, logger)
