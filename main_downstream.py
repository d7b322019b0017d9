"""Downstream fine-tuning / probing entry point on the HIP path: the reference's CLI (main_downstream.py:34-86) and flow
(:88-290).

  torchrun --nnodes 1 --nproc_per_node 1 main_downstream.py --local_rank 0 --model_name vit --cfg CFG.yaml \
      --model_load_path PRETRAINED.pt --classifier linear --grad_clip 1.0 --batch_size 64 [--lock]

Backbone: `ViTBackbone` from VIT.* (register tokens included) in MAE.COMPUTE_DTYPE; head: TRAIN.CLASSIFIER `linear` (class
token) or `attentive` (every token, 12 heads, one query); two fused optimizers of the TRAIN.OPTIMIZER kind (backbone at BASE_LR, head at 100 x BASE_LR;
MIN_LR = BASE_LR * 1e-3, x100 for the head) with TRAIN.SCHEDULER warm-up schedules, only the head's with TRAIN.LOCK.  Data: the labelled
scans of DATA.TRAIN / VAL / TEST_CSV_PATH (DATA.DATASET, TRAIN.LABEL_NAME; class-balanced draws, or DATA.FEW_SHOTS rows per class)
through the fp16 cache and the device-resident pool, or synthetic labelled volumes (DATA.SYNTHETIC).

Multi-label mode (an addition of this build): `--label_names NAME [NAME ...]` (TRAIN.LABEL_NAMES; `all` = every label of
DATA.DATASET) trains ONE model with a sigmoid output per name on `bce_with_logits` instead of one binary model per
TRAIN.LABEL_NAME; `--pos_weight balanced` weighs each label's positive term by the imbalance the sampler leaves.

Mixup, CutMix and label smoothing (additions of this build): `--mixup ALPHA`, `--cutmix ALPHA`, `--smoothing EPS` (TRAIN.MIXUP,
TRAIN.CUTMIX, TRAIN.LABEL_SMOOTHING; TRAIN.MIX_PROB / MIX_SWITCH_PROB / MIX_MODE as timm's Mixup) mix each training batch on the
device and train on the soft-target loss; validation and test see plain batches and the plain loss.  All three at 0 (the default)
hand the engine the criterion of a run without them.

Random 3-D affine (an addition of this build): `--affine_prob P --affine_rotate DEG [DEG DEG] --affine_scale S --affine_translate F`
(TRAIN.AFFINE_PROB / ROTATE / SCALE / TRANSLATE / ISOTROPIC) rotates, zooms and translates each training scan with probability P in
the launch that assembles the batch; validation and test keep the plain cast.  P = 0 (the default) is a run without it.

Patch dropout (an addition of this build): `--patch_dropout R` (VIT.PATCH_DROPOUT, 0 <= R < 1) lets every training step embed and run a
random int(L * (1 - R)) of each scan's L patch tokens; validation and test run all of them.  Ignored with --lock.  0 (the default) is a
run without it.
"""
import argparse
import json
import os
import random

import numpy as np
import torch
import torch.distributed as dist
import torch.nn as nn

from config import get_config
from engine_downstream import tester, trainer
from headct_foundation_amd.classifier import AttentionClassifier, LinearClassifier, bce_with_logits, cross_entropy
from headct_foundation_amd.data import (CLASS_MAPPINGS, SyntheticLabelled, SyntheticMultiLabelled, expand_label_names, get_fewshots_dataloaders,
                                        get_finetune_dataloaders)
from headct_foundation_amd.dino_model import ViTBackbone
from headct_foundation_amd.layers import RMSNorm
from headct_foundation_amd.lr_sched import get_lr_scheduler
from headct_foundation_amd.mixup import MixedCriterion, Mixup
from headct_foundation_amd.misc import cleanup, init_distributed_mode, load_model, set_requires_grad_false
from headct_foundation_amd.optim import get_optimizer
from headct_foundation_amd.param_scales import describe_scales, layer_decay_scales, no_decay_scales
from logger import create_logger


def parse_option():
    parser = argparse.ArgumentParser('HIP downstream training and evaluation script', add_help=False)
    parser.add_argument('--cfg', type=str, required=True, metavar="FILE", help='path to config file')
    parser.add_argument("--opts", help="Modify config options using the command-line", default=None, nargs='+')
    parser.add_argument("--preds_save_name", type=str, help='save name tag for predictions')
    # distributed training
    parser.add_argument("--local_rank", type=int, default=int(os.environ.get("LOCAL_RANK", 0)), help='local rank')
    parser.add_argument('--dist-backend', default='nccl', help='parsed and ignored, like the reference')
    parser.add_argument('--dist-url', default='env://', help='parsed and ignored, like the reference')
    parser.add_argument("--seed", type=int, help='seed')
    parser.add_argument("--use_amp", action='store_true')
    # wandb configs
    parser.add_argument("--use_wandb", action='store_true')
    parser.add_argument("--filename", type=str, default="monai-test")
    parser.add_argument("--wandb_project", type=str, default="monai-test")
    # model parameters
    parser.add_argument("--model_name", type=str, help='model name')
    parser.add_argument("--model_load_path", type=str, help='path to trained model')
    parser.add_argument("--classifier", type=str, help='classifier name (linear or attentive)')
    parser.add_argument("--label_name", type=str, help='label name for downstream tasks')
    parser.add_argument("--label_names", type=str, nargs='+', help="multi-label mode: one sigmoid output per name ('all' = every label of the dataset)")
    parser.add_argument("--pos_weight", type=str, choices=['none', 'balanced'], help='multi-label mode: weight of the positive term per label')
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
    parser.add_argument("--patch_dropout", type=float, help='share of patch tokens each training step drops (VIT.PATCH_DROPOUT), in [0, 1); 0 = off')
    parser.add_argument("--mixup", type=float, help='mixup alpha (TRAIN.MIXUP), >= 0; 0 = off')
    parser.add_argument("--cutmix", type=float, help='CutMix alpha (TRAIN.CUTMIX), >= 0; 0 = off')
    parser.add_argument("--smoothing", type=float, help='label smoothing (TRAIN.LABEL_SMOOTHING), in [0, 1); 0 = off; softmax mode only')
    parser.add_argument("--affine_prob", type=float, help='probability of the random 3-D affine per training sample (TRAIN.AFFINE_PROB); 0 = off')
    parser.add_argument("--affine_rotate", type=float, nargs='+', help='rotation range in degrees, one angle or one per axis (TRAIN.AFFINE_ROTATE)')
    parser.add_argument("--affine_scale", type=float, help='zoom range s: factor ~ U(1 - s, 1 + s) (TRAIN.AFFINE_SCALE), in [0, 1)')
    parser.add_argument("--affine_translate", type=float, help="translation range as a fraction of the volume's side (TRAIN.AFFINE_TRANSLATE), in [0, 1)")
    # dataset parameters
    parser.add_argument('--dataset', type=str, help='dataset name')
    parser.add_argument('--train_csv_path', type=str, help='path to train csv file')
    parser.add_argument('--val_csv_path', type=str, help='path to val csv file')
    parser.add_argument('--test_csv_path', type=str, help='path to test csv file')
    parser.add_argument("--few_shots", type=int, help='number of few shots')
    args, _ = parser.parse_known_args()
    return args, get_config(args)


def learning_rates(config):
    """(backbone lr, backbone min lr, head lr, head min lr) of main_downstream.py:218-240: MIN_LR = BASE_LR * 1e-3, x100 for the head."""
    base = config.TRAIN.BASE_LR
    return base, base * 1e-3, base * 1e2, base * 1e-3 * 1e2


def multilabel_names(config) -> list:
    """The labels of multi-label mode ([]: the single-label path): TRAIN.LABEL_NAMES with 'all' expanded, checked against the
    dataset's labels unless the data is synthetic, where the names are free."""
    names = list(config.TRAIN.LABEL_NAMES)
    if not names:
        return []
    if config.DATA.NUM_CLASSES != 2:
        raise ValueError(f"TRAIN.LABEL_NAMES makes every label one binary (sigmoid) output: DATA.NUM_CLASSES must be 2, not {config.DATA.NUM_CLASSES}")
    if config.DATA.SYNTHETIC and names != ["all"]:
        return names
    names = expand_label_names(config.DATA.DATASET, names)
    known = CLASS_MAPPINGS.get(config.DATA.DATASET)
    if known is None:
        raise ValueError(f"Unrecognized dataset: {config.DATA.DATASET}")
    unknown = [n for n in names if n not in known]
    if unknown or len(set(names)) != len(names):
        raise ValueError(f"TRAIN.LABEL_NAMES {names}: {unknown or 'repeated names'} not among dataset {config.DATA.DATASET}'s labels {known}")
    return names


def build_criterion(config, pos_weight=None, seed: int = 0, logger=None):
    """What the engine gets as `criterion`: `cross_entropy` (or the `bce_with_logits` closure of multi-label mode) exactly as before
    when TRAIN.MIXUP, TRAIN.CUTMIX and TRAIN.LABEL_SMOOTHING are all 0, else a `MixedCriterion` whose draws are seeded by `seed`."""
    t = config.TRAIN
    names = list(t.LABEL_NAMES)
    if t.LABEL_SMOOTHING > 0 and names:
        raise ValueError("TRAIN.LABEL_SMOOTHING is defined for the softmax mode only: it cannot be combined with TRAIN.LABEL_NAMES")
    if not (t.MIXUP > 0 or t.CUTMIX > 0 or t.LABEL_SMOOTHING > 0):
        return (lambda logits, target: bce_with_logits(logits, target, pos_weight)) if names else cross_entropy
    mix = None
    if t.MIXUP > 0 or t.CUTMIX > 0:
        mix = Mixup(t.MIXUP, t.CUTMIX, prob=t.MIX_PROB, switch_prob=t.MIX_SWITCH_PROB, mode=t.MIX_MODE, seed=seed)
    if logger is not None:
        logger.info(f"Fine-tuning recipe: TRAIN.MIXUP {t.MIXUP}, TRAIN.CUTMIX {t.CUTMIX} (prob {t.MIX_PROB}, switch {t.MIX_SWITCH_PROB}, mode "
                    f"{t.MIX_MODE}, seed {seed}), TRAIN.LABEL_SMOOTHING {t.LABEL_SMOOTHING}: training batches are mixed with their "
                    "reverse on the device; validation and test use the plain loss")
    return MixedCriterion(mix, t.LABEL_SMOOTHING, multilabel=bool(names), pos_weight=pos_weight)


def build_model(config, device):
    v = config.VIT
    num_outputs = len(multilabel_names(config)) or config.DATA.NUM_CLASSES
    if config.MAE.NORM_LAYER == 'layernorm':  # main_downstream.py:111-116
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
                        drop_path_rate=v.DROP_PATH_RATE, patch_dropout=0.0 if config.TRAIN.LOCK else v.PATCH_DROPOUT)  # a frozen backbone's features stay the deterministic ones
    if config.TRAIN.CLASSIFIER == 'linear':
        classifier = LinearClassifier(dim=v.HIDDEN_SIZE, num_classes=num_outputs, feature_grad=not config.TRAIN.LOCK)
    elif config.TRAIN.CLASSIFIER == 'attentive':
        classifier = AttentionClassifier(dim=v.HIDDEN_SIZE, num_classes=num_outputs, num_heads=12, num_queries=1,
                                         compute_dtype=config.MAE.COMPUTE_DTYPE)
    else:
        raise ValueError(f"Classifier {config.TRAIN.CLASSIFIER} not supported")
    return model.to(device), classifier.to(device)


def main(config, wandb_run, logger):
    if config.MODEL.NAME != "vit":
        raise ValueError(f"Backbone {config.MODEL.NAME} not supported")
    if config.DATA.NUM_CLASSES == 1:
        raise NotImplementedError(f"Unknown number of classes: {config.DATA.NUM_CLASSES}")
    if not torch.cuda.is_available():
        raise SystemExit("main_downstream.py (HIP) needs an MI355X: the path has no CPU fallback")
    device = torch.device("cuda", torch.cuda.current_device())
    bs, v = config.DATA.BATCH_SIZE, config.VIT
    names = multilabel_names(config)
    if names:  # the expanded names are what the engine, the log and the predictions pickle carry
        config.defrost()
        config.TRAIN.LABEL_NAMES = names
        config.freeze()
        logger.info(f"Multi-label mode: {len(names)} sigmoid outputs {names}, pos_weight {config.TRAIN.POS_WEIGHT}")
    pos_weight = None
    if config.DATA.SYNTHETIC:
        nb = max(1, config.DATA.SYNTHETIC_SAMPLES // bs)
        if names:
            mk = lambda k, salt: SyntheticMultiLabelled(k, bs, v.IN_CHANS, v.INPUT_SIZE, len(names), device, config.SEED + salt)
        else:
            mk = lambda k, salt: SyntheticLabelled(k, bs, v.IN_CHANS, v.INPUT_SIZE, config.DATA.NUM_CLASSES, device, config.SEED + salt)
        train_loader, val_loader, test_loader = mk(nb, 0), mk(max(1, nb // 4), 1000), mk(max(1, nb // 4), 2000)
    else:  # main_downstream.py:98-103
        get = get_finetune_dataloaders if config.DATA.FEW_SHOTS == -1 else get_fewshots_dataloaders
        train_loader, val_loader, test_loader, class_weights = get(config, device, dist.get_rank(), dist.get_world_size())
        if names:  # the fourth value is the loss's pos_weight [T] (TRAIN.POS_WEIGHT 'balanced') or None
            pos_weight = None if class_weights is None else class_weights.to(device)
            logger.info(f"Positive weights: {None if class_weights is None else class_weights.tolist()}")
        else:
            logger.info(f"Class weights: {None if class_weights is None else class_weights.tolist()}")
    t = config.TRAIN
    if t.AFFINE_PROB > 0 and config.DATA.SYNTHETIC:
        logger.info(f"TRAIN.AFFINE_PROB {t.AFFINE_PROB} is ignored: the synthetic volumes do not go through the loader's transforms")
    elif t.AFFINE_PROB > 0:
        logger.info(f"Random affine: TRAIN.AFFINE_PROB {t.AFFINE_PROB}, TRAIN.AFFINE_ROTATE {list(t.AFFINE_ROTATE)} degrees, TRAIN.AFFINE_SCALE "
                    f"{t.AFFINE_SCALE} ({'one factor' if t.AFFINE_ISOTROPIC else 'a factor per axis'}), TRAIN.AFFINE_TRANSLATE {t.AFFINE_TRANSLATE} of the "
                    f"side (seed {config.SEED + dist.get_rank()}): training scans are resampled in the launch that assembles the batch; "
                    "validation and test keep the plain cast")
    criterion = build_criterion(config, pos_weight, seed=config.SEED + dist.get_rank(), logger=logger)

    model, classifier = build_model(config, device)
    load_model(config, model, None, logger)
    if config.TRAIN.LOCK:
        for p in model.parameters():
            p.requires_grad_(False)
    if config.TRAIN.LORA:  # main_downstream.py:168-170: adapters, biases, norms and embeddings train; the rest is frozen
        set_requires_grad_false(model, lora=config.TRAIN.LORA)
    logger.info(f"Total trainable parameters: {sum(p.numel() for p in model.parameters() if p.requires_grad)}")

    total = len(train_loader) * config.TRAIN.MAX_EPOCHS
    warmup = int(config.TRAIN.PER_WARMUP * total)
    lr_m, min_m, lr_c, min_c = learning_rates(config)
    config.defrost()
    config.TRAIN.MIN_LR = min_m
    config.freeze()
    logger.info(f"Effective Learning Rate: {config.TRAIN.BASE_LR}, Effective Batch Size: {bs * dist.get_world_size()}, "
                f"Max Epochs: {config.TRAIN.MAX_EPOCHS}")
    logger.info(f"Number of Warmup Steps: {warmup}, Total Steps: {total}")
    opt_c = get_optimizer(config, lr_c, [classifier])
    sch_c = get_lr_scheduler(config, opt_c, warmup, total, min_c)
    if config.TRAIN.LOCK:
        optimizers, schedulers = [opt_c], [sch_c]
    else:
        opt_m = get_optimizer(config, lr_m, [model])
        if config.TRAIN.LAYER_DECAY != 1.0:  # the head is one layer above the backbone: scale 1 at its 100 x BASE_LR
            opt_m.set_scales(layer_decay_scales(model, config.TRAIN.LAYER_DECAY), no_decay_scales(model) if config.TRAIN.WD_EXCLUDE_1D else None)
        optimizers, schedulers = [opt_m, opt_c], [get_lr_scheduler(config, opt_m, warmup, total, min_m), sch_c]
    if config.TRAIN.LAYER_DECAY != 1.0 and config.TRAIN.LOCK:
        logger.info(f"TRAIN.LAYER_DECAY {config.TRAIN.LAYER_DECAY} is ignored: TRAIN.LOCK freezes the backbone")
    if config.VIT.DROP_PATH_RATE > 0.0:
        logger.info(f"VIT.DROP_PATH_RATE {config.VIT.DROP_PATH_RATE}: block j of {v.NUM_LAYERS} drops its residual branches per sample at rate "
                    f"{config.VIT.DROP_PATH_RATE} * j / {max(1, v.NUM_LAYERS - 1)}")
    if config.VIT.PATCH_DROPOUT > 0.0 and config.TRAIN.LOCK:
        logger.info(f"VIT.PATCH_DROPOUT {config.VIT.PATCH_DROPOUT} is ignored: TRAIN.LOCK freezes the backbone, whose features stay those of every patch")
    elif config.VIT.PATCH_DROPOUT > 0.0:
        logger.info(f"VIT.PATCH_DROPOUT {config.VIT.PATCH_DROPOUT}: each training sample keeps {model.patch_keep} of {model.num_patches} patches, "
                    f"{1 + model.num_register_tokens + model.patch_keep} tokens per sample instead of {model.num_tokens}; validation and test run every patch")
    if config.TRAIN.WD_EXCLUDE_1D or (config.TRAIN.LAYER_DECAY != 1.0 and not config.TRAIN.LOCK):
        for what, opt in zip(("backbone", "classifier") if len(optimizers) == 2 else ("classifier",), optimizers):
            logger.info(f"{what} {describe_scales(opt.scales())}")
    best_auroc, best_model, best_classifier = trainer(config=config, model=model, classifier=classifier, train_loader=train_loader,
                                            val_loader=val_loader, optimizers=optimizers, schedulers=schedulers, criterion=criterion,
                                            start_epoch=0, max_epochs=config.TRAIN.MAX_EPOCHS, val_every=config.TRAIN.VAL_EVERY,
                                            logger=logger, device=device, wandb_run=wandb_run)
    logger.info(f"train completed, best train loss: {best_auroc:.4f} ")
    test_loss = tester(config=config, model=best_model, classifier=best_classifier, test_loader=test_loader, criterion=criterion,
                       logger=logger, device=device, wandb_run=wandb_run)
    logger.info(f"test completed, best test loss: {test_loss:.4f} ")
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
    main(config, None, logger)
