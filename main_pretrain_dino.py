"""DINO pre-training entry point on the HIP path: the reference's CLI flags (main_pretrain_dino.py:36-75) and flow (:78-290).

  torchrun --nnodes 1 --nproc_per_node N --master-addr 127.0.0.1 main_pretrain_dino.py --local_rank 0 --model_name dino \
      --batch_size 8 --max_epochs 200 --base_lr 5e-4 --cfg configs/dino/dino_HeadCT.yaml --optimizer AdamW --scheduler cosine

Student and momentum teacher are MultiCropWrapper(ViTBackbone, DINOHead) pairs; the teacher starts as a copy of the student
and is only ever written by the momentum update.  Data: synthetic multi-crop batches (2 global + DINO.LOCAL_CROP_NUM local crops,
all at VIT.INPUT_SIZE as the reference resizes them): independent noise crops by default, or with DATA.DEVICE_AUGMENT True the
reference's DataAugmentationDINO3D on the device (DeviceAugmentDINO3D behind MultiCropLoader) over synthetic fp16 volumes.
With DATA.SYNTHETIC False the same augmentation runs over the cached scans of the three CSVs (PretrainVolumes).
"""
import argparse
import json
import os
import random

os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC for RCCL between ranks (before HIP initialises)

import numpy as np
import torch
import torch.distributed as dist

from config import get_config
from engine_pretrain_dino import tester, trainer
from headct_foundation_amd.data import DeviceAugmentDINO3D, MultiCropLoader, SyntheticVolumes, pretrain_volume_loaders
from headct_foundation_amd.dino import DINOLoss, DinoDataParallel, DinoOptimizer, SyntheticCrops, get_wd_scheduler, wd_cosine_scheduler
from headct_foundation_amd.dino_model import DINOHead, MultiCropWrapper, ViTBackbone
from headct_foundation_amd.ibot import IBOTPatchLoss, IBotMaskGenerator, IBotObjective
from headct_foundation_amd.lr_sched import get_lr_scheduler
from headct_foundation_amd.misc import cleanup, init_distributed_mode
from headct_foundation_amd.param_scales import describe_scales, no_decay_scales
from logger import create_logger


def parse_option():
    parser = argparse.ArgumentParser('HIP DINO training and evaluation script', add_help=False)
    parser.add_argument('--cfg', type=str, required=True, metavar="FILE", help='path to config file')
    parser.add_argument("--opts", help="Modify config options using the command-line", default=None, nargs='+')
    # distributed training
    parser.add_argument("--local_rank", type=int, default=int(os.environ.get("LOCAL_RANK", 0)), help='local rank')
    parser.add_argument('--dist-backend', default='nccl', help='parsed and ignored, like the reference')
    parser.add_argument('--dist-url', default='env://', help='parsed and ignored, like the reference')
    parser.add_argument("--seed", type=int, help='seed')
    parser.add_argument("--use_amp", action='store_true')
    # wandb configs
    parser.add_argument("--use_wandb", action='store_true')
    parser.add_argument("--wandb_project", type=str, default="monai-test")
    # model parameters
    parser.add_argument("--model_name", type=str, help='model name')
    parser.add_argument("--model_load_path", type=str, help='path to trained model')
    parser.add_argument("--optimizer", type=str, help='training optimizer')
    parser.add_argument("--scheduler", type=str, help='learning rate scheduler')
    parser.add_argument("--base_lr", type=float, help='base learning rate')
    parser.add_argument("--min_lr", type=float, help='minimum learning rate')
    parser.add_argument("--weight_decay", type=float, help='weight decay')
    parser.add_argument("--grad_clip", type=float, help='gradient clipping')
    parser.add_argument("--batch_size", type=int, help='batch size')
    parser.add_argument("--num_workers", type=int, help='number of workers for dataloader')
    parser.add_argument("--max_epochs", type=int, help='max epoch')
    parser.add_argument("--wd_exclude_1d", action='store_true', help='no weight decay on biases, norm scales, tokens and the position table')
    parser.add_argument("--drop_path", type=float, help="stochastic depth rate of the student's backbone (VIT.DROP_PATH_RATE), in [0, 1); 0 = off")
    parser.add_argument("--centering", type=str, help="teacher distribution of the DINO loss (DINO.CENTERING): 'centering' (EMA centre) or 'sinkhorn_knopp'")
    parser.add_argument("--koleo_weight", type=float, help="weight of the KoLeo regulariser on the student's class tokens (DINO.KOLEO_WEIGHT); 0 = off")
    parser.add_argument("--ibot_weight", type=float, help="weight of the iBOT masked patch-token loss (DINO.IBOT_WEIGHT); 0 = off")
    parser.add_argument("--ibot_mask_ratio", type=float, nargs=2, metavar=("LO", "HI"), help="range of the masked share of a masked global crop (DINO.IBOT_MASK_RATIO)")
    parser.add_argument("--ibot_mask_prob", type=float, help="share of the global crops that are masked per step (DINO.IBOT_MASK_PROB)")
    # dataset parameters
    parser.add_argument('--train_csv_path', type=str, help='path to train csv file')
    parser.add_argument('--val_csv_path', type=str, help='path to val csv file')
    parser.add_argument('--test_csv_path', type=str, help='path to test csv file')
    args, _ = parser.parse_known_args()
    return args, get_config(args)


def build_pair(config, device, drop_path_rate: float = 0.0, return_cls: bool = False):
    """MultiCropWrapper(ViTBackbone, DINOHead) from the VIT.* / DINO.* blocks (main_pretrain_dino.py:107-172).  `drop_path_rate`: the
    student's backbone takes VIT.DROP_PATH_RATE, the teacher's 0.  `return_cls`: the student's under DINO.KOLEO_WEIGHT > 0.  With
    DINO.IBOT_WEIGHT > 0 both backbones carry a `mask_token` (the momentum update needs equal flat layouts; the teacher's is never read)."""
    v, d = config.VIT, config.DINO
    backbone = ViTBackbone(in_chans=v.IN_CHANS, img_size=v.INPUT_SIZE, patch_size=v.PATCH_SIZE, hidden_size=v.HIDDEN_SIZE, mlp_dim=v.MLP_DIM,
                           num_layers=v.NUM_LAYERS, num_heads=v.NUM_HEADS, patch_embed=v.PATCH_EMBED, pos_embed=v.POS_EMBED,
                           classification=v.CLASSIFICATION, num_classes=config.DATA.NUM_CLASSES, dropout_rate=v.DROPOUT_RATE,
                           spatial_dims=v.SPATIAL_DIMS, num_register_tokens=v.NUM_REGISTER_TOKENS, qkv_bias=v.USE_BIAS,
                           compute_dtype=config.MAE.COMPUTE_DTYPE, drop_path_rate=drop_path_rate, mask_token=config.DINO.IBOT_WEIGHT > 0)
    head = DINOHead(in_dim=v.HIDDEN_SIZE, out_dim=d.HEAD_N_PROTOTYPES, hidden_dim=d.HEAD_HIDDEN_DIM, bottleneck_dim=d.BOTTLENECK_DIM,
                    nlayers=d.HEAD_N_LAYERS, use_bn=d.USE_BN, norm_last_layer=d.NORM_LAST_LAYER, compute_dtype=config.MAE.COMPUTE_DTYPE)
    return MultiCropWrapper(backbone, head, return_cls=return_cls).to(device)


def load_pretrained(config, model, momentum_model, logger):
    """MODEL.PRETRAINED -> checkpoint dict (or None); `module.` / `_orig_mod.` prefixes dropped, non-strict (misc.py:72-96)."""
    if not config.MODEL.PRETRAINED:
        return None
    ckpt = torch.load(config.MODEL.PRETRAINED, map_location="cpu", weights_only=True)
    strip = lambda sd: {k.replace("module.", "").replace("_orig_mod.", ""): t for k, t in sd.items()}
    logger.info(f"Load Pretrained Model: {model.load_state_dict(strip(ckpt['state_dict']), strict=False)} for Architecture: {config.MODEL.NAME}")
    if ckpt.get('momentum_model_state_dict') is not None:
        report = momentum_model.load_state_dict(strip(ckpt['momentum_model_state_dict']), strict=False)
        logger.info(f"Load Pretrained Momentum Model: {report} for Architecture: {config.MODEL.NAME}")
    return ckpt


def build_loaders(config, device, rank, world):
    """train / val / test loaders of crop lists, seeded SEED + rank + salt.  DATA.DEVICE_AUGMENT: every loader is the same
    DataAugmentationDINO3D over cached-format volumes (main_pretrain_dino.py:83-95 of the reference), here on the device.
    DATA.SYNTHETIC False: that augmentation over the cached scans of DATA.*_CSV_PATH."""
    if not config.DATA.SYNTHETIC:
        dino_aug = lambda salt: DeviceAugmentDINO3D(list(config.MODEL.ROI), config.DINO.GLOBAL_CROP_SIZE, config.DINO.LOCAL_CROP_SIZE,
                                                    config.DINO.LOCAL_CROP_NUM, seed=config.SEED + rank + salt, field=config.DINO.CROP_FIELD,
                                                    local_field=config.DINO.LOCAL_CROP_FIELD)
        bases = pretrain_volume_loaders(config, device, rank, world, config.VIT.INPUT_SIZE, config.VIT.IN_CHANS)
        return [MultiCropLoader(b, dino_aug(salt)) for b, salt in zip(bases, (0, 1000, 2000))]
    n_crops = 2 + config.DINO.LOCAL_CROP_NUM
    bs = config.DATA.BATCH_SIZE
    nb = max(1, config.DATA.SYNTHETIC_SAMPLES // max(1, world) // bs)
    sizes = ((nb, 0), (max(1, nb // 4), 1000), (max(1, nb // 4), 2000))
    if not config.DATA.DEVICE_AUGMENT:
        return [SyntheticCrops(k, bs, n_crops, config.VIT.IN_CHANS, config.VIT.INPUT_SIZE, device, config.SEED + rank + salt) for k, salt in sizes]
    roi = list(config.MODEL.ROI)
    if roi != [config.VIT.INPUT_SIZE] * 3:
        raise ValueError(f"MODEL.ROI {roi} is the size of the crops and must be what the backbone is built for "
                         f"(VIT.INPUT_SIZE {config.VIT.INPUT_SIZE}); the position table is not resized on every call")
    mk = lambda k, salt: MultiCropLoader(
        SyntheticVolumes(k, bs, config.VIT.IN_CHANS, roi[0], device, config.SEED + rank + salt, dtype=torch.float16),
        DeviceAugmentDINO3D(roi, config.DINO.GLOBAL_CROP_SIZE, config.DINO.LOCAL_CROP_SIZE, config.DINO.LOCAL_CROP_NUM,
                            seed=config.SEED + rank + salt, field=config.DINO.CROP_FIELD, local_field=config.DINO.LOCAL_CROP_FIELD))
    return [mk(k, salt) for k, salt in sizes]


def main(config, wandb_run, logger):
    if config.MODEL.NAME != "dino":
        raise ValueError(f"Model {config.MODEL.NAME} not supported")
    if not torch.cuda.is_available():
        raise SystemExit("main_pretrain_dino.py (HIP) needs an MI355X: the DINO path has no CPU fallback")
    rank, world = dist.get_rank(), dist.get_world_size()
    device = torch.device("cuda", torch.cuda.current_device())
    n_crops = 2 + config.DINO.LOCAL_CROP_NUM
    bs = config.DATA.BATCH_SIZE
    train_loader, val_loader, test_loader = build_loaders(config, device, rank, world)

    student = build_pair(config, device, config.VIT.DROP_PATH_RATE, return_cls=config.DINO.KOLEO_WEIGHT > 0)
    teacher = build_pair(config, device)
    teacher.load_state_dict(student.state_dict())  # the momentum teacher starts from the student's weights
    ckpt = load_pretrained(config, student, teacher, logger)
    for p in teacher.parameters():
        p.requires_grad_(False)
    model = DinoDataParallel(student, device_ids=[device])
    momentum_model = DinoDataParallel(teacher, device_ids=[device])

    total = len(train_loader) * config.TRAIN.MAX_EPOCHS
    warmup = int(config.TRAIN.PER_WARMUP * total)
    config.defrost()
    config.TRAIN.BASE_LR = config.TRAIN.BASE_LR * bs * world / 256  # linear scaling rule, main_pretrain_dino.py:209-212
    config.TRAIN.MIN_LR = config.TRAIN.BASE_LR * 1e-3
    config.freeze()
    logger.info(f"Effective Learning Rate: {config.TRAIN.BASE_LR}, Effective Batch Size: {bs * world}, Max Epochs: {config.TRAIN.MAX_EPOCHS}")
    logger.info(f"Number of Warmup Steps: {warmup}, Total Steps: {total}")
    optimizer = DinoOptimizer(model, lr=config.TRAIN.BASE_LR, betas=(config.TRAIN.BETA1, config.TRAIN.BETA2), weight_decay=config.TRAIN.WEIGHT_DECAY,
                              kind=config.TRAIN.OPTIMIZER, momentum=config.TRAIN.MOMENTUM)
    if config.TRAIN.WD_EXCLUDE_1D:  # the weight-decay schedule (0.04 -> 0.4) then leaves gains, biases and tokens alone
        optimizer.set_scales(wd_scale=no_decay_scales(student))
        logger.info(describe_scales(optimizer.scales()))
    lr_scheduler = get_lr_scheduler(config, optimizer.primary, warmup, total, config.TRAIN.MIN_LR)
    wd_scheduler = get_wd_scheduler(config, len(train_loader))
    momentum_scheduler = wd_cosine_scheduler(config.DINO.MOMENTUM_TEACHER, config.DINO.MOMENTUM_TEACHER_END, config.TRAIN.MAX_EPOCHS, len(train_loader))
    first_epoch = 0
    if ckpt is not None:
        if 'optimizer' in ckpt:
            optimizer.load_state_dict(ckpt['optimizer'])
        if 'scheduler' in ckpt:
            lr_scheduler.load_state_dict(ckpt['scheduler'])
        first_epoch = ckpt.get('epoch', 0)
    criterion = DINOLoss(out_dim=config.DINO.HEAD_N_PROTOTYPES, ncrops=n_crops, warmup_teacher_temp=config.DINO.WARMUP_TEACHER_TEMP,
                         teacher_temp=config.DINO.TEACHER_TEMP, warmup_teacher_temp_epochs=config.DINO.WARMUP_TEACHER_EPOCHS,
                         nepochs=config.TRAIN.MAX_EPOCHS, centering=config.DINO.CENTERING, sk_iters=config.DINO.SK_ITERS).to(device)
    if config.DINO.IBOT_WEIGHT > 0:  # the engine finds the patch objective on the criterion; masks are drawn per step, seeded per rank
        patch_loss = IBOTPatchLoss(out_dim=config.DINO.HEAD_N_PROTOTYPES, warmup_teacher_temp=config.DINO.WARMUP_TEACHER_TEMP,
                                   teacher_temp=config.DINO.TEACHER_TEMP, warmup_teacher_temp_epochs=config.DINO.WARMUP_TEACHER_EPOCHS,
                                   nepochs=config.TRAIN.MAX_EPOCHS, centering=config.DINO.CENTERING, sk_iters=config.DINO.SK_ITERS).to(device)
        masks = IBotMaskGenerator(config.VIT.INPUT_SIZE // config.VIT.PATCH_SIZE, tuple(config.DINO.IBOT_MASK_RATIO), config.DINO.IBOT_MASK_PROB,
                                  seed=config.SEED + rank + 3000)
        criterion.ibot = IBotObjective(config.DINO.IBOT_WEIGHT, masks, patch_loss, config.VIT.NUM_REGISTER_TOKENS)
    best = trainer(config=config, model=model, momentum_model=momentum_model, train_loader=train_loader, val_loader=val_loader,
                   optimizer=optimizer, lr_scheduler=lr_scheduler, wd_scheduler=wd_scheduler, momentum_scheduler=momentum_scheduler,
                   dino_criterion=criterion, start_epoch=first_epoch, max_epochs=config.TRAIN.MAX_EPOCHS, val_every=config.TRAIN.VAL_EVERY,
                   logger=logger, device=device, wandb_run=wandb_run)
    logger.info(f"train completed, best train dino loss: {best:.4f}")
    held_out = tester(config=config, model=model, test_loader=test_loader, dino_criterion=criterion, momentum_model=momentum_model,
                      logger=logger, device=device, wandb_run=wandb_run)
    logger.info(f"test completed, best test dino loss: {held_out:.4f}")
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
