"""Configuration surface of the reference (config.py:6-273), MAE-relevant tree kept key-for-key so the reference's
yaml files and `--opts` overrides load unchanged.  Built on headct_foundation_amd.cfgnode.CfgNode (yacs subset)."""
import math
import os

import yaml

from headct_foundation_amd.cfgnode import CfgNode as CN

_C = CN()
_C.BASE = ['']

_C.DATA = CN()
_C.DATA.BATCH_SIZE = 64
_C.DATA.BASE_PATH = '<path-to>/datasets'
_C.DATA.TRAIN_CSV_PATH = '<path-to>/datasets/train.csv'
_C.DATA.VAL_CSV_PATH = '<path-to>/datasets/val.csv'
_C.DATA.TEST_CSV_PATH = '<path-to>/datasets/test.csv'
_C.DATA.PIN_MEMORY = True
_C.DATA.NUM_WORKERS = 4
_C.DATA.CACHE_NUM = -1
_C.DATA.CACHE_RATE = 1.0
_C.DATA.CACHE_DIR = '<path-to>/cache_dir'
_C.DATA.DATASET = 'nyu'
_C.DATA.FEW_SHOTS = -1
_C.DATA.NUM_CLASSES = 2
# additions of this build (not in the reference): synthetic volumes when no dataset is mounted
_C.DATA.SYNTHETIC = False
_C.DATA.SYNTHETIC_SAMPLES = 8
# DINO entry point: cut the crops from synthetic fp16 volumes of MODEL.ROI on the device (DeviceAugmentDINO3D) instead of feeding noise crops
_C.DATA.DEVICE_AUGMENT = False
# fine-tuning loader: draws per rank and epoch of the class-balanced sampler (the reference hard-codes 500), and the byte budget of
# the device-resident pool of cache items, which DATA.CACHE_NUM / CACHE_RATE bound as they do MONAI's CacheDataset (0 = no pool)
_C.DATA.TRAIN_SAMPLES_PER_RANK = 500
_C.DATA.DEVICE_POOL_GB = 32.0

_C.MODEL = CN()
_C.MODEL.NAME = 'mae'
_C.MODEL.PRETRAINED = None
_C.MODEL.DIR = '<path-to>/model_saved'
_C.MODEL.SAVE_NAME = 'debug.pt'
_C.MODEL.ROI = [96, 96, 96]
_C.MODEL.IN_CHANS = 3

_C.MAE = CN()
_C.MAE.INPUT_SIZE = 96
_C.MAE.PATCH_SIZE = 16
_C.MAE.MASK_RATIO = 0.75
_C.MAE.IN_CHANS = 3
_C.MAE.DROPOUT_RATE = 0.0
_C.MAE.PATCH_EMBED = 'conv'
_C.MAE.POS_EMBED = 'sincos'
_C.MAE.NORM_LAYER = 'layernorm'
_C.MAE.SPATIAL_DIMS = 3
_C.MAE.NORM_PIX_LOSS = False
_C.MAE.RETURN_IMAGE = False
_C.MAE.ENCODER_EMBED_DIM = 768
_C.MAE.ENCODER_DEPTH = 12
_C.MAE.ENCODER_MLP_DIM = 3072
_C.MAE.ENCODER_NUM_HEADS = 12
_C.MAE.DECODER_EMBED_DIM = 768
_C.MAE.DECODER_DEPTH = 8
_C.MAE.DECODER_MLP_DIM = 2048
_C.MAE.DECODER_NUM_HEADS = 16
_C.MAE.USE_BIAS = False
# addition of this build: arithmetic of the HIP path ('bf16' = bf16 storage + MFMA, 'fp32' = parity mode)
_C.MAE.COMPUTE_DTYPE = 'bf16'

# DINO / VIT trees are kept so the reference's yaml files still merge; those paths are out of scope here.
_C.DINO = CN()
_C.DINO.GLOBAL_CROP_SIZE = [112, 112, 112]
_C.DINO.GLOBAL_CROP_NUM = 2
_C.DINO.LOCAL_CROP_SIZE = [64, 64, 64]
_C.DINO.LOCAL_CROP_NUM = 2
# the zero-padded field the global crops are cut from (ResizeWithPadOrCrop) and its centre crop for the local ones (transforms.py:73, 94)
_C.DINO.CROP_FIELD = 224
_C.DINO.LOCAL_CROP_FIELD = 192
_C.DINO.HEAD_N_LAYERS = 3
_C.DINO.HEAD_N_PROTOTYPES = 65536
_C.DINO.BOTTLENECK_DIM = 256
_C.DINO.HEAD_HIDDEN_DIM = 2048
_C.DINO.MOMENTUM_TEACHER = 0.994
_C.DINO.MOMENTUM_TEACHER_END = 1.0
_C.DINO.WARMUP_TEACHER_TEMP = 0.04
_C.DINO.TEACHER_TEMP = 0.07
_C.DINO.WARMUP_TEACHER_EPOCHS = 30
_C.DINO.DINO_LOSS_WEIGHT = 1.0
_C.DINO.USE_BN = True
_C.DINO.NORM_LAST_LAYER = True
_C.DINO.FREEZE_LAST_LAYER = 1
# additions of this build (DINOv2's class-token objective).  CENTERING: how the teacher distribution is kept from collapsing -- 'centering' is
# the reference's EMA centre, 'sinkhorn_knopp' runs SK_ITERS Sinkhorn-Knopp iterations over the batch of all ranks and needs no running state.
# KOLEO_WEIGHT > 0 adds that weight times the KoLeo regulariser of the student's class-token features of the two global crops (per rank) to
# the training loss; validation and test report the DINO term alone.  0.0 = off.
_C.DINO.CENTERING = 'centering'
_C.DINO.SK_ITERS = 3
_C.DINO.KOLEO_WEIGHT = 0.0
# iBOT masked patch-token loss (DINOv2's patch objective; an addition of this build).  IBOT_WEIGHT > 0 adds that weight times the loss between the
# student's masked patch tokens of the two global crops and the teacher's at the same positions; student and teacher backbones then carry a
# `mask_token`.  Per step int(2 B * IBOT_MASK_PROB) of the 2 B global crops are masked, block-wise in 3-D, at ratios spread over IBOT_MASK_RATIO
# [lo, hi].  Training only: validation and test report the DINO term alone.  0.0 = off: no parameter, launch, log line or checkpoint key changes.
_C.DINO.IBOT_WEIGHT = 0.0
_C.DINO.IBOT_MASK_RATIO = [0.1, 0.5]
_C.DINO.IBOT_MASK_PROB = 0.5

_C.VIT = CN()
_C.VIT.INPUT_SIZE = 96
_C.VIT.PATCH_SIZE = 12
_C.VIT.IN_CHANS = 3
_C.VIT.DROPOUT_RATE = 0.0
# addition of this build: stochastic depth (drop path) of the trainable ViT backbone, 0 <= r < 1; block j of L drops each of its two
# residual branches per sample at rate r * j / (L - 1) in training mode (headct_foundation_amd/dropout.py).  0.0 = off.
_C.VIT.DROP_PATH_RATE = 0.0
# addition of this build: patch dropout of the trainable ViT backbone when fine-tuning, 0 <= r < 1: in training mode each sample keeps a
# random int(L * (1 - r)) of its L patch tokens and the blocks run on those; validation and test see every patch
# (headct_foundation_amd/dropout.py).  0.0 = off.
_C.VIT.PATCH_DROPOUT = 0.0
_C.VIT.PATCH_EMBED = 'conv'
_C.VIT.POS_EMBED = 'sincos'
_C.VIT.NORM_LAYER = 'layernorm'
_C.VIT.SPATIAL_DIMS = 3
_C.VIT.NUM_LAYERS = 12
_C.VIT.NUM_HEADS = 12
_C.VIT.HIDDEN_SIZE = 768
_C.VIT.MLP_DIM = 3072
_C.VIT.NUM_REGISTER_TOKENS = 0
_C.VIT.PATCHES_OVERLAP = 0.2
_C.VIT.POOLING = 'cls'
_C.VIT.CLASSIFICATION = False
_C.VIT.USE_BIAS = False

_C.TRAIN = CN()
_C.TRAIN.MAX_EPOCHS = 100
_C.TRAIN.VAL_EVERY = 10
_C.TRAIN.BASE_LR = 1.5e-3
_C.TRAIN.MIN_LR = 1.5e-7
_C.TRAIN.WEIGHT_DECAY = 0.04
_C.TRAIN.WEIGHT_DECAY_END = 0.4
_C.TRAIN.BETA1 = 0.9
_C.TRAIN.BETA2 = 0.95
_C.TRAIN.MOMENTUM = 0.9
_C.TRAIN.LOSS = 'l1'
_C.TRAIN.TEMPERATURE = 0.5
_C.TRAIN.OPTIMIZER = 'AdamW'
_C.TRAIN.SCHEDULER = 'cosine'
_C.TRAIN.PER_WARMUP = 0.05
_C.TRAIN.GRAD_CLIP = 1.0
_C.TRAIN.LOCK = False
_C.TRAIN.LORA = False
_C.TRAIN.CLASSIFIER = 'linear'
_C.TRAIN.LABEL_NAME = 'cancer'
# additions of this build: multi-label fine-tuning, one sigmoid output per name (['all'] = every label of DATA.DATASET); [] = the
# reference's one binary model per TRAIN.LABEL_NAME.  POS_WEIGHT 'balanced' weighs each label's positive term by the imbalance
# the sampler leaves (data.multilabel_pos_weight), 'none' by 1.
_C.TRAIN.LABEL_NAMES = []
_C.TRAIN.POS_WEIGHT = 'none'
# additions of this build: per-parameter multipliers on the fused optimizers (headct_foundation_amd/param_scales.py).  LAYER_DECAY
# (main_downstream.py): block i of L trains at lr * LAYER_DECAY^(L - i), the embeddings at lr * LAYER_DECAY^(L + 1); 1.0 = off.
# WD_EXCLUDE_1D: no weight decay on biases, norm scales, cls_token, register_tokens, the position table and weight_g.  Both off =
# the reference's single param group.
_C.TRAIN.LAYER_DECAY = 1.0
_C.TRAIN.WD_EXCLUDE_1D = False
# additions of this build: mixup, CutMix and label smoothing of the fine-tuning recipe (headct_foundation_amd/mixup.py, timm's Mixup).
# MIXUP / CUTMIX are the Beta alphas (0 = off); with both on, CutMix is taken with probability MIX_SWITCH_PROB; a batch (MIX_MODE
# 'batch') or a sample ('elem') is mixed with probability MIX_PROB.  LABEL_SMOOTHING in [0, 1) is for the softmax mode only.  All
# off = the reference's plain batches and nn.CrossEntropyLoss.
_C.TRAIN.MIXUP = 0.0
_C.TRAIN.CUTMIX = 0.0
_C.TRAIN.MIX_PROB = 1.0
_C.TRAIN.MIX_SWITCH_PROB = 0.5
_C.TRAIN.MIX_MODE = 'batch'
_C.TRAIN.LABEL_SMOOTHING = 0.0
# addition of this build: random 3-D affine augmentation of the training batches (headct_foundation_amd/data.py RandAffine3D; MONAI's
# RandAffine, which the reference's vit_transforms leaves out), resampled in the loader's one launch.  A sample is transformed with
# probability AFFINE_PROB (0 = off: the loader of a build without it): rotation about each axis ~ U(-r, r) degrees (AFFINE_ROTATE: three
# angles, or one for all), zoom ~ U(1 - s, 1 + s) (AFFINE_SCALE = s; one factor, or one per axis with AFFINE_ISOTROPIC False),
# translation ~ U(-f, f) * S voxels per axis (AFFINE_TRANSLATE = f, a fraction of the volume's side).  Validation and test are not touched.
_C.TRAIN.AFFINE_PROB = 0.0
_C.TRAIN.AFFINE_ROTATE = [10.0, 10.0, 10.0]
_C.TRAIN.AFFINE_SCALE = 0.1
_C.TRAIN.AFFINE_TRANSLATE = 0.05
_C.TRAIN.AFFINE_ISOTROPIC = True

# addition of this build: segmentation fine-tuning (main_segmentation.py; headct_foundation_amd/segmentation.py).  A linear voxel decoder
# on the backbone's patch tokens trained on CE_WEIGHT * cross-entropy + DICE_WEIGHT * Dice over the voxels of uint8 label volumes with
# values 0 .. NUM_CLASSES - 1; IGNORE_INDEX (fixed at 255) marks voxels that count nowhere.  CLASS_WEIGHT: one cross-entropy weight per
# class ([] = none).  SAVE_PREDS: the test pass writes the arg-max volumes as NIfTI files.  No other entry point reads this node.
_C.SEG = CN()
_C.SEG.NUM_CLASSES = 2
_C.SEG.CE_WEIGHT = 1.0
_C.SEG.DICE_WEIGHT = 1.0
_C.SEG.CLASS_WEIGHT = []
_C.SEG.IGNORE_INDEX = 255
_C.SEG.SAVE_PREDS = False
# test pass on each scan's own file grid (headct_foundation_amd/native.py): <name>_native.nii.gz with the image's affine, volumes in
# mL (native_volumes.csv) and Dice / IoU against the mask file itself.  Needs real data (DATA.SYNTHETIC has no file grid).
_C.SEG.NATIVE_PREDS = False
_C.SEG.NATIVE_INTERP = 'linear'  # 'linear' (trilinear blend of the logits) | 'nearest'
# boundary metrics in millimetres on the file grid (headct_foundation_amd/surface.py): HD, HD95, ASSD and the surface Dice NSD at
# SURFACE_TOLERANCE_MM per scan (native_surface.csv) and as means over the scans.  Needs NATIVE_PREDS.
_C.SEG.SURFACE_METRICS = False
_C.SEG.SURFACE_TOLERANCE_MM = 2.0
# lesions on the file grid (headct_foundation_amd/components.py), at COMPONENT_CONNECTIVITY (6 | 18 | 26).  MIN_COMPONENT_ML > 0:
# predicted components below that volume become background before anything is written or scored.  LESION_METRICS: lesion-wise
# detection counts per scan (native_lesion_counts.csv, native_lesions.csv) and NativeLesionRecall / Precision / F1.  Need NATIVE_PREDS.
_C.SEG.MIN_COMPONENT_ML = 0.0
_C.SEG.LESION_METRICS = False
_C.SEG.COMPONENT_CONNECTIVITY = 26
# random 3-D affine of the training batches, scans and masks alike (headct_foundation_amd/data.py augment_segmentation_batch): a sample is
# transformed with probability AFFINE_PROB (0 = off: the loader of a build without it), the scan trilinear, the mask nearest neighbour
# through the same matrix; the magnitudes are TRAIN.AFFINE_ROTATE / AFFINE_SCALE / AFFINE_TRANSLATE / AFFINE_ISOTROPIC.  AFFINE_OUTSIDE is
# the label where the scan is zero-padded: 'background' (class 0, MONAI's zeros padding) | 'ignore' (255: counts nowhere).  Validation and
# test are not touched.  TRAIN.AFFINE_PROB itself stays refused in this mode.
_C.SEG.AFFINE_PROB = 0.0
_C.SEG.AFFINE_OUTSIDE = 'background'

_C.LOG = CN()
_C.LOG.OUTPUT_DIR = '<path-to>/headCT_foundation/log'
_C.LOG.FILENAME = 'headCT_foundation'

_C.WANDB = CN()
_C.WANDB.WANDB_ENABLE = False
_C.WANDB.PROJECT = 'headCT_foundation'

_C.SEED = 42
_C.AMP_ENABLE = False
_C.LOCAL_RANK = 0
_C.OUTPUT = ''
_C.TAG = 'default'
_C.PREDS_SAVE_NAME = 'None'


def _update_config_from_file(config, cfg_file):
    """yaml merge with `BASE:` inheritance (config.py:163-180)."""
    config.defrost()
    with open(cfg_file, 'r') as f:
        yaml_cfg = yaml.safe_load(f) or {}
    for cfg in yaml_cfg.setdefault('BASE', ['']):
        if cfg:
            _update_config_from_file(config, os.path.join(os.path.dirname(cfg_file), cfg))
    print(f'=> merge config from {cfg_file}')
    config.merge_from_file(cfg_file)
    config.freeze()


_ARG_TO_KEY = [  # CLI flag -> config key (config.py:199-251)
    ('preds_save_name', 'PREDS_SAVE_NAME'), ('dataset', 'DATA.DATASET'), ('batch_size', 'DATA.BATCH_SIZE'),
    ('few_shots', 'DATA.FEW_SHOTS'), ('num_workers', 'DATA.NUM_WORKERS'), ('train_csv_path', 'DATA.TRAIN_CSV_PATH'),
    ('val_csv_path', 'DATA.VAL_CSV_PATH'), ('test_csv_path', 'DATA.TEST_CSV_PATH'), ('optimizer', 'TRAIN.OPTIMIZER'),
    ('scheduler', 'TRAIN.SCHEDULER'), ('max_epochs', 'TRAIN.MAX_EPOCHS'), ('grad_clip', 'TRAIN.GRAD_CLIP'),
    ('base_lr', 'TRAIN.BASE_LR'), ('min_lr', 'TRAIN.MIN_LR'), ('weight_decay', 'TRAIN.WEIGHT_DECAY'), ('lock', 'TRAIN.LOCK'),
    ('pooling', 'VIT.POOLING'), ('seed', 'SEED'), ('use_amp', 'AMP_ENABLE'), ('use_wandb', 'WANDB.WANDB_ENABLE'),
    ('wandb_project', 'WANDB.PROJECT'), ('model_name', 'MODEL.NAME'), ('model_load_path', 'MODEL.PRETRAINED'),
    ('label_name', 'TRAIN.LABEL_NAME'), ('label_names', 'TRAIN.LABEL_NAMES'), ('pos_weight', 'TRAIN.POS_WEIGHT'), ('classifier', 'TRAIN.CLASSIFIER'), ('filename', 'LOG.FILENAME'),
    ('wd_exclude_1d', 'TRAIN.WD_EXCLUDE_1D'),
]


def _check_mix_keys(t):
    num = lambda v: isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v)
    for key in ('MIXUP', 'CUTMIX'):
        if not (num(t[key]) and t[key] >= 0.0):
            raise ValueError(f"TRAIN.{key} (a Beta alpha, 0 = off) must be >= 0: got {t[key]}")
    for key in ('MIX_PROB', 'MIX_SWITCH_PROB'):
        if not (num(t[key]) and 0.0 <= t[key] <= 1.0):
            raise ValueError(f"TRAIN.{key} must lie in [0, 1]: got {t[key]}")
    if not (num(t.LABEL_SMOOTHING) and 0.0 <= t.LABEL_SMOOTHING < 1.0):
        raise ValueError(f"TRAIN.LABEL_SMOOTHING must lie in [0, 1): got {t.LABEL_SMOOTHING}")
    if t.MIX_MODE not in ('batch', 'elem'):
        raise ValueError(f"TRAIN.MIX_MODE must be 'batch' or 'elem': got {t.MIX_MODE!r}")


def _check_affine_keys(t):
    num = lambda v: isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v)
    if not (num(t.AFFINE_PROB) and 0.0 <= t.AFFINE_PROB <= 1.0):
        raise ValueError(f"TRAIN.AFFINE_PROB must lie in [0, 1]: got {t.AFFINE_PROB}")
    rot = list(t.AFFINE_ROTATE) if isinstance(t.AFFINE_ROTATE, (list, tuple)) else [t.AFFINE_ROTATE]
    if len(rot) not in (1, 3) or not all(num(r) and 0.0 <= r <= 180.0 for r in rot):
        raise ValueError(f"TRAIN.AFFINE_ROTATE must be one or three angles in [0, 180] degrees: got {t.AFFINE_ROTATE}")
    if not (num(t.AFFINE_SCALE) and 0.0 <= t.AFFINE_SCALE < 1.0):
        raise ValueError(f"TRAIN.AFFINE_SCALE must lie in [0, 1): got {t.AFFINE_SCALE}")
    if not (num(t.AFFINE_TRANSLATE) and 0.0 <= t.AFFINE_TRANSLATE < 1.0):
        raise ValueError(f"TRAIN.AFFINE_TRANSLATE (a fraction of the volume's side) must lie in [0, 1): got {t.AFFINE_TRANSLATE}")
    if not isinstance(t.AFFINE_ISOTROPIC, bool):
        raise ValueError(f"TRAIN.AFFINE_ISOTROPIC must be True or False: got {t.AFFINE_ISOTROPIC!r}")


def _check_dino_keys(d):
    if d.CENTERING not in ('centering', 'sinkhorn_knopp'):
        raise ValueError(f"DINO.CENTERING must be 'centering' or 'sinkhorn_knopp': got {d.CENTERING!r}")
    if not (isinstance(d.SK_ITERS, int) and not isinstance(d.SK_ITERS, bool) and d.SK_ITERS >= 1):
        raise ValueError(f"DINO.SK_ITERS must be an integer >= 1: got {d.SK_ITERS!r}")
    w = d.KOLEO_WEIGHT
    if not (isinstance(w, (int, float)) and not isinstance(w, bool) and math.isfinite(w) and w >= 0.0):
        raise ValueError(f"DINO.KOLEO_WEIGHT must be >= 0 (0 = off): got {w!r}")
    num = lambda v: isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v)
    if not (num(d.IBOT_WEIGHT) and d.IBOT_WEIGHT >= 0.0):
        raise ValueError(f"DINO.IBOT_WEIGHT must be >= 0 (0 = off): got {d.IBOT_WEIGHT!r}")
    r = d.IBOT_MASK_RATIO
    if not (isinstance(r, (list, tuple)) and len(r) == 2 and all(num(v) for v in r) and 0.0 < r[0] <= r[1] <= 1.0):
        raise ValueError(f"DINO.IBOT_MASK_RATIO must be [lo, hi] with 0 < lo <= hi <= 1: got {r!r}")
    if not (num(d.IBOT_MASK_PROB) and 0.0 < d.IBOT_MASK_PROB <= 1.0):
        raise ValueError(f"DINO.IBOT_MASK_PROB (the share of global crops that are masked) must lie in (0, 1]: got {d.IBOT_MASK_PROB!r}")
    if d.IBOT_WEIGHT > 0.0 and d.USE_BN:
        raise ValueError("DINO.IBOT_WEIGHT > 0 with DINO.USE_BN True: one head serves class and patch rows, and its batch statistics would mix them")


SEG_MAX_CLASSES = 16  # the class counts the segmentation kernels are compiled for


def _check_seg_keys(g):
    num = lambda v: isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v)
    k = g.NUM_CLASSES
    if not (isinstance(k, int) and not isinstance(k, bool) and 2 <= k <= SEG_MAX_CLASSES):
        raise ValueError(f"SEG.NUM_CLASSES must be an integer in [2, {SEG_MAX_CLASSES}]: got {k!r}")
    for key in ('CE_WEIGHT', 'DICE_WEIGHT'):
        if not (num(g[key]) and g[key] >= 0.0):
            raise ValueError(f"SEG.{key} must be >= 0: got {g[key]!r}")
    if g.CE_WEIGHT == 0.0 and g.DICE_WEIGHT == 0.0:
        raise ValueError("SEG.CE_WEIGHT and SEG.DICE_WEIGHT are both 0: nothing to train on")
    cw = g.CLASS_WEIGHT
    if not (isinstance(cw, (list, tuple)) and len(cw) in (0, k) and all(num(v) and v >= 0.0 for v in cw) and (not cw or sum(cw) > 0)):
        raise ValueError(f"SEG.CLASS_WEIGHT must be [] or {k} weights >= 0 that are not all 0: got {cw!r}")
    if g.IGNORE_INDEX != 255:
        raise ValueError(f"SEG.IGNORE_INDEX is fixed at 255 (the label volumes are uint8): got {g.IGNORE_INDEX!r}")
    if not isinstance(g.SAVE_PREDS, bool):
        raise ValueError(f"SEG.SAVE_PREDS must be True or False: got {g.SAVE_PREDS!r}")
    if not isinstance(g.NATIVE_PREDS, bool):
        raise ValueError(f"SEG.NATIVE_PREDS must be True or False: got {g.NATIVE_PREDS!r}")
    if g.NATIVE_INTERP not in ('linear', 'nearest'):
        raise ValueError(f"SEG.NATIVE_INTERP must be 'linear' or 'nearest': got {g.NATIVE_INTERP!r}")
    if not isinstance(g.SURFACE_METRICS, bool):
        raise ValueError(f"SEG.SURFACE_METRICS must be True or False: got {g.SURFACE_METRICS!r}")
    if g.SURFACE_METRICS and not g.NATIVE_PREDS:
        raise ValueError("SEG.SURFACE_METRICS without SEG.NATIVE_PREDS: the boundary metrics are measured on the scan's own grid")
    if not (num(g.SURFACE_TOLERANCE_MM) and g.SURFACE_TOLERANCE_MM >= 0.0):
        raise ValueError(f"SEG.SURFACE_TOLERANCE_MM must be finite and >= 0: got {g.SURFACE_TOLERANCE_MM!r}")
    if not (num(g.MIN_COMPONENT_ML) and g.MIN_COMPONENT_ML >= 0.0):
        raise ValueError(f"SEG.MIN_COMPONENT_ML must be finite and >= 0: got {g.MIN_COMPONENT_ML!r}")
    if not isinstance(g.LESION_METRICS, bool):
        raise ValueError(f"SEG.LESION_METRICS must be True or False: got {g.LESION_METRICS!r}")
    if isinstance(g.COMPONENT_CONNECTIVITY, bool) or g.COMPONENT_CONNECTIVITY not in (6, 18, 26):
        raise ValueError(f"SEG.COMPONENT_CONNECTIVITY must be one of 6, 18, 26: got {g.COMPONENT_CONNECTIVITY!r}")
    if (g.MIN_COMPONENT_ML > 0.0 or g.LESION_METRICS) and not g.NATIVE_PREDS:
        raise ValueError("SEG.MIN_COMPONENT_ML / SEG.LESION_METRICS without SEG.NATIVE_PREDS: millilitres and lesions exist only on the scan's own grid")
    if not (num(g.AFFINE_PROB) and 0.0 <= g.AFFINE_PROB <= 1.0):
        raise ValueError(f"SEG.AFFINE_PROB must lie in [0, 1]: got {g.AFFINE_PROB!r}")
    if g.AFFINE_OUTSIDE not in ('background', 'ignore'):
        raise ValueError(f"SEG.AFFINE_OUTSIDE must be 'background' or 'ignore': got {g.AFFINE_OUTSIDE!r}")


def check_segmentation_mode(config):
    """What main_segmentation.py refuses: recipes that would have to move, mix or drop label voxels (follow-ups).  Drop path, dropout,
    LoRA, layer decay, TRAIN.WD_EXCLUDE_1D, RMSNorm, register tokens and TRAIN.LOCK live in the backbone or the optimizer and pass."""
    t = config.TRAIN
    if t.AFFINE_PROB > 0:
        raise ValueError(f"TRAIN.AFFINE_PROB {t.AFFINE_PROB} in segmentation mode: the switch of this mode is SEG.AFFINE_PROB (--seg_affine_prob), "
                         "which resamples the masks with the scans")
    if t.MIXUP > 0 or t.CUTMIX > 0:
        raise ValueError(f"TRAIN.MIXUP {t.MIXUP} / TRAIN.CUTMIX {t.CUTMIX} in segmentation mode: the label volumes would need mixing (not implemented)")
    if config.VIT.PATCH_DROPOUT > 0:
        raise ValueError(f"VIT.PATCH_DROPOUT {config.VIT.PATCH_DROPOUT} in segmentation mode: the decoder needs every patch token")
    if config.VIT.INPUT_SIZE % config.VIT.PATCH_SIZE:
        raise ValueError(f"VIT.INPUT_SIZE {config.VIT.INPUT_SIZE} is no multiple of VIT.PATCH_SIZE {config.VIT.PATCH_SIZE}")
    if config.SEG.NATIVE_PREDS and config.DATA.SYNTHETIC:
        raise ValueError("SEG.NATIVE_PREDS with DATA.SYNTHETIC True: synthetic volumes have no file grid to carry the prediction back to")


def update_config(config, args):
    _update_config_from_file(config, args.cfg)
    config.defrost()
    if getattr(args, 'opts', None):
        config.merge_from_list(args.opts)
    for flag, key in _ARG_TO_KEY:
        val = getattr(args, flag, None)
        if val:  # same truthiness rule as the reference's _check_args (config.py:196-197)
            node = config
            parts = key.split('.')
            for p in parts[:-1]:
                node = node[p]
            node[parts[-1]] = val
    if getattr(args, 'layer_decay', None) is not None:  # not through the truthiness rule: --layer_decay 0 must be refused, not dropped
        config.TRAIN.LAYER_DECAY = float(args.layer_decay)
    if getattr(args, 'drop_path', None) is not None:  # not through the truthiness rule: --drop_path 0 reaches the config
        config.VIT.DROP_PATH_RATE = float(args.drop_path)
    if getattr(args, 'patch_dropout', None) is not None:  # as --drop_path: 0 reaches the config
        config.VIT.PATCH_DROPOUT = float(args.patch_dropout)
    for flag, key in (('mixup', 'MIXUP'), ('cutmix', 'CUTMIX'), ('smoothing', 'LABEL_SMOOTHING')):  # as --drop_path: 0 reaches the config
        if getattr(args, flag, None) is not None:
            config.TRAIN[key] = float(getattr(args, flag))
    for flag, key in (('affine_prob', 'AFFINE_PROB'), ('affine_scale', 'AFFINE_SCALE'), ('affine_translate', 'AFFINE_TRANSLATE')):  # 0 reaches the config
        if getattr(args, flag, None) is not None:
            config.TRAIN[key] = float(getattr(args, flag))
    if getattr(args, 'affine_rotate', None) is not None:
        rot = args.affine_rotate if isinstance(args.affine_rotate, (list, tuple)) else [args.affine_rotate]
        config.TRAIN.AFFINE_ROTATE = [float(r) for r in rot]
    if getattr(args, 'centering', None) is not None:
        config.DINO.CENTERING = str(args.centering)
    if getattr(args, 'koleo_weight', None) is not None:  # as --drop_path: 0 reaches the config
        config.DINO.KOLEO_WEIGHT = float(args.koleo_weight)
    if getattr(args, 'ibot_weight', None) is not None:  # as --drop_path: 0 reaches the config
        config.DINO.IBOT_WEIGHT = float(args.ibot_weight)
    if getattr(args, 'ibot_mask_ratio', None) is not None:
        config.DINO.IBOT_MASK_RATIO = [float(v) for v in args.ibot_mask_ratio]
    if getattr(args, 'ibot_mask_prob', None) is not None:
        config.DINO.IBOT_MASK_PROB = float(args.ibot_mask_prob)
    if getattr(args, 'seg_classes', None) is not None:
        config.SEG.NUM_CLASSES = int(args.seg_classes)
    for flag, key in (('dice_weight', 'DICE_WEIGHT'), ('ce_weight', 'CE_WEIGHT')):  # as --drop_path: 0 reaches the config
        if getattr(args, flag, None) is not None:
            config.SEG[key] = float(getattr(args, flag))
    if getattr(args, 'save_preds', None):
        config.SEG.SAVE_PREDS = True
    if getattr(args, 'native_preds', None):
        config.SEG.NATIVE_PREDS = True
    if getattr(args, 'native_interp', None) is not None:
        config.SEG.NATIVE_INTERP = str(args.native_interp)
    if getattr(args, 'surface_metrics', None):
        config.SEG.SURFACE_METRICS = True
    if getattr(args, 'surface_tolerance_mm', None) is not None:
        config.SEG.SURFACE_TOLERANCE_MM = float(args.surface_tolerance_mm)
    if getattr(args, 'min_component_ml', None) is not None:  # as --drop_path: 0 reaches the config
        config.SEG.MIN_COMPONENT_ML = float(args.min_component_ml)
    if getattr(args, 'lesion_metrics', None):
        config.SEG.LESION_METRICS = True
    if getattr(args, 'component_connectivity', None) is not None:
        config.SEG.COMPONENT_CONNECTIVITY = int(args.component_connectivity)
    if getattr(args, 'seg_affine_prob', None) is not None:  # as --drop_path: 0 reaches the config
        config.SEG.AFFINE_PROB = float(args.seg_affine_prob)
    if getattr(args, 'seg_affine_outside', None) is not None:
        config.SEG.AFFINE_OUTSIDE = str(args.seg_affine_outside)
    _check_seg_keys(config.SEG)
    _check_dino_keys(config.DINO)
    ld = config.TRAIN.LAYER_DECAY
    if not (isinstance(ld, (int, float)) and math.isfinite(ld) and 0.0 < ld <= 1.0):
        raise ValueError(f"TRAIN.LAYER_DECAY must lie in (0, 1]: got {ld}")
    pdrop = config.VIT.PATCH_DROPOUT
    if not (isinstance(pdrop, (int, float)) and not isinstance(pdrop, bool) and math.isfinite(pdrop) and 0.0 <= pdrop < 1.0):
        raise ValueError(f"VIT.PATCH_DROPOUT (the share of patch tokens dropped in training) must lie in [0, 1): got {pdrop}")
    _check_mix_keys(config.TRAIN)
    _check_affine_keys(config.TRAIN)
    config.LOCAL_RANK = args.local_rank
    config.OUTPUT = os.path.join(config.OUTPUT)
    config.freeze()


def get_config(args):
    """Clone of the defaults, updated from `args.cfg`, `args.opts` and the named CLI flags (config.py:261-273)."""
    config = _C.clone()
    update_config(config, args)
    return config
