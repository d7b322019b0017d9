"""headct_foundation_amd: MI355X-native (gfx950) MAE pre-training hot path behind the reference's interface."""
from .mae import MaskedAutoencoderViT, build_sincos_position_embedding  # noqa: F401
from ._lib import HctError  # noqa: F401
from .pos_embed import interpolate_pos_embed  # noqa: F401
from .vit import ViT  # noqa: F401
from .layers import RMSNorm  # noqa: F401
from .classifier import AttentionClassifier, LinearClassifier, bce_with_logits, cross_entropy, soft_cross_entropy  # noqa: F401
from .mixup import MixedCriterion, Mixup, mix_multilabel_targets, mix_volumes, rand_box3d  # noqa: F401
from .optim import HipAdamW, HipLamb, HipLion, HipSGD, clip_grad_norm_  # noqa: F401
from .param_scales import layer_decay_scales, no_decay_scales, vit_layer_id  # noqa: F401
from .data import (DevicePool, LabelledVolumes, PretrainVolumes, RandAffine3D, VolumeCache, affine_augment, affine_matrices,  # noqa: F401
                   gather_augment, load_volume)
from .nifti import read_nifti, write_nifti  # noqa: F401
from .retrieval import FeatureBank, extract_features, knn_predict, pool_tokens, retrieval_metrics  # noqa: F401
from .reconstruct import Reconstruction, anomaly_score, cover_passes  # noqa: F401
from .segmentation import SegmentationHead, affine_labels, gather_flip_labels, seg_loss, seg_predict  # noqa: F401
