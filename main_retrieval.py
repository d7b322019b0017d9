"""Volume-to-volume retrieval, k-NN evaluation and attention maps with a pre-trained encoder on the HIP path (the reference's README:
feature extraction, retrieval mAP on RSNA / CQ500, attention-map visualisation; its code stops at notebooks/extract_feature_sample.ipynb).

  python main_retrieval.py --model_name vit --cfg CFG.yaml --model_load_path PRETRAINED.pt --save_dir OUT \
      [--pooling cls|mean|cls_mean] [--topk 1 5 10] [--bank_dtype bf16|fp32] [--attention_maps N]

Single process.  The forward-only `ViT` of VIT.* (MAE.NORM_LAYER, MAE.COMPUTE_DTYPE) loads MODEL.PRETRAINED; gallery = the scans of
DATA.TRAIN_CSV_PATH (or --gallery_csv_path), queries = DATA.TEST_CSV_PATH (or --query_csv_path), through the labelled loaders of
main_downstream.py, or synthetic labelled volumes with different seeds (DATA.SYNTHETIC).  Features are pooled (VIT.POOLING), the
gallery becomes a `FeatureBank`, and every query is searched with the fused similarity + top-k kernel.  Logged and written to
--save_dir: P@k and mAP@k (headct_foundation_amd.retrieval.retrieval_metrics), weighted k-NN accuracy and AUROC, the features, labels,
names and neighbour table, and with --attention_maps N the class token's attention maps of the first N query scans.
"""
import argparse
import json
import os
import random

import numpy as np
import torch
import torch.nn as nn

from config import get_config
from headct_foundation_amd.data import SyntheticLabelled, get_finetune_dataloaders
from headct_foundation_amd.layers import RMSNorm
from headct_foundation_amd.metrics import multiclass_accuracy, multiclass_auroc
from headct_foundation_amd.misc import load_model
from headct_foundation_amd.retrieval import FeatureBank, extract_features, knn_predict, retrieval_metrics
from headct_foundation_amd.vit import ViT
from logger import create_logger


def parse_option():
    parser = argparse.ArgumentParser('HIP retrieval / k-NN evaluation / attention map script', add_help=False)
    parser.add_argument('--cfg', type=str, required=True, metavar="FILE", help='path to config file')
    parser.add_argument("--opts", help="Modify config options using the command-line", default=None, nargs='+')
    parser.add_argument("--local_rank", type=int, default=0, help='parsed for symmetry with the training scripts; single process')
    parser.add_argument("--seed", type=int, help='seed')
    parser.add_argument("--filename", type=str, default="retrieval")
    # model parameters
    parser.add_argument("--model_name", type=str, help='model name')
    parser.add_argument("--model_load_path", type=str, help='path to trained model')
    parser.add_argument("--pooling", type=str, choices=['cls', 'mean', 'cls_mean'], help='token pooling of the features (VIT.POOLING)')
    parser.add_argument("--label_name", type=str, help='label name of the relevance / k-NN classes')
    parser.add_argument("--batch_size", type=int, help='batch size')
    parser.add_argument("--num_workers", type=int, help='number of workers for dataloader')
    # dataset parameters
    parser.add_argument('--dataset', type=str, help='dataset name')
    parser.add_argument('--gallery_csv_path', type=str, help='csv of the gallery scans (default DATA.TRAIN_CSV_PATH)')
    parser.add_argument('--query_csv_path', type=str, help='csv of the query scans (default DATA.TEST_CSV_PATH)')
    # retrieval parameters
    parser.add_argument('--topk', type=int, nargs='+', default=[1, 5, 10], help='the k of P@k / mAP@k; the largest is the k-NN k')
    parser.add_argument('--bank_dtype', type=str, default='bf16', choices=['bf16', 'fp32'], help='storage of the normalised features')
    parser.add_argument('--knn_temperature', type=float, default=0.07, help='T of the weighted k-NN votes exp(score / T)')
    parser.add_argument('--attention_maps', type=int, default=0, help='write attention maps of the first N query scans')
    parser.add_argument('--save_dir', type=str, default='retrieval_out', help='directory of the output files')
    args, _ = parser.parse_known_args()
    # the loaders read DATA.TRAIN / TEST_CSV_PATH: the gallery and query flags land there
    args.train_csv_path, args.test_csv_path = args.gallery_csv_path, args.query_csv_path
    return args, get_config(args)


def build_model(config, device):
    v = config.VIT
    if config.MAE.NORM_LAYER == 'layernorm':
        norm_layer = nn.LayerNorm
    elif config.MAE.NORM_LAYER == 'rmsnorm':
        norm_layer = RMSNorm
    else:
        raise ValueError(f"Normalization layer {config.MAE.NORM_LAYER} not supported")
    model = ViT(in_chans=v.IN_CHANS, img_size=v.INPUT_SIZE, patch_size=v.PATCH_SIZE, hidden_size=v.HIDDEN_SIZE, mlp_dim=v.MLP_DIM,
                num_layers=v.NUM_LAYERS, num_heads=v.NUM_HEADS, patch_embed=v.PATCH_EMBED, pos_embed=v.POS_EMBED, classification=False,
                dropout_rate=v.DROPOUT_RATE, spatial_dims=v.SPATIAL_DIMS, num_register_tokens=v.NUM_REGISTER_TOKENS, qkv_bias=v.USE_BIAS,
                lora=config.TRAIN.LORA, norm_layer=norm_layer, compute_dtype=config.MAE.COMPUTE_DTYPE, drop_path_rate=0.0)
    return model.to(device).eval()


def main(config, args, logger):
    if config.MODEL.NAME != "vit":
        raise ValueError(f"Backbone {config.MODEL.NAME} not supported")
    if not torch.cuda.is_available():
        raise SystemExit("main_retrieval.py (HIP) needs an MI355X: the path has no CPU fallback")
    ks = sorted(set(args.topk))
    if ks[0] < 1 or ks[-1] > 64:
        raise ValueError(f"--topk {args.topk}: every k must be in [1, 64]")
    device = torch.device("cuda", torch.cuda.current_device())
    bs, v = config.DATA.BATCH_SIZE, config.VIT
    if config.DATA.SYNTHETIC:
        nb = max(1, config.DATA.SYNTHETIC_SAMPLES // bs)
        mk = lambda k, salt: SyntheticLabelled(k, bs, v.IN_CHANS, v.INPUT_SIZE, config.DATA.NUM_CLASSES, device, config.SEED + salt)
        gallery_loader, query_loader = mk(nb, 0), mk(max(1, nb // 4), 2000)
    else:  # every scan once, in file order: the validation-style loaders over the two csv files
        _, gallery_loader, query_loader = _eval_loaders(config, device)

    model = build_model(config, device)
    load_model(config, model, None, logger)
    pooling = config.VIT.POOLING
    g_feats, g_labels, g_names = extract_features(model, gallery_loader, pooling)
    q_feats, q_labels, q_names = extract_features(model, query_loader, pooling)
    logger.info(f"Gallery: {tuple(g_feats.shape)}, queries: {tuple(q_feats.shape)}, pooling: {pooling}, bank: {args.bank_dtype}")

    bank = FeatureBank(g_feats, g_labels, g_names, dtype=args.bank_dtype)
    scores, idx = bank.search(q_feats, ks[-1])
    metrics = retrieval_metrics(idx, q_labels, g_labels, ks)
    ncls = config.DATA.NUM_CLASSES
    probs = knn_predict(scores, idx, g_labels, ncls, T=args.knn_temperature)
    metrics["kNN_accuracy"] = [float(a) for a in multiclass_accuracy(probs, q_labels, ncls)]
    metrics["kNN_AUROC"] = [float(a) for a in multiclass_auroc(probs, q_labels, ncls)]
    metrics.update(k_nn=ks[-1], pooling=pooling, bank_dtype=args.bank_dtype, n_gallery=len(g_names), n_query=len(q_names))
    for k in ks:
        logger.info(f"P@{k}: {metrics[f'P@{k}']:.4f}  mAP@{k}: {metrics[f'mAP@{k}']:.4f}")
    logger.info(f"k-NN (k = {ks[-1]}) MulticlassAccuracy: {metrics['kNN_accuracy']}  MulticlassAUROC: {metrics['kNN_AUROC']}")

    os.makedirs(args.save_dir, exist_ok=True)
    out = lambda name: os.path.join(args.save_dir, name)
    np.save(out("gallery_features.npy"), g_feats.cpu().numpy())
    np.save(out("query_features.npy"), q_feats.cpu().numpy())
    np.save(out("gallery_labels.npy"), g_labels.cpu().numpy())
    np.save(out("query_labels.npy"), q_labels.cpu().numpy())
    np.save(out("neighbours.npy"), idx.cpu().numpy())
    for name, names in (("gallery_names.json", g_names), ("query_names.json", q_names)):
        with open(out(name), "w") as f:
            json.dump(names, f)
    with open(out("retrieval.json"), "w") as f:
        json.dump(metrics, f, indent=1)

    done = 0
    for data, _, _ in query_loader:  # attention_{i}.npy: [H, S, S, S] fp16, the class token's map of the last block, trilinear
        if done >= args.attention_maps:
            break
        maps = model.attention_map(data.to(device), block=-1, upsample="trilinear")
        for m in maps[:args.attention_maps - done]:
            np.save(out(f"attention_{done}.npy"), m.to(torch.float16).cpu().numpy())
            done += 1
    logger.info(f"retrieval completed: files under {args.save_dir}")
    return metrics


def _eval_loaders(config, device):
    """(train, gallery, query) loaders over DATA.TRAIN / TEST_CSV_PATH that visit every scan once without augmentation: the
    validation pipeline of get_finetune_dataloaders applied to both files (the gallery file is passed as the validation csv)."""
    config.defrost()
    config.DATA.VAL_CSV_PATH = config.DATA.TRAIN_CSV_PATH
    config.freeze()
    train_loader, val_loader, test_loader, _ = get_finetune_dataloaders(config, device, 0, 1)
    return train_loader, val_loader, test_loader


if __name__ == "__main__":
    args, config = parse_option()
    seed = config.SEED
    random.seed(seed); np.random.seed(seed); torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)
    logger = create_logger(output_dir=config.LOG.OUTPUT_DIR, dist_rank=0, name=config.LOG.FILENAME)
    logger.info(config.dump())
    logger.info(json.dumps(vars(args)))
    main(config, args, logger)
