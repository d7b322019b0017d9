"""Reconstructions and anomaly (error) maps of head CT scans with a pre-trained masked autoencoder on the HIP path (the reference has
`unpatchify` and an unread MAE.RETURN_IMAGE and stops there).

  python main_reconstruct.py --model_name mae --cfg CFG.yaml --model_load_path MAE.pt --save_dir OUT \
      [--passes N] [--max_scans N] [--label_name NAME] [--nifti]

Single process.  The `MaskedAutoencoderViT` of MAE.* loads MODEL.PRETRAINED; the scans are those of DATA.TEST_CSV_PATH (or
--test_csv_path) through the pre-training loaders, or with --label_name through the labelled evaluation loaders of
main_downstream.py, or synthetic volumes (DATA.SYNTHETIC).  Every batch goes through `model.reconstruct`: a covering schedule of masks
(--passes, default the fewest that mask every patch once), the de-normalised predictions averaged per voxel, the per-patch loss
term averaged into an error map.  Written to --save_dir: scores.csv (name, mean and max patch error, the loss of every pass),
error_maps.npy [n, g, g, g], reconstruct.json, with --label_name the AUROC of the mean score against label > 0, and with --nifti
per scan the input, the reconstruction and the error map as NIfTI volumes in MODEL space.
"""
import argparse
import csv
import json
import os
import random

import numpy as np
import torch

from config import get_config
from headct_foundation_amd.data import SyntheticLabelled, SyntheticVolumes, get_finetune_dataloaders, pretrain_volume_loaders
from headct_foundation_amd.metrics import binary_auroc
from headct_foundation_amd.misc import load_model
from headct_foundation_amd.nifti import write_nifti
from headct_foundation_amd.reconstruct import anomaly_score, cover_passes
from logger import create_logger
from main_pretrain_mae import build_model


def parse_option(argv=None):
    parser = argparse.ArgumentParser('HIP MAE reconstruction / error map script', add_help=False)
    parser.add_argument('--cfg', type=str, required=True, metavar="FILE", help='path to config file')
    parser.add_argument("--opts", help="Modify config options using the command-line", default=None, nargs='+')
    parser.add_argument("--local_rank", type=int, default=0, help='parsed for symmetry with the training scripts; single process')
    parser.add_argument("--seed", type=int, help='seed (also the seed of the mask schedule)')
    parser.add_argument("--filename", type=str, default="reconstruct")
    # model parameters
    parser.add_argument("--model_name", type=str, help='model name')
    parser.add_argument("--model_load_path", type=str, help='path to trained model')
    parser.add_argument("--label_name", type=str, help='label name: read the labelled evaluation loaders and report the AUROC of the score')
    parser.add_argument("--batch_size", type=int, help='batch size')
    parser.add_argument("--num_workers", type=int, help='number of workers for dataloader')
    # dataset parameters
    parser.add_argument('--dataset', type=str, help='dataset name')
    parser.add_argument('--test_csv_path', type=str, help='csv of the scans (default DATA.TEST_CSV_PATH)')
    # reconstruction parameters
    parser.add_argument('--passes', type=int, default=None, help='masks per scan (default: the fewest that mask every patch at least once; 1 = one random mask)')
    parser.add_argument('--max_scans', type=int, default=0, help='stop after N scans (0 = all)')
    parser.add_argument('--nifti', action='store_true',
                        help='write NAME_input / NAME_recon / NAME_error .nii.gz per scan, in MODEL space: the voxel grid the model sees after the '
                             'loading chain, with an identity affine (not the geometry of the original scan)')
    parser.add_argument('--save_dir', type=str, default='reconstruct_out', help='directory of the output files')
    args, _ = parser.parse_known_args(argv)
    return args, get_config(args)


def _loader(config, args, device):
    """Batches `(volume, target or None, names)` of the scans, every scan once, in file order."""
    mae, bs = config.MAE, config.DATA.BATCH_SIZE
    labelled = bool(args.label_name)
    if config.DATA.SYNTHETIC:
        nb = max(1, config.DATA.SYNTHETIC_SAMPLES // bs)
        if labelled:
            return SyntheticLabelled(nb, bs, mae.IN_CHANS, mae.INPUT_SIZE, config.DATA.NUM_CLASSES, device, config.SEED)
        vols = SyntheticVolumes(nb, bs, mae.IN_CHANS, mae.INPUT_SIZE, device, config.SEED)
        return [(v, None, [f"synthetic_{i}_{b}" for b in range(bs)]) for i, v in enumerate(vols)]
    config.defrost()  # the loaders open all three csv files: the scans' file stands in for the two this script does not read
    for key in ("TRAIN_CSV_PATH", "VAL_CSV_PATH"):
        if not os.path.isfile(str(getattr(config.DATA, key))):
            setattr(config.DATA, key, config.DATA.TEST_CSV_PATH)
    config.VIT.INPUT_SIZE, config.VIT.IN_CHANS = mae.INPUT_SIZE, mae.IN_CHANS  # (the labelled loaders check the cache item against VIT.*)
    config.freeze()
    if labelled:
        return get_finetune_dataloaders(config, device, 0, 1)[2]
    test = pretrain_volume_loaders(config, device, 0, 1, mae.INPUT_SIZE, mae.IN_CHANS)[2]
    names = [test.paths[i] for i in test.indices]

    def batches():
        at = 0
        for v in test:
            yield v, None, names[at:at + v.shape[0]]
            at += v.shape[0]
    return batches()


def _stem(name, taken):
    """File stem of a scan name, unique within the run."""
    base = os.path.basename(str(name))
    for ext in (".nii.gz", ".nii"):
        if base.endswith(ext):
            base = base[:-len(ext)]
    base = base or "scan"
    stem, k = base, 1
    while stem in taken:
        stem, k = f"{base}_{k}", k + 1
    taken.add(stem)
    return stem


def main(config, args, logger):
    if config.MODEL.NAME != "mae":
        raise ValueError(f"Model {config.MODEL.NAME} not supported")
    if not torch.cuda.is_available():
        raise SystemExit("main_reconstruct.py (HIP) needs an MI355X: the path has no CPU fallback")
    device = torch.device("cuda", torch.cuda.current_device())
    model = build_model(config, device).eval()
    load_model(config, model, None, logger)
    L, K = model.num_patches, model.len_keep
    need = cover_passes(L, K)
    n_pass = need if args.passes is None else args.passes
    logger.info(f"{L} patches, {L - K} masked per pass: {n_pass} passes per scan (cover_passes = {need})")

    os.makedirs(args.save_dir, exist_ok=True)
    out = lambda name: os.path.join(args.save_dir, name)
    rows, maps, labels, taken, done = [], [], [], set(), 0
    for data, target, names in _loader(config, args, device):
        if args.max_scans and done >= args.max_scans:
            break
        take = data.shape[0] if not args.max_scans else min(data.shape[0], args.max_scans - done)
        data = data.to(device)
        rec = model.reconstruct(data, passes=args.passes, seed=config.SEED, error_volume=args.nifti)
        mean, top = anomaly_score(rec.error, rec.count, "mean").cpu(), anomaly_score(rec.error, rec.count, "max").cpu()
        loss = [float(v) for v in rec.loss.cpu()]
        maps.append(rec.error[:take].cpu().numpy())
        if target is not None:
            labels.append(target[:take].cpu().to(torch.int64).view(-1))
        for b in range(take):
            rows.append([str(names[b]), float(mean[b]), float(top[b])] + loss)
            if args.nifti:
                stem = _stem(names[b], taken)
                # NIfTI's first axis is the contiguous one: a channel's [S, S, S] block is written as it lies in memory
                for c in range(data.shape[1]):
                    tag = "" if data.shape[1] == 1 else f"_c{c}"
                    write_nifti(out(f"{stem}_input{tag}.nii.gz"), data[b, c].float().cpu().numpy())
                    write_nifti(out(f"{stem}_recon{tag}.nii.gz"), rec.recon[b, c].cpu().numpy())
                write_nifti(out(f"{stem}_error.nii.gz"), rec.error_volume[b].cpu().numpy())
        done += take
    if not rows:
        raise ValueError("no scans")

    with open(out("scores.csv"), "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["name", "score_mean", "score_max"] + [f"loss_pass{p}" for p in range(n_pass)])
        w.writerows(rows)
    np.save(out("error_maps.npy"), np.concatenate(maps))
    summary = {"passes": n_pass, "cover_passes": need, "mask_ratio": float(model.mask_ratio), "n_scans": len(rows),
               "mean_loss": float(np.mean([r[3:] for r in rows])), "mean_score": float(np.mean([r[1] for r in rows]))}
    if labels:
        summary["label_name"] = args.label_name
        summary["AUROC"] = float(binary_auroc(np.array([r[1] for r in rows]), (torch.cat(labels) > 0).numpy()))
        logger.info(f"AUROC of the mean patch error against {args.label_name} > 0: {summary['AUROC']:.4f}")
    with open(out("reconstruct.json"), "w") as f:
        json.dump(summary, f, indent=1)
    logger.info(f"mean loss {summary['mean_loss']:.6f} over {len(rows)} scans")
    logger.info(f"reconstruction completed: files under {args.save_dir}")
    return summary


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
