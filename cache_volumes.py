"""Warm the persistent cache ahead of training: the role of the reference's cpu_caching.py (driven by run_cache_data.py), with the
loading chain on the device instead of on CPU workers.

  python cache_volumes.py --cfg configs/mae/mae_HeadCT.yaml --csv <path-to>/train.csv --start_idx 0 --end_idx 1000
  python cache_volumes.py --cfg CFG.yaml --csv <path-to>/rsna_train_label.csv     (a label CSV of the fine-tuning tasks: only img_path is read)

Rows [start_idx, end_idx) of the CSV's img_path column go through VolumeCache (MODEL.ROI, MODEL.IN_CHANS, DATA.CACHE_DIR of the
config); one status line per scan, a final count of failures, exit status 1 if any failed."""
import argparse
import sys
import time

import torch

from config import get_config
from headct_foundation_amd.data import VolumeCache, read_image_paths


def parse_option():
    parser = argparse.ArgumentParser('fill the fp16 volume cache', add_help=True)
    parser.add_argument('--cfg', type=str, required=True, metavar="FILE", help='path to config file')
    parser.add_argument("--opts", help="Modify config options using the command-line", default=None, nargs='+')
    parser.add_argument('--csv', type=str, required=True, help='CSV with an img_path column (a pre-training list or a label CSV of the fine-tuning tasks)')
    parser.add_argument('--start_idx', type=int, default=0)
    parser.add_argument('--end_idx', type=int, default=None, help='one past the last row (default: the end of the file)')
    parser.add_argument("--local_rank", type=int, default=0)
    args = parser.parse_args()
    return args, get_config(args)


def main(args, config) -> int:
    if not torch.cuda.is_available():
        raise SystemExit("cache_volumes.py needs an MI355X: the loading chain has no CPU fallback")
    device = torch.device("cuda", args.local_rank)
    paths = read_image_paths(args.csv)
    end = len(paths) if args.end_idx is None else min(args.end_idx, len(paths))
    cache = VolumeCache(config.DATA.CACHE_DIR, config.MODEL.ROI, config.MODEL.IN_CHANS)
    failed = 0
    for idx in range(max(0, args.start_idx), end):
        t0 = time.perf_counter()
        try:
            cache.get(paths[idx], device)
            print(f"[{idx}] ok {time.perf_counter() - t0:.2f}s {paths[idx]}", flush=True)
        except Exception as e:
            failed += 1
            print(f"[{idx}] FAILED {paths[idx]}: {e}", flush=True)
    print(f"cached rows [{max(0, args.start_idx)}, {end}) of {args.csv}: {failed} failed", flush=True)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main(*parse_option()))
