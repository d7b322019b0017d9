"""The loading chain (NIfTI -> fp16 cache item) per volume, on a 512 x 512 x 160 int16 phantom at 0.47 x 0.47 x 1.3 mm stored
gzip-compressed in the usual axial LPS order.

    python scripts/bench_loading.py [--reps 5] [--iters 5] [--roi 96] [--channels 3] [--no-cpu]
        host decode (gunzip + header + tables + staging into pinned memory), the upload, the device chain (HIP events around
        `iters` runs of run_loading_chain on an uploaded buffer, median and spread of `reps` repeats) and `load_volume` as a
        whole (host clock); GB/s of the device chain against the bytes its kernels must move (each buffer written once and read
        once by the next kernel); and, beside it, the scipy / torch chain of tests/loading_ref.py on the CPU with 16 threads (once).
        One JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from headct_foundation_amd.data import DecodedVolume, load_volume, run_loading_chain  # noqa: E402
from tests import loading_ref as R  # noqa: E402

SHAPE, ZOOMS = (512, 512, 160), (0.47, 0.47, 1.3)


def timed(fn, iters):
    """ms per call: HIP events around `iters` calls."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def stats(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def main(args):
    dev = torch.device("cuda", 0)
    roi, chans = (args.roi,) * 3, args.channels
    raw = R.to_int16(R.phantom(SHAPE, seed=0), R.INT16_SLOPE, R.INT16_INTER)
    aff = np.diag([*ZOOMS, 1.0])
    stored, saff = R.stored_as(raw, aff, (0, 1, 2), (-1, -1, 1))  # LPS
    path = os.path.join(tempfile.mkdtemp(), "phantom.nii.gz")
    R.write_nifti(path, stored, saff, slope=R.INT16_SLOPE, inter=R.INT16_INTER)
    file_bytes = os.path.getsize(path)

    decode = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        dec = DecodedVolume(path)
        decode.append((time.perf_counter() - t0) * 1e3)
    gunzip = []
    for _ in range(args.reps):
        import gzip
        t0 = time.perf_counter()
        with gzip.open(path, "rb") as f:
            f.read()
        gunzip.append((time.perf_counter() - t0) * 1e3)
    staged = dec.host.to(dev, non_blocking=True)
    upload = [timed(lambda: staged.copy_(dec.host, non_blocking=True), args.iters) for _ in range(args.reps)]
    run_loading_chain(dec, staged, roi, chans)
    torch.cuda.synchronize()
    chain = [timed(lambda: run_loading_chain(dec, staged, roi, chans), args.iters) for _ in range(args.reps)]
    whole = []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        item = load_volume(path, roi, chans, dev)
        whole.append((time.perf_counter() - t0) * 1e3)
    d, m = dec.d, dec.m
    vox = lambda s: int(np.prod(s))
    moved = (vox(d) * 2 + vox(d) * 4                      # to RAS: int16 in, fp32 out
             + vox(d) * 4 + vox([m[0], d[1], d[2]]) * 8   # pass 0: fp32 in, float64 out
             + vox([m[0], d[1], d[2]]) * 8 + vox([m[0], m[1], d[2]]) * 8
             + vox([m[0], m[1], d[2]]) * 8 + vox(m) * 4   # pass 2: float64 in, fp32 out
             + vox(m) * 4                                 # box
             + vox(m) * 4 + chans * vox(roi) * 2)         # crop + window + resize (at most the whole volume in)
    out = {
        "metric": "loading chain per volume (NIfTI int16 .nii.gz -> fp16 cache item), device chain by HIP events, host parts by the host clock",
        "file_shape": list(SHAPE), "zooms": list(ZOOMS), "resampled_shape": m, "roi": list(roi), "channels": chans, "file_bytes": file_bytes,
        "reps": args.reps, "iters": args.iters,
        "host_decode_ms": stats(decode), "of_which_gunzip_ms": stats(gunzip), "upload_ms": stats(upload), "device_chain_ms": stats(chain),
        "load_volume_ms": stats(whole), "device_chain_bytes_moved": moved,
        "device_chain_GBps": round(moved / statistics.median(chain) / 1e6, 1),
        "volumes_per_s_device_chain": round(1e3 / statistics.median(chain), 1), "volumes_per_s_load_volume": round(1e3 / statistics.median(whole), 2),
    }
    if not args.no_cpu:
        torch.set_num_threads(16)
        t0 = time.perf_counter()
        values = R.scaled(raw, R.INT16_SLOPE, R.INT16_INTER)
        zooms = [float(np.float32(z)) for z in ZOOMS]
        vol = R.resample_f64(values, zooms)
        t1 = time.perf_counter()
        want = R.window_resize(vol.astype(np.float32), R.foreground_box(vol), roi, chans)
        t2 = time.perf_counter()
        steps = R.fp16_steps(item, want)
        out.update({"cpu_chain_ms": round((t2 - t0) * 1e3, 1), "cpu_resample_ms": round((t1 - t0) * 1e3, 1), "cpu_threads": 16,
                    "item_vs_cpu_chain": {"share_differing": round(float((steps > 0).float().mean()), 6), "max_fp16_steps": int(steps.max())}})
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--roi", type=int, default=96)
    ap.add_argument("--channels", type=int, default=3)
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_loading.py measures on the GPU; there is no CPU path")
    main(args)
