"""What carrying a prediction back onto the scan's own grid costs on the HIP path.

  kernel   hct_seg_to_native alone at ViT-B/12^3, 96^3, bf16, K = 2 and K = 6, on one synthetic geometry of a 512 x 512 x 160 scan at
           0.45 x 0.45 x 1 mm (LPS on file, a foreground box that is not the whole volume): microseconds per call from HIP events
           around a window of back-to-back calls, beside the torch composition (un-patchify, float, grid_sample onto the file grid,
           arg-max, int16; its sampling grid is built once, outside the timing) in alternating windows of one process; the bytes the
           call has to move (the logits read once, 2 bytes stored per voxel) against the 6.29 TB/s float4-copy floor the other
           benches quote.
  scan     the wall time of one scan as the test pass runs it: tables, upload, kernel, copy to the host and write_nifti of the
           int16 volume as .nii.gz.  The gzip write runs on one host core and dominates; it is host-bound, not a GPU figure.

  python scripts/bench_seg_native.py [--calls 20] [--rounds 3] [--out profiles/seg_native_bench.json]
Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from headct_foundation_amd import _lib, native, nifti  # noqa: E402

COPY_FLOOR_BYTES_PER_S = 6.29e12  # float4 copy on one MI355X, as scripts/bench_ibot.py quotes it
P, G, FIRST = 12, 8, 1
S = P * G


def synthetic_geometry() -> native.ScanGeometry:
    shape, zooms = (512, 512, 160), (0.45, 0.45, 1.0)
    perm, flip = (0, 1, 2), (True, True, False)
    gm = [nifti.spacing_geometry(shape[o], zooms[o]) for o in range(3)]
    affine = np.diag([-0.45, -0.45, 1.0, 1.0])
    affine[:3, 3] = (115.0, 115.0, -80.0)
    return native.ScanGeometry(shape, perm, flip, shape, [g[0] for g in gm], [g[1] for g in gm], affine, (20, 25, 5), (190, 200, 150))


def window(fn, calls: int) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls


def torch_grid(geom, tables, dev):
    """grid_sample's grid [1, nk, nj, ni, 3] and the inside mask for the file grid, from the same tables (clamped coordinates)."""
    ni, nj, nk = geom.file_shape
    t = [torch.from_numpy(tab["i0"].astype(np.float32) + tab["w"]).to(dev) for tab in tables]
    ins = [torch.from_numpy(tab["inside"]).to(dev).bool() for tab in tables]
    grid = torch.empty(1, nk, nj, ni, 3, dtype=torch.float32, device=dev)
    full = [t[0][None, None, :], t[1][None, :, None], t[2][:, None, None]]
    for a in range(3):
        o = geom.perm.index(a)
        grid[0, ..., 2 - o] = ((2.0 * full[a] + 1.0) / S - 1.0).expand(nk, nj, ni)
    inside = ins[2][:, None, None] & ins[1][None, :, None] & ins[0][None, None, :]
    return grid, inside


def bench(lib, dev, calls: int, rounds: int) -> dict:
    geom = synthetic_geometry()
    ni, nj, nk = geom.file_shape
    tables = native.native_tables(geom, S, "linear")
    tabs = native.upload_tables(tables, dev)
    grid, inside = torch_grid(geom, tables, dev)
    voxels = ni * nj * nk
    T = FIRST + G ** 3
    out = {}
    for K in (2, 6):
        N = K * P ** 3
        g = torch.Generator(device=dev).manual_seed(K)
        logits = (2 * torch.randn(T, N, device=dev, generator=g)).to(torch.bfloat16)
        pred = torch.empty(nk, nj, ni, dtype=torch.int16, device=dev)
        cv = torch.empty(K, dtype=torch.int64, device=dev)
        ws = torch.empty(lib.hct_seg_to_native_workspace_bytes(ni, nj, nk, K), dtype=torch.uint8, device=dev)
        st = torch.cuda.current_stream().cuda_stream

        def hip():
            _lib.check(lib.hct_seg_to_native(logits.data_ptr(), _lib.HCT_BF16, N, T, FIRST, G, P, K, tabs["i0"].data_ptr(), tabs["i1"].data_ptr(),
                                             tabs["w"].data_ptr(), tabs["inside"].data_ptr(), *geom.perm, ni, nj, nk, None, pred.data_ptr(),
                                             cv.data_ptr(), None, ws.data_ptr(), ws.numel(), st), "hct_seg_to_native")

        def composed():
            x = logits[FIRST:].reshape(G, G, G, K, P, P, P).permute(3, 0, 4, 1, 5, 2, 6).reshape(1, K, S, S, S).float()
            v = torch.nn.functional.grid_sample(x, grid, mode="bilinear", padding_mode="border", align_corners=False)
            return torch.where(inside, v[0].argmax(0), 0).to(torch.int16)
        for _ in range(3):
            hip()
        ref = composed()
        torch.cuda.synchronize()
        w_hip, w_torch = [], []
        for _ in range(rounds):  # alternate the two in one process
            w_hip.append(window(hip, calls))
            w_torch.append(window(composed, max(1, calls // 10)))
        hip()
        torch.cuda.synchronize()
        agree = float((pred == ref).float().mean())
        del ref
        t0 = time.perf_counter()  # one scan as the test pass runs it
        res = native.seg_to_native(logits, P, K, FIRST, geom, "linear")
        host = res["pred"].cpu().numpy()
        t1 = time.perf_counter()
        with tempfile.TemporaryDirectory() as d:
            nifti.write_nifti(os.path.join(d, "scan_native.nii.gz"), host, affine=np.asarray(geom.affine), dtype="i2")
            size = os.path.getsize(os.path.join(d, "scan_native.nii.gz"))
        t2 = time.perf_counter()
        nbytes = S ** 3 * K * 2 + voxels * 2
        us = statistics.median(w_hip)
        out[f"K{K}"] = {"us_per_call": round(us, 1), "windows_us": [round(v, 1) for v in w_hip], "calls_per_window": calls,
                        "torch_composition_us": round(statistics.median(w_torch), 1), "torch_windows_us": [round(v, 1) for v in w_torch],
                        "speedup": round(statistics.median(w_torch) / us, 2), "bytes": nbytes, "TB_per_s": round(nbytes / us * 1e-6, 3),
                        "share_of_copy_floor": round(nbytes / us * 1e6 / COPY_FLOOR_BYTES_PER_S, 3), "agreement_with_torch": round(agree, 6),
                        "class_voxels": [int(v) for v in cv.cpu()],
                        "scan_wall_s": {"tables_kernel_copy_to_host": round(t1 - t0, 3), "gzip_write_host_bound": round(t2 - t1, 3),
                                        "total": round(t2 - t0, 3), "file_bytes": size}}
        del logits, pred
        torch.cuda.empty_cache()
    return {"shape": "ViT-B/12^3, 96^3, bf16 -> 512 x 512 x 160 at 0.45 x 0.45 x 1 mm, box 190 x 200 x 150 of 231 x 231 x 160 mm", **out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="", help="also write the JSON to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_seg_native.py needs an MI355X: nothing here is measured on the CPU")
    dev = torch.device("cuda:0")
    result = {"metric": "segmentation on the scan's own grid (bf16, one MI355X)", "hct_seg_to_native": bench(_lib.load(), dev, a.calls, a.rounds)}
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
