"""Timing of the connected-component kernels (headct_foundation_amd/components.py, csrc/components.hip) at the size of a head CT:
512 x 512 x 160 voxels of 0.45 x 0.45 x 1 mm, K = 2, at connectivity 6 and 26, on three masks: `specks` (an ellipsoid pair of about
30 mL plus 200 specks of one to eight voxels), `large` (a pair of about 1.3 L) and `bernoulli` (every voxel on with probability 0.3,
the many-components worst case).

    python scripts/bench_components.py [--cases specks large bernoulli] [--connectivity 6 26] [--reps 5] [--scipy_reps 1] [--scan]
                                       [--out profiles/components_bench.json]

Per case and connectivity: the stages (masks, label, compact, sizes, overlap, remove, recount) from HIP events, their algorithmic
bytes against the float4-copy floor, and label + compact + sizes alternating with scipy.ndimage.label + numpy.bincount on the same
mask on the host, which is the only yardstick there is.  `--scan` times the native pass of one scan (seg_to_native on planted
logits) with SEG.MIN_COMPONENT_ML / SEG.LESION_METRICS off and on.  Medians go to --out.
"""
import argparse
import datetime
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from headct_foundation_amd import _lib, components, native  # noqa: E402
from tests import components_ref as R  # noqa: E402

SHAPE = (160, 512, 512)          # [nk, nj, ni]
SPACING = (1.0, 0.45, 0.45)      # (s_k, s_j, s_i) in mm
RADII_MM = {"specks": (19.3, 19.3, 19.3), "large": (59.0, 70.0, 75.0)}   # 4/3 pi abc = 30.1 mL and 1.30 L
COPY_FLOOR = 6.29e12             # bytes / s of a float4 copy on this chip
# bytes per voxel a stage has to move at the least: inputs read once, outputs written once
STAGE_BYTES = {"masks": 2 + 1 + 1, "label": 1 + 4, "compact": 4 + 4, "sizes": 4, "overlap": 4 + 1, "remove": 4 + 2, "recount": 2 + 1}


def planted(case: str):
    """(pred int16, labels uint8), K = 2."""
    if case == "bernoulli":
        return R.bernoulli(SHAPE, 0.3, 0).astype(np.int16), R.bernoulli(SHAPE, 0.3, 1).astype(np.uint8)
    radii = [r / s for r, s in zip(RADII_MM[case], SPACING)]
    centre = (SHAPE[0] / 2, SHAPE[1] / 2, SHAPE[2] / 2)
    g = R.ellipsoid(SHAPE, centre, radii)
    p = R.ellipsoid(SHAPE, (centre[0] + 2, centre[1] + 5, centre[2] - 4), [1.03 * r for r in radii])
    if case == "specks":
        gen = np.random.default_rng(0)
        for _ in range(200):
            k, j, i = (int(gen.integers(2, s - 4)) for s in SHAPE)
            p[k:k + int(gen.integers(1, 3)), j:j + int(gen.integers(1, 3)), i:i + int(gen.integers(1, 3))] = True
    return p.astype(np.int16), g.astype(np.uint8)


def event_ms(fn, reps=6):
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times[1:])


def bench_case(case, conn, reps, scipy_reps, dev):
    pred, labels = planted(case)
    lib = _lib.load()
    nk, nj, ni = SHAPE
    nvox = nk * nj * ni
    pd, yd = torch.from_numpy(pred).to(dev), torch.from_numpy(labels).to(dev)
    st = _lib.stream_ptr(dev)
    flags = torch.empty(SHAPE, dtype=torch.uint8, device=dev)
    lab = torch.empty(SHAPE, dtype=torch.int32, device=dev)
    n_dev = torch.empty(1, dtype=torch.int64, device=dev)
    ws = torch.empty(max(16, lib.hct_cc_label_workspace_bytes(nk, nj, ni), lib.hct_cc_compact_workspace_bytes(nk, nj, ni),
                         lib.hct_seg_recount_workspace_bytes(nk, nj, ni, 2)), dtype=torch.uint8, device=dev)
    cv, cn = torch.empty(2, dtype=torch.int64, device=dev), torch.empty(2, 3, dtype=torch.int64, device=dev)
    scratch = pd.clone()

    def masks():
        _lib.check(lib.hct_cc_masks(pd.data_ptr(), yd.data_ptr(), nk, nj, ni, 1, flags.data_ptr(), st))

    def label():
        _lib.check(lib.hct_cc_label(flags.data_ptr(), 1, nk, nj, ni, conn, lab.data_ptr(), ws.data_ptr(), ws.numel(), st))

    def compact():
        _lib.check(lib.hct_cc_compact(lab.data_ptr(), nk, nj, ni, n_dev.data_ptr(), ws.data_ptr(), ws.numel(), st))

    masks(), label(), compact()
    n = int(n_dev.item())
    sizes, over = torch.empty(n + 1, dtype=torch.int64, device=dev), torch.empty(n + 1, dtype=torch.int64, device=dev)
    stages = {
        "masks": masks,
        "label": label,
        "compact": lambda: (label(), compact()),  # compact needs root form each time: the label stage's median is subtracted below
        "sizes": lambda: _lib.check(lib.hct_cc_sizes(lab.data_ptr(), nvox, n, sizes.data_ptr(), st)),
        "overlap": lambda: _lib.check(lib.hct_cc_overlap(lab.data_ptr(), n, flags.data_ptr(), 2, nvox, over.data_ptr(), st)),
        "remove": lambda: _lib.check(lib.hct_cc_remove_small(scratch.data_ptr(), lab.data_ptr(), sizes.data_ptr(), 10, nvox, st)),
        "recount": lambda: _lib.check(lib.hct_seg_recount(pd.data_ptr(), yd.data_ptr(), nk, nj, ni, 2, cv.data_ptr(), cn.data_ptr(), ws.data_ptr(), ws.numel(),
                                                          st)),
    }
    ms = {name: event_ms(fn) for name, fn in stages.items()}
    ms["compact"] = max(ms["compact"] - ms["label"], 0.0)
    label(), compact()
    res = {"case": case, "connectivity": conn, "components": n, "mask_voxels": int((pred == 1).sum()), "stage_ms": ms,
           "stage_share_of_copy_floor": {k: STAGE_BYTES[k] * nvox / COPY_FLOOR / (v / 1e3) if v > 0 else None for k, v in ms.items()}}

    def device():
        label(), compact()
        m = int(n_dev.item())
        return components.component_sizes(lab, m)

    mask = (pred == 1) & (labels != 255)
    t_dev, t_ref, want = [], [], None
    for r in range(max(reps, scipy_reps)):
        if r < reps:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = device()
            torch.cuda.synchronize()
            t_dev.append(time.perf_counter() - t0)
        if r < scipy_reps:
            t0 = time.perf_counter()
            want, want_n = R.label_ref(mask, conn)
            want_sizes = np.bincount(want.reshape(-1), minlength=want_n + 1)
            t_ref.append(time.perf_counter() - t0)
    res.update(device_s=statistics.median(t_dev), device_s_all=t_dev)
    if t_ref:
        want_sizes[0] = 0
        res.update(scipy_s=statistics.median(t_ref), scipy_s_all=t_ref, speedup=statistics.median(t_ref) / statistics.median(t_dev),
                   labels_equal=bool(np.array_equal(lab.cpu().numpy(), want)), sizes_equal=bool(np.array_equal(got.cpu().numpy(), want_sizes)))
    return res


def bench_scan(reps, dev):
    """seg_to_native on planted logits (K = 2, a 96^3 item of 8^3 patches) for a 512 x 512 x 160 scan, then the filter at 0.05 mL and
    the lesion metrics at connectivity 26: the native pass's device work per scan with the two features off and on."""
    G, P, K = 8, 12, 2
    S = G * P
    ni, nj, nk = SHAPE[2], SHAPE[1], SHAPE[0]
    steps = (1.0 / 0.45, 1.0 / 0.45, 1.0)
    m = (int(ni * 0.45), int(nj * 0.45), nk)
    aff = np.diag([0.45, 0.45, 1.0, 1.0])
    geom = native.ScanGeometry((ni, nj, nk), (0, 1, 2), (False, False, False), (ni, nj, nk), m, steps, aff, (0, 0, 0), m)
    inside = torch.from_numpy(R.ellipsoid((S, S, S), (S / 2, S / 2 + 3, S / 2), (S * 0.09, S * 0.09, S * 0.13)))
    inside[5:7, 20:22, 30:31] = True  # a speck the filter removes
    vol = torch.where(inside, 5.0, -5.0).to(torch.float32)
    vol = torch.stack([-vol, vol])                                                              # [K, t0, t1, t2]
    tok = vol.view(K, G, P, G, P, G, P).permute(1, 3, 5, 0, 2, 4, 6).reshape(G ** 3, K * P ** 3)
    tok = torch.cat([torch.zeros(1, K * P ** 3), tok]).to(dev)
    labels = np.zeros(SHAPE, np.uint8)
    labels[R.ellipsoid(SHAPE, (SHAPE[0] / 2 + 2, SHAPE[1] / 2 + 4, SHAPE[2] / 2 - 3), [r / s for r, s in zip(RADII_MM["specks"], SPACING)])] = 1
    yd = torch.from_numpy(labels).to(dev)
    tabs = native.upload_tables(native.native_tables(geom, S), dev)
    mv = components.min_voxels_for(0.05, aff)

    def off():
        return native.seg_to_native(tok, P, K, 1, geom, labels=yd, tables=tabs)

    def on():
        out = off()
        kept = components.remove_small_components(out["pred"], K, mv, 26, labels=yd)
        return kept, components.lesion_metrics(kept["pred"], yd, K, 26)

    off(), on()
    t_off, t_on = [], []
    for _ in range(reps):
        for fn, acc in ((off, t_off), (on, t_on)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            acc.append(time.perf_counter() - t0)
    kept, les = on()
    return {"off_s": statistics.median(t_off), "on_s": statistics.median(t_on), "min_voxels": mv, "removed": kept["removed"].tolist(),
            "n_gt": les["n_gt"].tolist(), "n_pred": les["n_pred"].tolist(), "gt_detected": les["gt_detected"].tolist(),
            "pred_matched": les["pred_matched"].tolist()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["specks", "large", "bernoulli"], choices=["specks", "large", "bernoulli"])
    ap.add_argument("--connectivity", nargs="+", type=int, default=[6, 26], choices=[6, 18, 26])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scipy_reps", type=int, default=1)
    ap.add_argument("--scan", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "components_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    result = {"date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(dev), "shape_kji": list(SHAPE), "spacing_kji_mm": list(SPACING),
              "reps": args.reps, "scipy_reps": args.scipy_reps, "tile_dims": list(components.tile_dims()), "form": "global union-find, runs pre-linked",
              "cases": []}
    for case in args.cases:
        for conn in args.connectivity:
            res = bench_case(case, conn, args.reps, args.scipy_reps, dev)
            result["cases"].append(res)
            print(json.dumps({k: v for k, v in res.items() if not k.endswith("_all")}), flush=True)
    if args.scan:
        result["scan"] = bench_scan(args.reps, dev)
        print(json.dumps(result["scan"]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
