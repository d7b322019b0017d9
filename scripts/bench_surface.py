"""Timing of the surface-distance metrics (headct_foundation_amd/surface.py, csrc/surface.hip) at the size of a head CT:
512 x 512 x 160 voxels of 0.45 x 0.45 x 1 mm, planted ellipsoid pairs of about 30 mL and about 1.3 L, K = 2 and K = 6 (the
ellipsoid cut into five slabs).

    python scripts/bench_surface.py [--cases 30ml 1300ml] [--classes 2 6] [--reps 5] [--scipy_reps 1] [--scan] [--out profiles/surface_bench.json]

Per case: `surface_metrics` (wall time around a device synchronisation: the call reads a box and a result back per class, so the
host's share belongs to it) alternating with the scipy composition of tests/surface_ref.py on the same masks, which is the only
yardstick there is; the per-stage split of one class (edges, the transform of both surfaces, statistics, select) from HIP events;
and the transform's fused-min steps and bytes against the fp64 vector rate and the float4-copy floor.  `--scan` times the native
pass of one scan (seg_to_native on planted logits, then the metrics) with the switch off and on.  Medians go to --out.
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

from headct_foundation_amd import _lib, native, surface  # noqa: E402
from tests import surface_ref as R  # noqa: E402

SHAPE = (160, 512, 512)          # [nk, nj, ni]
SPACING = (1.0, 0.45, 0.45)      # (s_k, s_j, s_i) in mm
RADII_MM = {"30ml": (19.3, 19.3, 19.3), "1300ml": (59.0, 70.0, 75.0)}   # 4/3 pi abc = 30.1 mL and 1.30 L
COPY_FLOOR = 6.29e12             # bytes / s of a float4 copy on this chip
FP64_OPS = 78.6e12 / 2           # fp64 vector instructions / s (78.6 TFLOP/s counts a fused multiply-add as two)
STEP_OPS = 4                     # multiply by the spacing, square, add, minimum


def planted(case: str, K: int):
    """(pred int16, labels uint8): an ellipsoid of the case's volume as labels, the prediction 3 % larger and shifted by (2, 5, -4)
    voxels; for K > 2 both are cut into K - 1 slabs along k, one class each."""
    radii = [r / s for r, s in zip(RADII_MM[case], SPACING)]
    centre = (SHAPE[0] / 2, SHAPE[1] / 2, SHAPE[2] / 2)
    g = R.ellipsoid(SHAPE, centre, radii)
    p = R.ellipsoid(SHAPE, (centre[0] + 2, centre[1] + 5, centre[2] - 4), [1.03 * r for r in radii])
    k = np.arange(SHAPE[0])[:, None, None]
    lo, hi = centre[0] - radii[0], centre[0] + radii[0]
    cls = np.clip(((k - lo) / (hi - lo) * (K - 1)).astype(np.int64), 0, K - 2) + 1
    return np.where(p, cls, 0).astype(np.int16), np.where(g, cls, 0).astype(np.uint8)


def wall(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out


def stage_split(pred, labels, c, tau):
    """HIP-event times in ms of one class's stages, and the box."""
    lib, dev = _lib.load(), pred.device
    nk, nj, ni = pred.shape
    st = _lib.stream_ptr(dev)
    flags = torch.empty(nk, nj, ni, dtype=torch.uint8, device=dev)
    dg, dp = (torch.empty(nk, nj, ni, dtype=torch.float64, device=dev) for _ in range(2))
    ws = torch.empty(max(lib.hct_surface_edges_workspace_bytes(nk, nj, ni), lib.hct_surface_stats_workspace_bytes(nk, nj, ni),
                         lib.hct_surface_select_workspace_bytes()), dtype=torch.uint8, device=dev)
    head, counts, vals = torch.empty(8, dtype=torch.int64, device=dev), torch.empty(4, dtype=torch.int64, device=dev), torch.empty(8, dtype=torch.float64, device=dev)
    _lib.check(lib.hct_surface_edges(pred.data_ptr(), labels.data_ptr(), nk, nj, ni, c, flags.data_ptr(), head.data_ptr(), ws.data_ptr(), ws.numel(), st))
    n_p, n_g, *box = head.cpu().tolist()
    ranks = surface.percentile_ranks(n_p)[:2] + surface.percentile_ranks(n_g)[:2]
    stages = {
        "edges": lambda: lib.hct_surface_edges(pred.data_ptr(), labels.data_ptr(), nk, nj, ni, c, flags.data_ptr(), head.data_ptr(), ws.data_ptr(), ws.numel(), st),
        "edt_both": lambda: (lib.hct_edt3d(flags.data_ptr(), 2, nk, nj, ni, *box, *SPACING, dg.data_ptr(), st),
                             lib.hct_edt3d(flags.data_ptr(), 1, nk, nj, ni, *box, *SPACING, dp.data_ptr(), st)),
        "stats": lambda: lib.hct_surface_stats(flags.data_ptr(), dg.data_ptr(), dp.data_ptr(), nk, nj, ni, *box, tau, counts.data_ptr(), vals.data_ptr(),
                                               ws.data_ptr(), ws.numel(), st),
        "select": lambda: lib.hct_surface_select(flags.data_ptr(), dg.data_ptr(), dp.data_ptr(), nk, nj, ni, *box, *ranks, vals[4:].data_ptr(), ws.data_ptr(),
                                                 ws.numel(), st),
    }
    out = {}
    for name, fn in stages.items():
        times = []
        for _ in range(6):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b))
        out[name + "_ms"] = statistics.median(times[1:])
    bk, bj, bi = (box[3 + a] - box[a] for a in range(3))
    cells = bk * bj * bi
    steps, nbytes = 2.0 * cells * (bk + bj + bi), 2.0 * cells * 41  # per surface: flags in, float64 out, then two in-place passes
    sec = out["edt_both_ms"] / 1e3
    out.update(box=[bk, bj, bi], n_pred=n_p, n_gt=n_g, edt_steps=steps, edt_bytes=nbytes, edt_steps_per_s=steps / sec, edt_bytes_per_s=nbytes / sec,
               edt_share_of_fp64_rate=steps * STEP_OPS / sec / FP64_OPS, edt_share_of_copy_floor=nbytes / sec / COPY_FLOOR,
               edt_pass_steps={"k": 2.0 * cells * bk, "j": 2.0 * cells * bj, "i": 2.0 * cells * bi})
    return out


def bench_case(case, K, reps, scipy_reps, dev):
    pred, labels = planted(case, K)
    pd, yd = torch.from_numpy(pred).to(dev), torch.from_numpy(labels).to(dev)
    tau = 2.0
    surface.surface_metrics(pd, yd, K, SPACING, tau)  # warm-up
    t_dev, t_ref, got, want = [], [], None, None
    for r in range(max(reps, scipy_reps)):
        if r < reps:
            t_dev += wall(lambda: surface.surface_metrics(pd, yd, K, SPACING, tau), 1)
        if r < scipy_reps:
            t0 = time.perf_counter()
            want = R.surface_metrics(pred, labels, K, SPACING, tau)
            t_ref.append(time.perf_counter() - t0)
    got = surface.surface_metrics(pd, yd, K, SPACING, tau)
    res = {"case": case, "K": K, "device_s": statistics.median(t_dev), "device_s_all": t_dev, "HD95": got["HD95"][1:].tolist(), "ASSD": got["ASSD"][1:].tolist(),
           "NSD": got["NSD"][1:].tolist(), "volume_ml": float((labels > 0).sum() * np.prod(SPACING) / 1000.0)}
    if t_ref:
        worst = max(float(np.nanmax(np.abs(got[k][1:] - want[k][1:]) / np.maximum(np.abs(want[k][1:]), 1e-300))) for k in ("HD", "HD95", "ASSD"))
        res.update(scipy_s=statistics.median(t_ref), scipy_s_all=t_ref, speedup=statistics.median(t_ref) / statistics.median(t_dev), worst_rel_diff=worst,
                   nsd_equal=bool(np.array_equal(got["NSD"], want["NSD"], equal_nan=True)))
    res["stages_class_1"] = stage_split(pd, yd, 1, tau)
    return res


def bench_scan(reps, dev):
    """seg_to_native on planted logits (K = 2, a 96^3 item of 8^3 patches) for a 512 x 512 x 160 scan, then the metrics: the
    native pass's device work per scan with SEG.SURFACE_METRICS off and on."""
    G, P, K = 8, 12, 2
    S = G * P
    ni, nj, nk = SHAPE[2], SHAPE[1], SHAPE[0]
    steps = (1.0 / 0.45, 1.0 / 0.45, 1.0)
    m = (int(ni * 0.45), int(nj * 0.45), nk)
    aff = np.diag([0.45, 0.45, 1.0, 1.0])
    geom = native.ScanGeometry((ni, nj, nk), (0, 1, 2), (False, False, False), (ni, nj, nk), m, steps, aff, (0, 0, 0), m)
    inside = torch.from_numpy(R.ellipsoid((S, S, S), (S / 2, S / 2 + 3, S / 2), (S * 0.09, S * 0.09, S * 0.13)))
    vol = torch.where(inside, 5.0, -5.0).to(torch.float32)
    vol = torch.stack([-vol, vol])                                                              # [K, t0, t1, t2]
    tok = vol.view(K, G, P, G, P, G, P).permute(1, 3, 5, 0, 2, 4, 6).reshape(G ** 3, K * P ** 3)
    tok = torch.cat([torch.zeros(1, K * P ** 3), tok]).to(dev)
    labels = np.zeros(SHAPE, np.uint8)
    labels[R.ellipsoid(SHAPE, (SHAPE[0] / 2 + 2, SHAPE[1] / 2 + 4, SHAPE[2] / 2 - 3), [r / s for r, s in zip(RADII_MM["30ml"], SPACING)])] = 1
    yd = torch.from_numpy(labels).to(dev)
    tabs = native.upload_tables(native.native_tables(geom, S), dev)

    def off():
        return native.seg_to_native(tok, P, K, 1, geom, labels=yd, tables=tabs)

    def on():
        out = off()
        return surface.surface_metrics(out["pred"], yd, K, surface.voxel_spacing(aff), 2.0)

    off(), on()
    t_off, t_on = [], []
    for _ in range(reps):
        t_off += wall(off, 1)
        t_on += wall(on, 1)
    got = on()
    return {"off_s": statistics.median(t_off), "on_s": statistics.median(t_on), "HD95": got["HD95"][1:].tolist(), "n_pred": got["n_pred"][1:].tolist(),
            "n_gt": got["n_gt"][1:].tolist()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=list(RADII_MM), choices=list(RADII_MM))
    ap.add_argument("--classes", nargs="+", type=int, default=[2, 6])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scipy_reps", type=int, default=1)
    ap.add_argument("--scan", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surface_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    result = {"date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(dev), "shape_kji": list(SHAPE), "spacing_kji_mm": list(SPACING),
              "reps": args.reps, "scipy_reps": args.scipy_reps, "cases": []}
    for case in args.cases:
        for K in args.classes:
            res = bench_case(case, K, args.reps, args.scipy_reps, dev)
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
