"""Volume-to-volume retrieval search: FeatureBank.search (hct_topk_dot: fused similarity + top-k, no [Q, G] matrix) against
(qn @ gn.T).topk(k) in torch, on the same normalised bf16 operands.  G = 25 000 gallery scans, D = 768, Q = 4 096 queries, k = 10.
Both run in one process in alternating blocks of timed calls, each block between two device synchronisations.  Prints one JSON line:
ms per search for each (median over the blocks, and the spread), and for the fused kernel its TFLOP/s (2 Q G D operations) and the
share of its operand-read floor ((Q + G) D 2 bytes at 8 TB/s: what the search costs when both operands are read once).

  python scripts/bench_retrieval.py [--gallery 25000] [--queries 4096] [--dim 768] [--k 10] [--blocks 5] [--iters 10]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from headct_foundation_amd import _lib  # noqa: E402
from headct_foundation_amd.retrieval import FeatureBank, topk_dot  # noqa: E402

HBM_BYTES_PER_S = 8.0e12


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gallery", type=int, default=25000)
    ap.add_argument("--queries", type=int, default=4096)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_retrieval.py needs an MI355X: the search has no CPU fallback")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    G, Q, D, k = a.gallery, a.queries, a.dim, a.k
    bank = FeatureBank(torch.randn(G, D, device=dev, generator=gen), dtype="bf16")
    qn = FeatureBank(torch.randn(Q, D, device=dev, generator=gen), dtype="bf16").feats  # the queries, normalised once for both sides
    gn = bank.feats

    fused = lambda: topk_dot(qn, gn, k)
    eager = lambda: (qn @ gn.T).topk(k, dim=1)
    # the two agree: same rows except where bf16 scores of the eager product tie or round across the k-th place
    s_f, i_f = fused()
    s_e, i_e = eager()
    same = float((i_f.to(torch.int64).sort(dim=1).values == i_e.sort(dim=1).values).float().mean())
    for _ in range(a.warmup):
        fused(), eager()
    ms_f, ms_e = [], []
    for _ in range(a.blocks):
        ms_f.append(timed(fused, a.iters))
        ms_e.append(timed(eager, a.iters))
    med = lambda v: sorted(v)[len(v) // 2]
    f, e = med(ms_f), med(ms_e)
    flops = 2.0 * Q * G * D
    floor_ms = (Q + G) * D * 2 / HBM_BYTES_PER_S * 1e3
    print(json.dumps({
        "metric": "retrieval search, bf16 unit vectors", "gallery": G, "queries": Q, "dim": D, "k": k, "blocks": a.blocks, "iters": a.iters,
        "fused_ms": round(f, 4), "fused_ms_min_max": [round(min(ms_f), 4), round(max(ms_f), 4)],
        "torch_matmul_topk_ms": round(e, 4), "torch_ms_min_max": [round(min(ms_e), 4), round(max(ms_e), 4)],
        "fused_tflops": round(flops / (f * 1e-3) / 1e12, 2), "operand_read_floor_ms": round(floor_ms, 5),
        "fused_share_of_operand_read_floor": round(floor_ms / f, 5),
        "fused_workspace_mb": round(_lib.load().hct_topk_dot_workspace(Q, G, k) / 2 ** 20, 2),
        "score_matrix_mb": round(Q * G * 2 / 2 ** 20, 1), "rows_in_common_with_torch": round(same, 5),
    }))


if __name__ == "__main__":
    main()
