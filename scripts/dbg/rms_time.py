"""RMSNorm against LayerNorm, forward and backward launch times on the step's two shapes (encoder 14 080 x 768, decoder 55 552 x 768),
by the method of ln_time.py: inputs rotated over several buffers so that they do not simply sit in the Infinity Cache.  The backward is
called as the plan calls it (bf16 dy, residual gradient added in place, bf16 shadow, column sum).  Both norms are instances of one kernel
family (csrc/elementwise.hip: norm_fwd_reg_kernel / norm_bwd_kernel with RMS = false / true), so the four lines time four instances."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from headct_foundation_amd import _lib
from headct_foundation_amd._lib import HCT_BF16

lib = _lib.load()
dev = torch.device("cuda")
st = torch.cuda.current_stream().cuda_stream


def timed(fn, n=40):
    for i in range(4):
        fn(i)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(n):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


for rows, D, nbuf in [(256 * 55, 768, 8), (256 * 217, 768, 4)]:
    xs = [torch.randn(rows, D, device=dev) for _ in range(nbuf)]
    ys = [torch.empty(rows, D, dtype=torch.bfloat16, device=dev) for _ in range(nbuf)]
    dys = [torch.randn(rows, D, device=dev).bfloat16() for _ in range(nbuf)]
    dxs = [torch.randn(rows, D, device=dev) for _ in range(nbuf)]
    g, b = torch.ones(D, device=dev), torch.zeros(D, device=dev)
    mean, rstd = torch.zeros(rows, device=dev), torch.ones(rows, device=dev)
    dg, db, dc = (torch.empty(D, device=dev) for _ in range(3))
    ws = torch.empty(lib.hct_layernorm_bwd_workspace_bytes(rows, D), dtype=torch.uint8, device=dev)
    p = lambda t: t.data_ptr()
    calls = {
        "layernorm fwd": lambda i: lib.hct_layernorm_fwd(p(xs[i % nbuf]), p(g), p(b), rows, D, 1e-5, p(ys[i % nbuf]), HCT_BF16, p(mean), p(rstd), st),
        "rmsnorm   fwd": lambda i: lib.hct_rmsnorm_fwd(p(xs[i % nbuf]), p(g), rows, D, 1e-6, p(ys[i % nbuf]), HCT_BF16, p(rstd), st),
        "layernorm bwd": lambda i: lib.hct_layernorm_bwd(p(dys[i % nbuf]), HCT_BF16, p(xs[i % nbuf]), p(mean), p(rstd), p(g), p(dxs[i % nbuf]), rows, D,
                                                         p(dxs[i % nbuf]), p(ys[i % nbuf]), HCT_BF16, p(dg), p(db), p(dc), p(ws), ws.numel(), st),
        "rmsnorm   bwd": lambda i: lib.hct_rmsnorm_bwd(p(dys[i % nbuf]), HCT_BF16, p(xs[i % nbuf]), p(rstd), p(g), p(dxs[i % nbuf]), rows, D,
                                                       p(dxs[i % nbuf]), p(ys[i % nbuf]), HCT_BF16, p(dg), p(dc), p(ws), ws.numel(), st),
    }
    for rep in range(2):  # alternated twice
        for name, fn in calls.items():
            _lib.check(fn(0), name)
            print(f"{name} rows={rows} D={D}: {timed(fn):.1f} us", flush=True)
