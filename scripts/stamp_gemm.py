"""In-kernel timeline of the persistent NT GEMM (diagnostic build: `python -m headct_foundation_amd.build --stamps`).

Wave 0 of every workgroup stamps s_memrealtime (100 MHz, chip-global) at four points of each tile:
  0 tile top | 1 first stage landed | 2 main loop done | 3 epilogue issued (all stores in flight)
and sums, per tile, the time it spends in the main loop's landing waits (from the counted wait to the barrier's exit, K / 64 - 1
of them per tile).  Prints, per call, the chip-wide mean of each segment per tile index, and the landing wait per stage pair against
the main loop's time per pair.  `walk=W` sets the tile walk's band width, `cold` as an argument writes 1 GiB between the launches, so that the operands come from HBM as they
do inside the training step and not from the Infinity Cache; `out=FILE` also writes the per-shape summary as JSON.
Shares only: the stamps' fences cost a little, never quote this build's run time.
"""
import ctypes as C, os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from headct_foundation_amd import _lib
_lib.LIB_PATH = os.path.join(os.path.dirname(_lib.LIB_PATH), f"libheadct_hip_{os.environ.get('HCT_STAMP_LIB', 'stamps')}.so")
from headct_foundation_amd._lib import HCT_BF16, HCT_F32, GemmArgs
lib = _lib.load(); dev = torch.device("cuda"); st = torch.cuda.current_stream().cuda_stream
lib.hct_debug_set_stamp_buffer.restype = C.c_int
lib.hct_debug_set_stamp_buffer.argtypes = [C.c_void_p, C.c_uint]
stamps = torch.zeros(2 * 256 * 64, dtype=torch.int32, device=dev)  # stamps of up to 256 workgroups, then their landing waits
COLD = "cold" in sys.argv[1:]
flush = torch.empty(1 << 30, dtype=torch.uint8, device=dev) if COLD else None
summary = []
_lib.check(lib.hct_debug_set_stamp_buffer(stamps.data_ptr(), stamps.numel()), "stamp buffer")


def call(name, M, N, K, out_f32=False, bias=False, residual=False, act=0, colsum=False):
    a = GemmArgs()
    A = torch.randn(M, K, device=dev).bfloat16(); B = (torch.randn(N, K, device=dev) * 0.05).bfloat16()
    a.A, a.a_dtype, a.lda, a.transA = A.data_ptr(), HCT_BF16, K, 0
    a.B, a.b_dtype, a.ldb, a.transB = B.data_ptr(), HCT_BF16, K, 1
    a.M, a.N, a.K = M, N, K
    Cm = torch.empty(M, N, dtype=torch.float32 if out_f32 else torch.bfloat16, device=dev)
    a.C, a.c_dtype, a.ldc = Cm.data_ptr(), HCT_F32 if out_f32 else HCT_BF16, N
    keep = [A, B, Cm]
    if bias:
        bv = torch.randn(N, device=dev); a.bias = bv.data_ptr(); keep.append(bv)
    if residual:
        r = torch.randn(M, N, device=dev); a.residual = r.data_ptr(); a.ldr = N; keep.append(r)
    if act:
        aux = torch.randn(M, N, device=dev).bfloat16(); a.aux, a.aux_dtype, a.ldaux = aux.data_ptr(), HCT_BF16, N; keep.append(aux)
    a.act = act; a.alpha = 1.0
    if colsum:
        cso = torch.zeros(N, device=dev); a.colsum_out = cso.data_ptr(); keep.append(cso)
    ws = torch.empty(max(16, lib.hct_gemm_workspace_bytes(C.byref(a))), dtype=torch.uint8, device=dev)
    lib.hct_debug_set_gemm_variant(256)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3):
        stamps.zero_()
        if COLD:
            flush.fill_(1)
        e0.record()
        _lib.check(lib.hct_gemm(C.byref(a), ws.data_ptr(), ws.numel(), st), "gemm")
        e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3
    raw = stamps.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    info = _lib.GemmPlanInfo()
    _lib.check(lib.hct_gemm_describe(C.byref(a), 0, ws.numel(), C.byref(info)), "describe")
    tiles, nblk = info.tiles, info.grid
    s = raw[:nblk * 64].reshape(nblk, 16, 4)
    waits = raw[nblk * 64:2 * nblk * 64].reshape(nblk, 64)[:, :16]
    t0 = s[:, 0, 0].min()
    print(f"{name}: M={M} N={N} K={K}: {us:.1f} us, {2.0*M*N*K/us/1e6:.0f} TF, {tiles} tiles on {nblk} WGs")
    print("   tile |  #WG | start(us) min/mean/max | wait-land | main loop | epilogue issue | landing waits |   (all us, mean over WGs)")
    pairs = K // 64
    tot_loop = tot_wait = 0.0
    n_whole = 0
    for i in range(16):
        live = s[:, i, 3] != 0
        if not live.any():
            break
        q = s[live, i, :].astype(np.float64)
        rel = (q[:, 0] - t0) / 100.0
        seg = (q[:, 1:] - q[:, :-1]) / 100.0
        wt = waits[live, i] / 100.0
        print(f"   {i:4d} | {int(live.sum()):4d} | {rel.min():6.1f} {rel.mean():6.1f} {rel.max():6.1f} | {seg[:,0].mean():9.2f} | "
              f"{seg[:,1].mean():9.2f} | {seg[:,2].mean():9.2f} | {wt.mean():9.2f}")
        if not info.sk_tiles or i >= 2:  # whole tiles only (items 0 / 1 of a stream-K launch are K ranges)
            tot_loop += seg[:, 1].sum(); tot_wait += wt.sum(); n_whole += int(live.sum())
    last = s[:, :, 3].max()
    print(f"   kernel span by stamps: {(last - t0)/100.0:.1f} us")
    if n_whole:
        loop, wait = tot_loop / n_whole, tot_wait / n_whole
        print(f"   whole tiles: main loop {loop:.2f} us = {loop / pairs * 1e3:.0f} ns per pair of {pairs}; landing waits {wait:.2f} us = "
              f"{wait / (pairs - 1) * 1e3:.0f} ns per wait, {100 * wait / loop:.0f} % of the main loop")
        summary.append(dict(name=name, M=M, N=N, K=K, cold=COLD, us=round(us, 1), tiles=tiles, grid=nblk, rows_per_tile=64 * info.row_tiles_per_wave,
                            walk_width=info.walk_width, pairs=pairs, main_loop_us=round(loop, 2), ns_per_pair=round(loop / pairs * 1e3),
                            landing_wait_us=round(wait, 2), ns_per_wait=round(wait / (pairs - 1) * 1e3), wait_share=round(wait / loop, 3)))


Md = 256 * 217
which = [w for w in sys.argv[1:] if w != "cold" and not w.startswith("out=") and not w.startswith("walk=")] or ["qkv", "fc1", "dgelu", "proj"]
for w in sys.argv[1:]:
    if w.startswith("walk="):  # tile walk: bands of that many column tiles (79: the plan's bands; default: none)
        lib.hct_debug_set_gemm_variant(-20 - int(w[5:]))
SKOFF = "skoff" in which  # whole tiles only (no stream-K remainder round)
if SKOFF:
    lib.hct_debug_set_gemm_variant(-1000 - (1 << 24))
if "qkv" in which: call("qkv fwd (plain bf16)", Md, 2304, 768)
if "fc1" in which: call("fc1 fwd (GELU, aux, bias)", Md, 3072, 768, bias=True, act=1)
if "dgelu" in which: call("fc2 dgrad (x gelu')", Md, 3072, 768, act=2)
# the forms the training step uses: forward saves gelu' (act 4), the backward multiplies by it and sums columns (act 5)
if "fc1d" in which: call("fc1 fwd (GELU + saved gelu', bias)", Md, 3072, 768, bias=True, act=4)
if "mulaux" in which: call("fc2 dgrad (x saved gelu' + column sums)", Md, 3072, 768, act=5, colsum=True)
if "encmulaux" in which: call("encoder fc2 dgrad (x saved gelu' + column sums)", 256 * 55, 3072, 768, act=5, colsum=True)
if "encproj" in which: call("encoder proj fwd (+bias +res f32)", 256 * 55, 768, 768, out_f32=True, bias=True, residual=True)
if "proj" in which: call("proj fwd (+bias +res f32)", Md, 768, 768, out_f32=True, bias=True, residual=True)
# 651 tiles: with the stream-K remainder round (default; argument skoff switches it off) item 0 / 1 of a workgroup are its
# follower / owner pieces, whose "epilogue issue" column is the slab hand-over / the fix-up + epilogue
if "fc1dgrad" in which: call("fc1 dgrad (plain bf16, K=3072)", Md, 768, 3072)
if "encfc1dgrad" in which: call("encoder fc1 dgrad (plain bf16, K=3072, 165 tiles)", 256 * 55, 768, 3072)
for w in sys.argv[1:]:
    if w.startswith("out="):
        import json
        with open(w[4:], "w") as f:
            json.dump(summary, f, indent=1)
