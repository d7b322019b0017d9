"""The persistent NT GEMM's operand rings (csrc/gemm.hip, gemm_bf16_nt256_kernel: A requested two stage pairs ahead into a ring of
three pairs, B one pair ahead into a ring of two) through the C ABI, against a float64 product of the bf16-rounded operands computed
on the CPU.  Bounds: those of tests/test_kernels_gpu.py::test_gemm_nt_bf16_mfma (1e-5 for fp32 outputs: exact bf16 products, fp32
accumulation; 4e-3 for bf16 outputs).

K = 128, 192, 256, 320, 768 are 2, 3, 4, 5 and 12 stage pairs: shorter than, equal to and longer than the prefetch depth, so every
combination of "this request exists / does not" at the top and the tail of an item runs.  M = 55, 256, 257 and 14 080 give a single
ragged tile, a full one, a row edge of one row and the encoder's shape, for which the plan picks 192-row tiles (asserted) whose
waves 6 and 7 issue B pieces only.  76 800 x 256 x {128, 192, 320} has more tiles than CUs, so the requests under an epilogue and the
hand-over from item to item run with the shortest item there is (no third pair at the top) and with a third pair in flight; the stream-K case covers follower and owner items.  Every epilogue instance
runs on every shape, three times on the same inputs: the kernel is deterministic, so a race in a ring shows as a difference."""
import ctypes as C

import pytest
import torch

from headct_foundation_amd import _lib
from headct_foundation_amd._lib import HCT_BF16, HCT_F32, GemmArgs, GemmPlanInfo
from tests import gemm_ref as R
from tests.util import rel_err

pytestmark = pytest.mark.gpu

TOL_F32, TOL_BF16 = 1e-5, 4e-3
ACT_GELU_D, ACT_MULAUX = 4, 5  # GELU that saves gelu'(pre-activation) in aux; product x aux


def _args(A, B, M, N, K, out, bias=None, residual=None, act=0, aux=None, colsum=None):
    a = GemmArgs()
    a.M, a.N, a.K = M, N, K
    a.A, a.a_dtype, a.lda, a.transA = A.data_ptr(), HCT_BF16, K, 0
    a.B, a.b_dtype, a.ldb, a.transB = B.data_ptr(), HCT_BF16, K, 1
    a.C, a.c_dtype, a.ldc = out.data_ptr(), HCT_BF16 if out.dtype == torch.bfloat16 else HCT_F32, N
    a.bias = bias.data_ptr() if bias is not None else None
    a.residual = residual.data_ptr() if residual is not None else None
    a.ldr = N
    a.act = act
    if aux is not None:
        a.aux, a.aux_dtype, a.ldaux = aux.data_ptr(), HCT_BF16, N
    a.colsum_out = colsum.data_ptr() if colsum is not None else None
    a.alpha = 1.0
    return a


def _launch(lib, a, ws):
    _lib.check(lib.hct_gemm(C.byref(a), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream), "hct_gemm")


def _plan(lib, a, ws):
    info = GemmPlanInfo()
    _lib.check(lib.hct_gemm_describe(C.byref(a), 0, ws.numel(), C.byref(info)), "hct_gemm_describe")
    return info


def _inputs(M, N, K, dev):
    g = torch.Generator(device="cpu").manual_seed(1000 * K + N + M)
    A = torch.randn(M, K, generator=g).bfloat16()
    B = (torch.randn(N, K, generator=g) * 0.05).bfloat16()
    bias = torch.randn(N, generator=g)
    res = torch.randn(M, N, generator=g)
    dact = torch.randn(M, N, generator=g).bfloat16()  # a saved gelu' for the x gelu' instance
    ref = A.double() @ B.double().t()                 # computed once, shared by the four instances
    # what tests/gemm_ref.py's bound() reads: the product of the absolute operands, and the epilogue inputs under its names
    data = dict(gen="gaussian", P=ref, absP=A.double().abs() @ B.double().abs().t(), bias=bias, res=res, aux=dact)
    return dict(A=A.to(dev), B=B.to(dev), bias=bias.to(dev), res=res.to(dev), dact=dact.to(dev), ref=ref, bias64=bias.double(),
                res64=res.double(), dact64=dact.double(), data=data)


def _run_all_modes(lib, M, N, K, dev, ws, expect_rows=None, expect_sk=False):
    x = _inputs(M, N, K, dev)
    A, B = x["A"], x["B"]
    outs = []
    for rep in range(3):
        o = {}
        o["plain"] = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
        o["res"] = torch.empty(M, N, dtype=torch.float32, device=dev)
        o["gelu"] = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
        o["gelu_d"] = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
        o["mulaux"] = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
        o["cs"] = torch.empty(N, dtype=torch.float32, device=dev)
        calls = [_args(A, B, M, N, K, o["plain"]),
                 _args(A, B, M, N, K, o["res"], bias=x["bias"], residual=x["res"]),
                 _args(A, B, M, N, K, o["gelu"], bias=x["bias"], act=ACT_GELU_D, aux=o["gelu_d"]),
                 _args(A, B, M, N, K, o["mulaux"], act=ACT_MULAUX, aux=x["dact"], colsum=o["cs"])]
        for i, a in enumerate(calls):
            if rep == 0:
                p = _plan(lib, a, ws)
                assert p.kernel == 2, "not the persistent NT kernel"  # HCT_GEMM_NT256
                assert p.epilogue_mode == (1, 2, 3, 4)[i] and (i != 3 or p.fuse_colsum)
                if expect_rows is not None and i < 2:
                    assert 64 * p.row_tiles_per_wave == expect_rows
                if expect_sk:
                    assert p.sk_tiles > 0, "the plan does not share this shape's remainder out"
            _launch(lib, a, ws)
        torch.cuda.synchronize()
        outs.append(o)
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[1][k]) and torch.equal(outs[0][k], outs[2][k]), f"{k}: launches differ"
    o = outs[0]
    pre = x["ref"] + x["bias64"]
    gelu = torch.nn.functional.gelu(pre)
    pr = pre.clone().requires_grad_(True)
    torch.nn.functional.gelu(pr).sum().backward()
    mul = x["ref"] * x["dact64"]
    errs = {"plain": rel_err(o["plain"], x["ref"]), "res": rel_err(o["res"], pre + x["res64"]), "gelu": rel_err(o["gelu"], gelu),
            "gelu_d": rel_err(o["gelu_d"], pr.grad), "mulaux": rel_err(o["mulaux"], mul), "cs": rel_err(o["cs"], mul.sum(0))}
    print(f"M={M} N={N} K={K}: " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    assert errs["res"] < TOL_F32
    for k in ("plain", "gelu", "gelu_d", "mulaux"):
        assert errs[k] < TOL_BF16, k
    assert errs["cs"] < 1e-4  # (the bound of test_gemm_nt_stream_k_remainder's column sums: fp32 sums of up to 76 800 fp32 products)
    # element by element against the derived bound of tests/gemm_ref.py (the global ratios above cannot see a few wrong elements)
    nt = dict(M=M, N=N, K=K, kernel=R.NT256)
    cases = {"plain": R.Case(name="plain", mode=1, **nt), "res": R.Case(name="res", mode=2, c_dtype=R.F32, bias=True, residual=True, **nt),
             "gelu": R.Case(name="gelu_d", mode=3, act=R.GELU_D, bias=True, aux_dtype=R.BF16, **nt),
             "mulaux": R.Case(name="mulaux", mode=4, act=R.MULAUX, aux_dtype=R.BF16, colsum=True, fuse=True, **nt)}
    ratios = {}
    for k, case in cases.items():
        ex = R.exact(case, x["data"])
        allow = R.bound(case, x["data"], ex)
        ratios[k] = R.worst(o[k].double().cpu(), ex["C"], allow["C"])
        if k == "gelu":
            ratios["gelu_d"] = R.worst(o["gelu_d"].double().cpu(), ex["aux"], allow["aux"])
        if k == "mulaux":
            ratios["cs"] = R.worst(o["cs"].double().cpu()[None], ex["colsum"][None], allow["colsum"][None])
    print("   |err| / bound: " + " ".join(f"{k}={v[0]:.3f}" for k, v in ratios.items()))
    for k, (ratio, row, col) in ratios.items():
        assert ratio <= 1.0, f"{k}: |err| / bound = {ratio:.3f} at ({row}, {col})"


@pytest.fixture(scope="module")
def ws(lib, cuda):
    w = torch.zeros(76800 // 256 * 4 * 768 * 4 + (1 << 20) + lib.hct_gemm_nt_stream_k_bytes() + 4096, dtype=torch.uint8, device=cuda)
    return w


@pytest.mark.parametrize("K", [128, 192, 256, 320, 768])
@pytest.mark.parametrize("N", [256, 768])
@pytest.mark.parametrize("M", [55, 256, 257, 14080])
def test_ring_depths_and_row_edges(lib, cuda, ws, M, N, K):
    # 14 080 rows: fewer 256-row tiles than CUs and no more 192-row tiles than CUs -> 192-row tiles for the plain / +residual instances
    _run_all_modes(lib, M, N, K, cuda, ws, expect_rows=192 if M == 14080 else None)


@pytest.mark.parametrize("K", [128, 192, 320])  # 2 pairs: no third pair at the top of an item; 3 and 5: a third pair in flight behind the epilogue
def test_more_tiles_than_cus_hands_over_between_items(lib, cuda, ws, K):
    _run_all_modes(lib, 76800, 256, K, cuda, ws, expect_rows=256)


def test_stream_k_follower_and_owner_items(lib, cuda, ws):
    """The smallest shape of a short list whose remainder round the plan shares out by K range."""
    pick = None
    dummy = torch.empty(16, dtype=torch.bfloat16, device=cuda)
    for M, N, K in ((2048, 256, 1024), (2048, 256, 1536), (2048, 256, 2048), (4096, 256, 3072)):
        if _plan(lib, _args(dummy, dummy, M, N, K, dummy), ws).sk_tiles > 0:
            pick = (M, N, K)
            break
    assert pick is not None, "no candidate shape splits"
    off = lib.hct_gemm_nt_flags_offset(ws.numel())
    flags = ws[off:off + 4096].view(torch.int32)
    flags.zero_()
    _run_all_modes(lib, *pick, cuda, ws, expect_sk=True)
    assert int((flags[:256] != 0).sum()) > 0, "stream-K did not engage"
    assert int(flags[512]) == 0, "a partial never arrived"
