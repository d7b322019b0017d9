"""CPU: the yardstick of the LayerNorm / RMSNorm kernel tests (tests/norm_ref.py).  The float64 restatements against float64 autograd
through F.layer_norm and through x rsqrt(mean(x^2) + eps) gamma; the fp32 restatements in the kernels' order against the float64 ones,
measured per (family, kind, eps, figure): that measurement, not the kernels, decides which figures take the project's bars and which
take ten times an entry of N.RESTATEMENT; the exact-sum inputs; the loop limits against the source and the case lists against them."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

from tests import norm_ref as N

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _close(a, b, tol):
    return float((a.double() - b.double()).abs().max()) <= tol * (float(b.double().abs().max()) + 1e-300)


# ---- the float64 restatements are the definitions ----------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", N.EPS_VALUES)
@pytest.mark.parametrize("family", N.FAMILIES)
def test_float64_restatement_is_autograd(family, eps):
    """y, mean, rstd; dx with the residual gradient added row by row and through a row map with -1 entries; dgamma, dbeta, colsum."""
    rows, D = 13, 260
    inp, ref = N.fwd_case(family, rows, D, "gauss", eps)
    x, gamma, beta = (inp[k].double().clone().requires_grad_(True) for k in ("x", "gamma", "beta"))
    eps32 = float(torch.tensor(eps, dtype=F32))
    if family == "layernorm":
        y = F.layer_norm(x, (D,), gamma, beta, eps32)
        assert _close(ref["mean"], x.detach().mean(1), 1e-14)
        assert _close(ref["rstd"], (x.detach().var(1, unbiased=False) + eps32).rsqrt(), 1e-14)
    else:
        y = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps32) * gamma
        assert _close(ref["rstd"], torch.rsqrt(x.detach().pow(2).mean(-1) + eps32), 1e-14)
    assert _close(ref["y"], y.detach(), 1e-14)
    (y * inp["dy"].double()).sum().backward()
    stats = dict(dy=inp["dy"], x=inp["x"], gamma=inp["gamma"], rstd_in=ref["rstd"], mean_in=ref.get("mean"))
    m, mc = N.row_map(rows)
    assert int((m < 0).sum()) == rows - mc and sorted(m[m >= 0].tolist()) == list(range(mc)) and m[m >= 0].tolist() != list(range(mc))
    comp = torch.randn(mc, D, generator=N.gen(5), dtype=F64)
    scattered = torch.zeros(rows, D, dtype=F64)
    scattered[m >= 0] = comp[m[m >= 0].long()]
    for dres, rmap, add in ((None, None, 0.0), (inp["dres"], None, inp["dres"].double()), (comp, m, scattered)):
        got = N.bwd(family, stats, dres, rmap)
        want = x.grad + add
        assert _close(got["dx"], want, 1e-13) and _close(got["dcolsum"], want.sum(0), 1e-13)
        assert _close(got["dgamma"], gamma.grad, 1e-13)
        if family == "layernorm":
            assert _close(got["dbeta"], beta.grad, 1e-13)


def test_kernel_order_sums_are_sums():
    """sum_rows_waves(order=True) in float64 is the column sum at every row limit, with the forward's and the backward's wave count."""
    for rows in N.ROW_LIMITS:
        t = torch.randn(rows, 8, generator=N.gen(rows, 3), dtype=F64)
        for waves in (N.BWD_WAVES, N.FWD_WAVES, 8):
            assert _close(N.sum_rows_waves(t, True, waves), t.sum(0), 1e-13)
    # and it is THAT order: with 8 waves, wave 0 takes rows 0 and 8, whose 1e8 cancel before any 1 is added; with 4 it takes rows 0, 4, 8
    # and loses row 4's 1 against the 1e8
    t = torch.tensor([[1e8], [1.0], [1.0], [1.0], [1.0], [1.0], [1.0], [1.0], [-1e8]], dtype=F32)
    assert float(N.sum_rows_waves(t, True, 8)) == 7.0 and float(N.sum_rows_waves(t, True, 4)) == 6.0


# ---- the fp32 restatement in the kernels' order: what decides the bars ---------------------------------------------------------------
@pytest.mark.parametrize("family", N.FAMILIES)
def test_fp32_restatement_decides_the_bars(family):
    """Every (family, kind, eps, figure): within a tenth of the fp32 bar, or recorded in N.RESTATEMENT at the measured value -- and no
    record names a clean kind.  rstd: within N.RSTD_CEILING (see there)."""
    worst = N.measure(family)
    seen = set()
    for k in sorted(worst, key=str):
        e, kind, name = worst[k], k[1], k[3]
        print(k, f"{e:.3e}", N.RESTATEMENT.get(k, ""))
        if name == "rstd":
            assert e <= N.RSTD_CEILING < N.RSTD_BAR / 3 and k not in N.RESTATEMENT, (k, e)
        elif k in N.RESTATEMENT:
            seen.add(k)
            assert e <= N.RESTATEMENT[k] <= 2.0 * e and N.RESTATEMENT[k] > N.FP32_BAR / 10 and kind not in N.CLEAN_KINDS, (k, e)
            assert N.bar(k, N.FP32_BAR) == 10.0 * N.RESTATEMENT[k] and N.bar(k, N.BF16_BAR) == max(N.BF16_BAR, 10.0 * N.RESTATEMENT[k])
        else:
            assert e <= N.FP32_BAR / 10, (k, e)
            assert N.bar(k, N.FP32_BAR) == N.FP32_BAR
    assert seen == {k for k in N.RESTATEMENT if k[0] == family}, "a recorded case is no longer walked"
    assert all(k[1] in ("offset", "const") for k in N.RESTATEMENT)


@pytest.mark.parametrize("family", N.FAMILIES)
def test_fp32_column_sums_hold_their_bounds(family):
    """dgamma, dbeta in fp32 in the kernels' order within (n + roundings) 2^-24 sum|terms| of float64; dcolsum within (n - 1) 2^-24 sum|dx|
    of the float64 sum of the SAME fp32 dx (the GPU file holds the kernel's column sum against the kernel's own dx in this way)."""
    for D, kind in ((260, "gauss"), (772, "offset"), (48, "outlier")):
        rows = N.base_rows(D, kind)
        inp = N.bwd_case(family, rows, D, kind, 1e-6, dict(dydt=BF16, dres="own"))
        got, ref = N.bwd_ref(family, inp, F32, True), N.bwd_ref(family, inp)
        for name, (roundings, mag) in N.sum_terms(family, inp).items():
            err = (got[name].double() - ref[name]).abs()
            assert bool((err <= N.product_sum_bound(rows, roundings, mag)).all()), (D, kind, name)
            assert float(err.max()) > 0.0  # the bound is not met by accident of an exact sum
        err = (got["dcolsum"].double() - got["dx"].double().sum(0)).abs()
        assert bool((err <= N.sum_bound(torch.tensor(rows), got["dx"].double().abs().sum(0))).all()), (D, kind)


# ---- exact sums --------------------------------------------------------------------------------------------------------------------
def _exact(family, inp, scale=1.0):
    """fp32 in the kernels' order == float64, bit for bit, and the same with the rows in another order."""
    ref = N.bwd(family, inp, inp["dres"])
    got = N.bwd(family, inp, inp["dres"], None, F32, True)
    perm = torch.randperm(inp["x"].shape[0], generator=N.gen(11))
    shuffled = {k: (v[perm] if v is not None and v.dim() and v.shape[0] == perm.numel() and k != "gamma" else v) for k, v in inp.items()}
    again = N.bwd(family, shuffled, shuffled["dres"], None, F32, True)
    for k in ref:
        assert torch.equal(got[k].double(), ref[k]), k
        assert torch.equal(again[k].double(), ref[k][perm] if k == "dx" else ref[k]), (k, "row order")
        assert torch.equal(ref[k] * scale, (ref[k] * scale).round()) and float(ref[k].abs().max()) * scale < 2 ** 24, k
    return ref


@pytest.mark.parametrize("family", N.FAMILIES)
def test_int_kind_is_exact_in_any_order(family):
    for D in N.bwd_ds():
        rows = N.base_rows(D, "int")
        inp = N.int_case(family, rows, D)
        a = inp["dy"].double() * inp["gamma"].double()
        assert bool((a.sum(1) == 0).all()) and bool(((a * inp["x"].double()).sum(1) == 0).all())
        assert bool((inp["rstd_in"] == 1).all()) and (family == "rmsnorm" or bool((inp["mean_in"] == 0).all()))
        assert torch.equal(inp["dy"], inp["dy"].to(BF16).float())  # exact in either storage type
        ref = _exact(family, inp)
        assert torch.equal(ref["dx"], a + inp["dres"].double()) and torch.equal(ref["dx"], ref["dx"].to(BF16).double())
        assert float(ref["dgamma"].abs().max()) > 0


@pytest.mark.parametrize("family", N.FAMILIES)
@pytest.mark.parametrize("D", N.INT_MEAN_D)
def test_int_kind_with_row_means_is_exact_in_any_order(family, D):
    """Non-zero mean_d(a) and mean_d(a xhat): integers over D, so every figure is a multiple of 1 / D; sum_r |dx| D < 2^24 per column makes
    every partial sum of every order exact."""
    inp = N.int_case(family, N.BASE_ROWS, D, means=True)
    xh = inp["x"].double() - (inp["mean_in"].double()[:, None] if family == "layernorm" else 0.0)
    a = inp["dy"].double() * inp["gamma"].double()
    assert int((a.sum(1) != 0).sum()) > 400 and int(((a * xh).sum(1) != 0).sum()) > 400
    assert family == "rmsnorm" or int((inp["mean_in"] != 0).sum()) > 300
    ref = _exact(family, inp, scale=float(D))
    assert float(ref["dx"].abs().sum(0).max()) * D < 2 ** 24
    assert not torch.equal(ref["dx"], ref["dx"].round())


def test_forward_mean_of_integer_rows_is_exact():
    for D in (4, 8, 256, 512, 1024):
        inp, ref = N.fwd_case("layernorm", N.base_rows(D, "int"), D, "int", 1e-5)
        assert torch.equal(inp["x"], inp["x"].round())
        assert torch.equal(N.fwd("layernorm", inp, 1e-5, F32, True)["mean"].double(), ref["mean"])


# ---- inputs, loop limits, case lists -------------------------------------------------------------------------------------------------
def test_input_kinds():
    D = 772
    x = {k: N._base(D, k)["x"].double() for k in N.KINDS}
    assert abs(float(x["gauss"].mean()) - 0.3) < 0.02 and abs(float(x["gauss"].std()) - 2.0) < 0.02
    assert abs(float(x["offset"].mean()) - 100.0) < 0.01 and abs(float(x["offset"].std()) - 0.1) < 0.01
    assert bool((x["outlier"][:, D // 3] == N.OUTLIER).all()) and float(x["outlier"].abs().sort(dim=1).values[:, -2].max()) < 6.0
    assert float(x["tiny"].var(1, unbiased=False).max()) < min(N.EPS_VALUES) / 10
    assert bool((x["const"] == x["const"][:, :1]).all()) and float(x["const"][:, 0].std()) > 1.0
    for rows in (1, 5):  # the leading rows of one matrix: what is measured on all of it holds for each part
        assert torch.equal(N.fwd_case("layernorm", rows, D, "gauss", 1e-5)[0]["x"], N._base(D, "gauss")["x"][:rows])
    dy = N._base(4, "gauss")  # D <= SMALL_D: no row of the backward is a cancellation
    kept = N.bwd_case("layernorm", 517, 4, "gauss", 1e-5, dict(dydt=F32, dres=None))
    assert float((N.bwd_ref("layernorm", kept)["dx"].norm(dim=1) * (1 / kept["rstd_in"].double())
                  / (kept["dy"].double() * kept["gamma"].double()).norm(dim=1)).min()) > 0.45 and dy["dy"].shape == (517, 4)


def test_loop_limits_match_the_source():
    src = open(os.path.join(ROOT, "headct_foundation_amd", "csrc", "elementwise.hip")).read()
    """Both families run one kernel family behind one host path (norm_fwd / norm_bwd / launch_norm_bwd), so every limit stands in the
    source once; each family's entry points must reach that one site."""
    def body(head):  # a function's text from its head up to the closing brace in column 0
        text = src[src.index(head):]
        return text[:text.index("\n}\n")]
    assert int(re.search(r"constexpr int kNormBwdBlocks = (\d+);", src).group(1)) * N.ROWS_PER_WG == N.BWD_WAVES
    assert int(re.search(r"constexpr int kNormFwdBlocks = (\d+);", src).group(1)) * N.ROWS_PER_WG == N.FWD_WAVES
    assert len(re.findall(r"const int nblk = min\(\(rows \+ 3\) / 4, (\w+)\);", src)) == 1  # the forward's grid cap: one site ...
    assert "const int nblk = min((rows + 3) / 4, kNormFwdBlocks);" in body("static int norm_fwd(")
    assert len(re.findall(r"const int nblk = min\((\w+), \(rows \+ 3\) / 4\);", src)) == 1  # ... and the backward's
    assert "const int nblk = min(kNormBwdBlocks, (rows + 3) / 4);" in body("static int norm_bwd(")
    assert int(re.search(r"constexpr int kFoldThreads = (\d+);", src).group(1)) == N.FOLD_GROUPS * N.FOLD_COLS
    fold = body("void __launch_bounds__(512) fold_partials_kernel")
    assert f"b0 += {N.FOLD_GROUPS} * {N.FOLD_IN_FLIGHT})" in fold and f"float v[{N.FOLD_IN_FLIGHT}];" in fold
    assert f"threadIdx.x & {N.FOLD_COLS - 1}" in fold and f"i < {N.FOLD_GROUPS}; ++i) v += s_red[i][c]" in fold
    # the chunk expression: four sites in norm_fwd_reg_kernel and three in norm_bwd_kernel, and none with another width
    chunks = re.findall(r"const int d = lane \* 4 \+ (\d+) \* i;", src)
    assert len(chunks) == 7 and all(int(c) == N.CHUNK_COLS for c in chunks)
    assert body("norm_fwd_reg_kernel(const float*").count(f"const int d = lane * 4 + {N.CHUNK_COLS} * i;") == 4
    assert body("norm_bwd_kernel(const T*").count(f"const int d = lane * 4 + {N.CHUNK_COLS} * i;") == 3
    assert src.count("else if (D <= 1024) HCT_NORM_FWD(4);") == 1 and "else if (D <= 1024) HCT_NORM_FWD(4);" in body("static int norm_fwd(")
    assert src.count("case 4: HCT_NORM_CASE(4); break;") == 1 and "case 4: HCT_NORM_CASE(4); break;" in body("static int launch_norm_bwd(")
    assert "HCT_NORM_CASE(5)" not in src and "HCT_NORM_FWD(5)" not in src
    assert body("static int norm_bwd(").count("launch_norm_bwd<RMS, T_, TS_>(") == 1  # the dtype ladder's one way to the NV switch
    # each family's entry points reach the one path: the plain backwards go through the mapped ones
    for family, rms in (("layernorm", "false"), ("rmsnorm", "true")):
        assert f'return norm_fwd<{rms}>("hct_{family}_fwd", ' in body(f"int hct_{family}_fwd(")
        assert f'return norm_bwd<{rms}>("hct_{family}_bwd", ' in body(f"int hct_{family}_bwd_mapped(")
        assert f"return hct_{family}_bwd_mapped(" in body(f"int hct_{family}_bwd(")
    assert "return hct_layernorm_bwd_workspace_bytes(rows, D);" in src[src.index("size_t hct_rmsnorm_bwd_workspace_bytes("):][:200]
    assert "return (size_t)kNormBwdBlocks * 3 * D * sizeof(float);" in body("size_t hct_layernorm_bwd_workspace_bytes(")
    assert N.CHUNK_COLS * N.MAX_NV == 1024 and N.FOLD_TRIP == 128


def test_case_lists_cross_every_limit():
    rows = set(N.ROW_LIMITS)
    assert {1, 3, 4, 5} <= rows  # one workgroup: one wave, three, four, a second workgroup of one
    for blocks in (N.FOLD_GROUPS, N.FOLD_TRIP):  # the fold: a block short of its groups / of a trip, exactly, one over
        assert {4 * (blocks - 1), 4 * blocks, 4 * (blocks + 1)} <= rows
    for waves in (N.BWD_WAVES, N.FWD_WAVES):  # the row loop's second trip: no wave, the last wave not yet, one wave, five waves
        assert {waves, waves + 1, waves + 5} <= rows and rows & {waves - 1, waves - 4}
    assert max(rows) > 2 * N.FWD_WAVES and max(rows) > 4 * N.BWD_WAVES and max(rows) % 4
    for nv in range(1, N.MAX_NV + 1):  # every NV with its last chunk short by a quad, full, and one quad into the next
        lim = N.CHUNK_COLS * nv
        assert {lim - 4, lim} <= set(N.D_LIMITS) and lim + 4 in set(N.D_LIMITS + N.D_FWD_ONLY)
    assert min(N.D_LIMITS) == 4 and all(D > 1024 and D % 4 == 0 for D in N.D_FWD_ONLY) and any(D > 2048 for D in N.D_FWD_ONLY)
    assert 260 in N.ROW_LIMIT_D and any(D < 64 * 4 for D in N.ROW_LIMIT_D)  # the row limits with NV = 2 and with idle lanes
    assert N.BASE_ROWS == max(N.D_LIMIT_ROWS) and N.BASE_ROWS > 4 * N.FOLD_TRIP and N.LONG_ROWS == max(N.ROW_LIMITS)
    combos = [(v["dydt"], v["shdt"]) for v in N.VARIANTS]
    assert {(F32, F32), (F32, BF16), (BF16, F32), (BF16, BF16)} <= set(combos) and any(s is None for _, s in combos)
    assert {v["dres"] for v in N.VARIANTS} == {None, "alias", "own", "mapped"} and {v["colsum"] for v in N.VARIANTS} == {True, False}
    for kinds in (N.KINDS + ("int",),):  # every kind meets both eps values across the variants
        assert {(k, e) for k, e, _ in N.bwd_plan(kinds)} == {(k, e) for k in kinds for e in N.EPS_VALUES}
