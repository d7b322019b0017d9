"""Pins tests/attn_head_ref.py before tests/test_attn_head_kernels_gpu.py uses it as a yardstick: every restatement against torch's own
function or autograd in float64 (the module-level formula of AttentionClassifier: F.scaled_dot_product_attention with scale = 1 on
pre-scaled queries, F.linear of the mean over the queries of an eval-mode batch norm); the restatements' own fp32 error, with every
reduction in the kernel's order, against the bars of the GPU file on every GPU case's inputs; and the stated properties of the case
lists (sizes past the loop limits they are there to cross) and of the inputs.  No GPU, no library."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import attn_head_ref as R
from tests import head_kernels_ref as H

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16


def _close(a, b, tol=1e-12):
    return H.rel(a, b) <= tol


def _randn(*shape, seed=0):
    return torch.randn(*shape, generator=H.gen(seed, *shape), dtype=F64)


# ---- against torch, float64 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,Hh,Q,dh", [(2, 5, 3, 1, 4), (2, 65, 3, 5, 72), (5, 217, 2, 4, 128)])
def test_query_attention_is_sdpa_and_its_autograd(B, N, Hh, Q, dh):
    ls = H.f32_scalar(dh ** -0.5)
    q, kv, dout = (_randn(Q, Hh * dh, seed=1).requires_grad_(True), _randn(B, N, 2, Hh, dh, seed=2).requires_grad_(True), _randn(B, Hh, Q, dh, seed=3))
    qs = (q * ls).reshape(1, Q, Hh, dh).permute(0, 2, 1, 3).expand(B, Hh, Q, dh)   # pre-scaled queries, scale = 1
    k, v = kv[:, :, 0].permute(0, 2, 1, 3), kv[:, :, 1].permute(0, 2, 1, 3)
    want = F.scaled_dot_product_attention(qs, k, v, scale=1.0)
    (want * dout).sum().backward()
    for order in (False, True):
        out, lse = R.query_attention(q.detach(), kv.detach(), ls, order)
        assert _close(out, want) and _close(lse, torch.logsumexp(R.logits(q.detach(), kv.detach(), ls), dim=-1))
        res = R.query_attention_bwd(q.detach(), kv.detach(), ls, out, lse, dout, order)
        assert _close(res["dk"], kv.grad[:, :, 0]) and _close(res["dv"], kv.grad[:, :, 1]) and _close(res["dq"], q.grad)
        assert bool((res["dk_mag"] >= res["dk"].abs() * (1 - 1e-12)).all()) and bool((res["dq_mag"] >= res["dq"].abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize("nq", R.HL_NQ)
@pytest.mark.parametrize("D", [1, 65, 768])
def test_head_linear_is_linear_of_the_mean_of_an_eval_batchnorm(D, nq):
    rows, n_out = 5, 3
    x, W, b, dl = _randn(rows, nq, D, seed=4), _randn(n_out, D, seed=5).requires_grad_(True), _randn(n_out, seed=6).requires_grad_(True), _randn(rows, n_out, seed=7)
    mean, var = _randn(D, seed=8), _randn(D, seed=9).abs() + 0.5
    for stats in (True, False):
        W.grad = b.grad = None
        xn = F.batch_norm(x.reshape(-1, D), mean, var, training=False, eps=R.EPS).reshape(rows, nq, D) if stats else x
        want = F.linear(xn.mean(dim=1), W, b)
        (want * dl).sum().backward()
        m, v = (mean, var) if stats else (None, None)
        for order in (False, True):
            assert _close(R.head_linear(x, m, v, R.EPS, W.detach(), b.detach(), False, order), want)
            assert _close(R.head_linear(x, m, v, R.EPS, W.detach(), b.detach(), True, order), want.tanh())
            dW, db = R.head_linear_wgrad(x, m, v, R.EPS, dl, order)
            assert _close(dW, W.grad) and _close(db, b.grad)
    assert _close(R.head_linear(x, None, None, R.EPS, W.detach(), None), x.mean(1) @ W.detach().t())
    assert _close(R.channel_norm(x[:, 0], mean, var, R.EPS), F.batch_norm(x[:, 0], mean, var, training=False, eps=R.EPS))


def test_copy_passes():
    x = _randn(300, 260, seed=10)
    assert _close(R.colsum(x, True), x.sum(0), 1e-14) and torch.equal(R.colsum(x), x.sum(0))
    ints = H.values((R.colsum_rows(4)[2], 4), "int", H.gen(11))
    assert torch.equal(R.colsum(ints, True), ints.sum(0))
    assert torch.equal(R.transpose_cast(x.float(), BF16), x.float().to(BF16).t()) and torch.equal(R.cast(x.float(), BF16), x.float().to(BF16))
    src, idx = torch.arange(12, dtype=torch.int32).reshape(4, 3), torch.tensor([3, -1, 0, 3], dtype=torch.int32)
    assert R.gather_rows(src, idx).tolist() == [[9, 10, 11], [0, 0, 0], [0, 1, 2], [9, 10, 11]]
    assert float(R.fma(torch.tensor(1.0 + 2.0 ** -12), torch.tensor(1.0 + 2.0 ** -12), torch.tensor(-1.0))) == 2.0 ** -11 + 2.0 ** -24  # one rounding


def test_colsum_chunks_is_the_plan_rule():
    """The rule of csrc/gemm_plan.h, restated: read from the header so that a change there is noticed here."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(__file__), "..", "headct_foundation_amd", "csrc", "gemm_plan.h")).read()
    body = re.search(r"inline int colsum_chunks\(int rows, int cols\) \{(.*?)\n\}", src, re.S).group(1)
    assert "(cols + 255) / 256" in body and "(1024 + colblk - 1) / colblk" in body and "(rows + 15) / 16" in body
    assert [R.colsum_chunks(r, c) for r, c in ((1, 4), (16, 4), (17, 4), (29, 260), (10 ** 6, 256), (10 ** 6, 260))] == [1, 1, 2, 2, 1024, 512]


# ---- the geometry: every case list is past the loop limit it is there to cross ----------------------------------------------------
def test_geometry_and_loop_limits():
    assert (R.LANES, R.WAVES, R.LDS_FLOATS, R.MAX_DH, R.CAST_TRIP, R.CAST_BLOCKS, R.GATHER_BLOCKS, R.GATHER_THREADS) == (64, 4, 64 * 1024 // 4, 128, 256 * 4, 2048, 8192, 256)
    Ns, Qs, dhs = set(R.ATTN_N), set(R.ATTN_Q), set(R.ATTN_DH)
    assert Ns == {n for n, _, _ in R.ATTN_CASES} and Qs == {q for _, q, _ in R.ATTN_CASES} and dhs == {d for _, _, d in R.ATTN_CASES}
    assert min(Ns) < R.WAVES and R.WAVES in Ns and R.WAVES + 1 in Ns and R.LANES in Ns and R.LANES + 1 in Ns and any(n > 3 * R.LANES and n % R.LANES for n in Ns)
    assert min(Qs) < R.WAVES and R.WAVES in Qs and R.WAVES + 1 in Qs
    assert any(d < R.LANES and d % 16 == 0 and d > 32 for d in dhs) and R.LANES in dhs and any(R.LANES < d < R.MAX_DH for d in dhs) and R.MAX_DH in dhs
    assert all(any(d > R.LANES and n == N for n, _, d in R.ATTN_CASES) for N in Ns)   # the second lane slot at every N
    assert R.ATTN_PEAKED_CASE in R.ATTN_CASES and R.ATTN_BATCH_CASE in R.ATTN_CASES and set(R.ATTN_BATCHES) == {1, 2, 5} and R.ATTN_BATCH_CASE[2] > R.LANES
    assert R.ATTN_H % 2 == 1 and set(R.ATTN_CHAINED_N) <= Ns
    for Q, dh, N in R.ATTN_LDS_CASES:
        assert Q * N + 4 * Q * dh + Q == R.LDS_FLOATS
    assert 6 * 22 * 128 + 2 * 22 > R.LDS_FLOATS >= 6 * 21 * 128 + 2 * 21
    # head_linear: a wave per output, four to a block; 64 lanes
    assert {r * c for r, c in R.HL_OUT} == {1, 3, 4, 5, 13} and {c for _, c in R.HL_OUT} == {1, 2, 5}
    assert {1, R.LANES - 1, R.LANES, R.LANES + 1} <= set(R.HL_D) and max(R.HL_D) == 768
    assert any(c * D > R.WGRAD_BLOCK and c * D % R.WGRAD_BLOCK for _, D, c in R.HL_BWD_CASES) and {D for _, D, _ in R.HL_BWD_CASES} >= set(R.HL_D)
    assert {(s, b) for s, b, _ in R.HL_VARIANTS} == {(True, True), (False, False), (True, False), (False, True)} and {t for _, _, t in R.HL_VARIANTS} == {True, False}
    # channel_norm: 256 quads per block
    quads = [r * C // 4 for r, C in R.CN_CASES]
    assert all(C % 4 == 0 for _, C in R.CN_CASES) and min(quads) == 1 and sum(q > 256 and q % 256 for q in quads) >= 3 and R.CN_REFUSED_C % 4
    # the copy passes
    assert max(R.CAST_N) > R.CAST_BLOCKS * R.CAST_TRIP and max(R.CAST_N) % 4 and {1, 3, 4, 5, R.CAST_TRIP - 1, R.CAST_TRIP + 1} <= set(R.CAST_N)
    assert len(set(R.DTYPE_PAIRS)) == 4
    assert (R.TILE, R.TILE) in R.TRANSPOSE_CASES and (R.TILE - 1, R.TILE + 1) in R.TRANSPOSE_CASES and any(r > 4 * R.TILE and c > 2 * R.TILE for r, c in R.TRANSPOSE_CASES)
    for cols in R.COLSUM_COLS_LIST:
        one, two, deep = R.colsum_rows(cols)
        chunks = [R.colsum_chunks(r, cols) for r in (one, two, deep)]
        assert chunks[0] == 1 and chunks[1] == 2 and two % 2 and chunks[2] > R.FOLD_GROUPS * 8   # a second trip of the fold's loop, too
        rpc = -(-deep // chunks[2])
        assert rpc > R.COLSUM_TRIP and deep % rpc and (chunks[2] - 1) * rpc < deep
    assert set(R.COLSUM_COLS_LIST) == {4, R.COLSUM_COLS, R.COLSUM_COLS + 4}
    n_rows, row_bytes = R.GATHER_BIG
    pieces = n_rows * row_bytes // 16
    assert R.GATHER_BLOCKS * R.GATHER_THREADS < pieces < R.GATHER_BLOCKS * R.GATHER_THREADS + row_bytes // 16 and n_rows * row_bytes < 34 * 2 ** 20
    assert all(b % 16 == 0 for b in R.GATHER_ROW_BYTES) and R.GATHER_REFUSED_BYTES % 16


# ---- the inputs ---------------------------------------------------------------------------------------------------------------------
def test_attention_inputs():
    N, Q, dh = R.ATTN_PEAKED_CASE
    for dt in (F32, BF16):
        inp = R.attn_inputs(R.ATTN_B, N, R.ATTN_H, Q, dh, "peaked", dt)
        s = R.logits(inp["q"].double(), inp["kv"].double(), inp["ls"])
        assert inp["kv"].dtype == dt and 20.0 < float(s.abs().max()) < 25.0
        assert 20.0 * 2.0 ** -22 < R.exponent_allowance(inp["q"], inp["kv"], inp["ls"]) < 50.0 * 2.0 ** -22
        mod = R.attn_inputs(R.ATTN_B, N, R.ATTN_H, Q, dh, "moderate", dt)
        assert float(R.logits(mod["q"].double(), mod["kv"].double(), mod["ls"]).abs().max()) < 6.0 and mod["ls"] == H.f32_scalar(dh ** -0.5)
    log2e = torch.tensor(1.4426950408889634, dtype=F32)
    for N in R.ATTN_EQUAL_KEY_N:
        inp = R.attn_equal_key_inputs(N, BF16)
        assert torch.equal(inp["kv"].float().to(BF16), inp["kv"]) and bool((inp["kv"][:, :, 0] == inp["kv"][:, :1, 0]).all())
        assert bool((R.logits(inp["q"], inp["kv"].float(), inp["ls"]) == 0).all()) and N & (N - 1) == 0
        out, lse = R.query_attention(inp["q"].double(), inp["kv"].double(), inp["ls"])
        assert _close(out[:, :, 0], inp["kv"].double()[:, :, 1].mean(1)) and _close(lse, torch.full_like(lse, math.log(N)))
        # the kernel's p: the hardware exp2 of fp32(-lse) fp32(log2 e) rounded to fp32, which is the integer -log2 N: p = 1 / N exactly
        assert float(-lse.float().flatten()[0] * log2e) == -math.log2(N)
        res = R.query_attention_bwd(inp["q"].double(), inp["kv"].double(), inp["ls"], out, lse, inp["dout"].double(), order=True)
        assert _close(res["dv"], (inp["dout"].double()[:, :, 0] / N)[:, None].expand(-1, N, -1, -1), 1e-14)


def test_head_and_copy_inputs():
    for nq in R.HL_NQ:
        inp = R.hl_inputs(13, 65, 5, nq, "int")
        v = R._mean_q(inp["x"], None, None, R.EPS)
        assert torch.equal(v, v.round()) and torch.equal(inp["x"].to(BF16).float(), inp["x"]) and bool((v[-1] != 0).any()) and bool((v[:, -1] != 0).any())
        dW, db = R.head_linear_wgrad(inp["x"], None, None, R.EPS, inp["dlogits"], order=True)
        assert torch.equal(dW.double(), inp["dlogits"].double().t() @ v.double()) and torch.equal(db, inp["dlogits"].sum(0))
        nrm = R.hl_inputs(13, 768, 5, nq)
        out = R.head_linear(nrm["x"].double(), None, None, R.EPS, nrm["W"].double(), None)
        assert 0.1 < float(out.abs().min()) and float(out.abs().max()) < 3.5   # tanh still moves, and no output is a cancelled sum
    x = R.cast_values(R.CAST_N[-1], F32, 1)
    assert float(x[2]) == 1.0 + 2.0 ** -8 and float(x[2].to(BF16)) == 1.0 and float(x[3].to(BF16)) == 1.0 + 2.0 ** -6 and bool(torch.isfinite(x).all())
    assert R.cast_values(1, F32, 1).shape == (1,) and R.cast_values(3, BF16, 1).dtype == BF16
    idx = R.gather_index(37, 11, 2)
    assert int(idx[0]) == -1 and int(idx[-1]) == -1 and int(idx[1]) == int(idx[2]) == 10 and int(idx.max()) == 10 and int((idx >= 0).sum()) > 20


# ---- the restatements' own fp32 error, on every GPU case's inputs -------------------------------------------------------------------
def _tenth_or_recorded(figs, seen):
    for k, (e, _, default) in figs.items():
        if k in R.RESTATEMENT:
            seen.add(k)
            assert e <= R.RESTATEMENT[k] <= 2.0 * e and R.RESTATEMENT[k] > default / 10, (k, e, R.RESTATEMENT[k])
        else:
            assert e <= default / 10, (k, e, default)


@pytest.mark.parametrize("Q,dh", R.ATTN_GROUPS)
def test_fp32_attention_restatement_holds_a_tenth_of_the_bars(Q, dh):
    """Every reduction in the kernel's order, in fp32 (with torch's exact exponential), against float64: each figure within a tenth of the
    bar that the GPU file holds it to, or recorded in R.RESTATEMENT (then ten times the record is the GPU bar)."""
    seen = set()
    for key, inp, var in R.attn_runs(Q, dh):
        figs = R.attn_errors(key, dict(var, allowance=0.0), R.attn_ref(inp, var, F32, True), R.attn_ref(inp, var))
        print(key, {k[-1]: f"{e:.2e}" for k, (e, _, _) in figs.items()})
        _tenth_or_recorded(figs, seen)
    assert seen == {k for k in R.RESTATEMENT if k[0] == "query_attention" and k[3:5] == (Q, dh) and k[1] > 1}, "a recorded case is no longer walked"


def test_fp32_attention_restatement_at_the_lds_boundary():
    seen = set()
    for key, inp, var in R.attn_lds_runs():
        figs = R.attn_errors(key, var, R.attn_ref(inp, var, F32, True, bwd=False), R.attn_ref(inp, var, bwd=False))
        print(key, {k[-1]: f"{e:.2e}" for k, (e, _, _) in figs.items()})
        _tenth_or_recorded(figs, seen)
    assert seen == {k for k in R.RESTATEMENT if k[0] == "query_attention" and k[1] == 1 and (k[3], k[4], k[2]) in R.ATTN_LDS_CASES}


@pytest.mark.parametrize("D", R.HL_D)
def test_fp32_head_linear_restatement_holds_a_tenth_of_the_bars(D):
    seen = set()
    for key, inp, var in R.hl_runs(D):
        e, b, default = R.hl_error(key, var, R.hl_ref(inp, var, F32, True), R.hl_ref(inp, var))
        _tenth_or_recorded({key + ("out",): (e, b, default)}, seen)
    assert seen == {k for k in R.RESTATEMENT if k[0] == "head_linear" and k[2] == D}, "a recorded case is no longer walked"
    for B, D_, n_out in R.HL_BWD_CASES:
        if D_ != D and not (D == 65 and D_ == 130):
            continue
        for key, inp, var in R.hl_bwd_runs(B, D_, n_out):
            (bW, bb), exact = R.hl_bwd_limits(inp, var)
            lo, hi = R.hl_bwd_ref(inp, var, F32, True), R.hl_bwd_ref(inp, var)
            for g, r, bound in zip(lo, hi, (bW, bb)):
                if exact:
                    assert torch.equal(g.double(), r), key
                else:
                    assert bool(((g.double() - r).abs() <= bound).all()), (key, float(((g.double() - r).abs() - bound).max()))


def test_fp32_channel_norm_and_colsum_restatements():
    for rows, C in R.CN_CASES:
        for key, inp, var in R.cn_runs(rows, C):
            e = H.worst_row(H.norm_ref(inp, var, F32)["out"], H.norm_ref(inp, var)["out"])
            assert e <= H.FP32_BAR / 10, (key, e)
    for cols in R.COLSUM_COLS_LIST:
        for rows in R.colsum_rows(cols):
            for kind in ("int", "normal"):
                x = H.values((rows, cols), kind, H.gen(rows, cols, 44))
                lo, hi = R.colsum(x, True), x.double().sum(0)
                if kind == "int":
                    assert torch.equal(lo.double(), hi)
                else:
                    assert bool(((lo.double() - hi).abs() <= H.sum_bound(torch.tensor(rows), x.double().abs().sum(0))).all())
