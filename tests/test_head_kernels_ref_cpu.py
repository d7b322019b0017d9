"""Pins tests/head_kernels_ref.py before tests/test_head_kernels_gpu.py uses it as a yardstick: every restatement against torch's own
module or function and against the DINO oracle, forwards and under autograd, in float64; the restatements' own fp32 error, with every
reduction in the kernel's order, against the bars of the GPU file on every GPU case's inputs; and the stated properties of those
inputs (sizes past the loop limits they are there to cross, exact integer sums).  No GPU, no library."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import dino_oracle as DO
from tests import head_kernels_ref as H

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16


def _close(a, b, tol=1e-12):
    return H.rel(a, b) <= tol


def _randn(*shape, seed=0):
    return torch.randn(*shape, generator=H.gen(seed, *shape), dtype=F64)


# ---- against torch and the oracle, float64 ------------------------------------------------------------------------------------------
def test_l2norm_is_f_normalize():
    z, dzn = _randn(5, 260, seed=1).requires_grad_(True), _randn(5, 260, seed=2)
    zn, inv = H.l2norm(z.detach())
    want = F.normalize(z, dim=-1, p=2)
    (want * dzn).sum().backward()
    assert _close(zn, want) and _close(inv, 1.0 / z.detach().norm(dim=1)) and _close(H.l2norm_bwd(dzn, zn, inv), z.grad)
    zn0, inv0 = H.l2norm(torch.zeros(1, 8, dtype=F64))
    assert bool((zn0 == 0).all()) and float(inv0) == 1e12 and torch.equal(zn0, F.normalize(torch.zeros(1, 8, dtype=F64), dim=-1))
    assert _close(H.l2norm(z.detach(), order=True)[0], want, 1e-14)  # the kernel's order is the same sum


def test_weight_norm_is_torch_weight_norm():
    lin = torch.nn.utils.weight_norm(nn.Linear(260, 6, bias=False).double())
    with torch.no_grad():
        lin.weight_g.copy_(_randn(6, 1, seed=3).abs() + 0.5)
        lin.weight_v.copy_(_randn(6, 260, seed=4))
    x, dy = _randn(3, 260, seed=5), _randn(3, 6, seed=6)
    (lin(x) * dy).sum().backward()
    v, g = lin.weight_v.detach(), lin.weight_g.detach()[:, 0]
    w, inv = H.weight_norm(v, g)
    assert _close(w, lin.weight.detach()) and _close(x @ w.t(), lin(x))
    dv, dg = H.weight_norm_bwd(dy.t() @ x, v, g, inv)
    assert _close(dv, lin.weight_v.grad) and _close(dg, lin.weight_g.grad[:, 0])


@pytest.mark.parametrize("affine", [True, False])
def test_batchnorm_is_nn_batchnorm1d(affine):
    M, D, eps = 10, 48, 1e-5
    bn = nn.BatchNorm1d(D, eps=eps, affine=affine).double().train()
    gamma, beta = torch.ones(D, dtype=F64), torch.zeros(D, dtype=F64)
    with torch.no_grad():
        bn.running_mean.copy_(_randn(D, seed=7))
        bn.running_var.copy_(_randn(D, seed=8).abs() + 0.5)
        if affine:
            bn.weight.copy_(_randn(D, seed=9))
            bn.bias.copy_(_randn(D, seed=10))
            gamma, beta = bn.weight.detach().clone(), bn.bias.detach().clone()
    running = (bn.running_mean.clone(), bn.running_var.clone())
    u, dh = (_randn(M, D, seed=11) * 2.0 + 0.5).requires_grad_(True), _randn(M, D, seed=12)
    y = bn(u)
    h = nn.GELU()(y)
    (h * dh).sum().backward()
    mean, var, rmean, rvar = H.bn_stats(u.detach(), 0.1, running)
    assert _close(rmean, bn.running_mean) and _close(rvar, bn.running_var)  # after one step, with the unbiased variance
    m2, v2, rm2, rv2 = H.bn_stats(u.detach(), 0.1, None)
    assert torch.equal(m2, mean) and torch.equal(v2, var) and rm2 is None and rv2 is None
    for chunk in (None, 4, 3):  # the chunked Chan fold is the same statistic
        mc, vc, _, _ = H.bn_stats(u.detach(), 0.1, running, order=True, chunk=chunk)
        assert _close(mc, mean) and _close(vc, var)
    hh, xhat, dact = H.bn_gelu(u.detach(), mean, var, gamma, beta, eps)
    assert _close(hh, h) and _close(gamma * H.bn_norm(u.detach(), mean, var, eps) + beta, y) and _close(xhat, H.bn_norm(u.detach(), mean, var, eps))
    yy = y.detach().clone().requires_grad_(True)
    nn.GELU()(yy).sum().backward()
    assert _close(dact, yy.grad)  # exact-erf GELU'
    sums, du = H.bn_gelu_bwd(dh, dact, xhat, gamma, var, eps, M)
    assert _close(du, u.grad)
    if affine:
        assert _close(sums[0], bn.bias.grad) and _close(sums[1], bn.weight.grad)
    else:  # the classifier heads' BatchNorm1d(affine=False): the input backward with a given g
        assert _close(H.bn_bwd_input(u.detach(), mean, var, eps, g=dh * dact), u.grad)
        assert _close(H.bn_bwd_input(u.detach(), mean, var, eps, g=dh * dact, order=True), u.grad)
    o_running = [r.clone() for r in running]
    assert _close(DO.batchnorm_train(u.detach(), gamma, beta, o_running[0], o_running[1], 0.1, eps), y)
    assert _close(o_running[0], rmean) and _close(o_running[1], rvar)


@pytest.mark.parametrize("nq,ncls", H.BWD_FUSED)
def test_fused_bn_bwd_input_is_autograd_through_the_linear(nq, ncls):
    """Linear(mean over nq consecutive rows of BatchNorm1d(affine=False)(x)): d / dx with g never materialised by the caller."""
    Bq, D = 4, 7
    bn, lin = nn.BatchNorm1d(D, affine=False).double().train(), nn.Linear(D, ncls).double()
    x, dl = (_randn(Bq * nq, D, seed=13) + 1.0).requires_grad_(True), _randn(Bq, ncls, seed=14)
    (lin(bn(x).reshape(Bq, nq, D).mean(dim=1)) * dl).sum().backward()
    mean, var, _, _ = H.bn_stats(x.detach())
    assert _close(H.bn_bwd_input(x.detach(), mean, var, bn.eps, dlogits=dl, W=lin.weight.detach(), nq=nq), x.grad)


def test_softmax_xent_is_nn_cross_entropy():
    inp = H.xent_inputs(257, 5)
    logits = inp["logits"].double().requires_grad_(True)
    loss = nn.CrossEntropyLoss()(logits, inp["target"])
    (3.0 * loss).backward()
    r_loss, r_dl = H.softmax_xent(logits.detach(), inp["target"], 3.0)
    assert _close(r_loss, loss) and _close(r_dl, logits.grad)
    o_loss, o_dl = H.softmax_xent(logits.detach(), inp["target"], 3.0, order=True)
    assert _close(o_loss, loss) and _close(o_dl, logits.grad)
    bad = inp["target"].clone()
    bad[3], bad[256] = -1, 5
    b_loss, b_dl = H.softmax_xent(logits.detach(), bad, 3.0)
    keep = torch.ones(257, dtype=torch.bool)
    keep[3] = keep[256] = False
    assert bool(torch.isnan(b_loss)) and torch.equal(b_dl[keep], r_dl[keep]) and bool(torch.isfinite(b_dl).all())


@pytest.mark.parametrize("nseg,total", H.CLIP_CASES)
def test_clip_total_norm_is_clip_grad_norm(nseg, total):
    """Parameters whose gradient norms are `norms`: the flat buffer is scaled as clip_grad_norm_ scales them."""
    g = H.gen(nseg, total, 31)
    sizes = [total // nseg] * (nseg - 1) + [total - (total // nseg) * (nseg - 1)]
    params = [nn.Parameter(torch.zeros(n, dtype=F64)) for n in sizes]
    for p in params:
        p.grad = torch.randn(p.shape, generator=g, dtype=F64)
    flat, norms = torch.cat([p.grad for p in params]).clone(), torch.stack([p.grad.norm() for p in params])
    for factor in (0.5, 2.0):
        for p, chunk in zip(params, flat.split(sizes)):
            p.grad = chunk.clone()
        max_norm = float(norms.norm()) * factor
        want = torch.nn.utils.clip_grad_norm_(params, max_norm)
        total_norm, coef, scaled = H.clip_total_norm(flat, norms, max_norm)
        assert _close(total_norm, want) and _close(scaled, torch.cat([p.grad for p in params]))
        assert (float(coef) == 1.0) == (factor > 1.0) and (factor < 1.0 or torch.equal(scaled, flat))


@pytest.mark.parametrize("V,B,K", [(2, 1, 4), (3, 3, 1000), (10, 3, 1028)])
def test_dino_loss_is_the_oracle(V, B, K):
    for kind in H.DINO_KINDS:
        inp = H.dino_inputs(V, B, K, kind, F32)
        student, teacher, center = inp["student"].double().requires_grad_(True), inp["teacher"].double(), inp["center"].double()
        want = DO.dino_loss(student, teacher, center, V, 0.1, 0.04)
        (3.0 * want).backward()
        loss, dstudent, csum = H.dino_loss(student.detach(), teacher, center, V, 0.1, 0.04, 3.0)
        assert _close(loss, want) and _close(dstudent, student.grad, 1e-10) and _close(csum, teacher.sum(0))
        o_loss, o_ds, o_csum = H.dino_loss(student.detach(), teacher, center, V, 0.1, 0.04, 3.0, order=True)
        assert _close(o_loss, want) and _close(o_ds, student.grad, 1e-10) and _close(o_csum, teacher.sum(0))
        # the centre: float64 against the oracle, and the fp32 sequence bit for bit
        assert _close(H.center_update(center, csum, 0.9, 2 * B), DO.update_center(center, teacher, 0.9)[0])
        t32 = inp["teacher"]
        assert torch.equal(H.center_update(inp["center"], torch.sum(t32, dim=0), 0.9, 2 * B), DO.update_center(inp["center"], t32, 0.9)[0])


def test_kernel_order_sums_are_sums():
    t = _randn(3, 1029, seed=15)
    for f in (H.sum_wave, H.sum_block):
        assert _close(f(t, True), t.sum(-1), 1e-14)
    assert _close(H.sum_strided(t[0], True), t[0].sum(), 1e-14)
    for f in (H.sum_rows, H.sum_row_chunks):
        assert _close(f(_randn(300, 5, seed=16), True), _randn(300, 5, seed=16).sum(0), 1e-14)
    ints = H.values((3, 1028), "int", H.gen(17))
    assert torch.equal(H.sum_wave(ints, True), ints.sum(-1)) and torch.equal(H.sum_block(ints, True), ints.sum(-1))


# ---- the restatements' own fp32 error, on every GPU case's inputs -------------------------------------------------------------------
@pytest.mark.parametrize("family", list(H.FAMILIES))
def test_fp32_restatement_holds_a_tenth_of_the_bars(family):
    """Every reduction in the kernel's order, in fp32, against float64: each figure within a tenth of the project bar that the GPU file
    holds it to, or recorded in H.RESTATEMENT (then ten times the record is the GPU bar); sums within their bound, exact on integers."""
    cases, runs, ref, spec = H.FAMILIES[family]
    seen, worst = set(), {}
    for case in cases:
        for key, inp, var in runs(*case):
            sp = spec(var)
            lo, hi = ref(inp, var, F32, True), ref(inp, var)
            for k, (e, b, default) in H.errors(key, inp, var, lo, hi, sp).items():
                worst[k[-1]] = max(worst.get(k[-1], 0.0), e / b)
                if k in H.RESTATEMENT:
                    seen.add(k)
                    assert e <= H.RESTATEMENT[k] <= 2.0 * e and H.RESTATEMENT[k] > default / 10, (k, e, H.RESTATEMENT[k])
                else:
                    assert e <= default / 10, (k, e, default)
            for name, (how, roundings) in sp.items():
                if how != "sum":
                    continue
                n, bound = H.sum_limits(inp, name, roundings)
                err = (lo[name].double() - hi[name]).abs()
                if var["kind"] == "int":
                    assert torch.equal(lo[name].double(), hi[name]), (key, name)
                else:
                    assert bool((err <= bound.reshape(err.shape)).all()), (key, name, float((err - bound.reshape(err.shape)).max()))
    print(family, {k: f"{v:.2f} of its bar" for k, v in worst.items()})
    assert seen == {k for k in H.RESTATEMENT if k[0] == family}, "a recorded case is no longer walked"


def test_offset_batchnorm_loses_three_digits_through_the_chan_fold():
    """mean / std = 1000: one chunk keeps the variance to 1e-5, the fold over three chunks to 1e-4 -- fp32 in this order, not the kernel."""
    inp = H.stats_inputs(257, 255, "offset")
    hi = H.bn_stats(inp["x"].double())[1]
    one, fold = (H.worst_col(H.bn_stats(inp["x"], order=True, chunk=c)[1], hi) for c in (None, H.CHUNK_ROWS))
    print(f"offset 100 / std 0.1, 257 rows: one chunk {one:.2e}, Chan fold {fold:.2e}")
    assert one < 2e-5 < fold < 2e-4


# ---- the geometry: every case list is past the loop limit it is there to cross -------------------------------------------------------
def test_geometry_and_loop_limits():
    assert (H.QUAD_BLOCK, H.QUAD_WAVE, H.ROWS_PER_BLOCK, H.COLS_PER_BLOCK, H.CHUNK_ROWS, H.DINO_CHUNK, H.XENT_ROWS) == (256 * 4, 64 * 4, 4, 256, 128, 1024, 256)
    for cases in (H.L2_CASES, H.WN_CASES):  # 64 lanes x 4 columns; 4 rows per block
        ns, rows = {n for _, n in cases}, {r for r, _ in cases}
        assert all(n % 4 == 0 for n in ns) and 4 in ns and H.QUAD_WAVE in ns and H.QUAD_WAVE + 4 in ns
        assert any(r < H.ROWS_PER_BLOCK for r in rows) and any(r > H.ROWS_PER_BLOCK and r % H.ROWS_PER_BLOCK for r in rows)
    l2n = {n for _, n in H.L2_CASES}
    assert H.QUAD_WAVE - 4 in l2n and any(n > 4 * H.QUAD_WAVE and n % H.QUAD_WAVE for n in l2n) and {1, 5, 9} == {m for m, _ in H.L2_CASES}
    assert any(k > 16 * H.ROWS_PER_BLOCK and k % H.ROWS_PER_BLOCK == 1 for k, _ in H.WN_CASES)
    # bn_gelu: 256 threads x 4 columns per block; the sums kernel one thread per column
    quads = [M * D // 4 for M, D in H.BNG_CASES]
    assert sum(q % 256 != 0 for q in quads) > len(quads) // 2 and min(quads) < 256 and max(quads) > 256 * 4
    assert any(D > H.COLS_PER_BLOCK for _, D in H.BNG_CASES) and any(M > H.CHUNK_ROWS for M, _ in H.BNG_CASES) and all(D % 4 == 0 for _, D in H.BNG_CASES)
    assert all(c in H.BNG_CASES for c in (H.BNG_NULL_CASE, H.BNG_WIDEN_CASE, H.BNG_DP_CASE))
    # BatchNorm statistics: one thread per column, 128-row chunks
    assert 1 in H.STATS_D and H.COLS_PER_BLOCK - 1 in H.STATS_D and H.COLS_PER_BLOCK + 1 in H.STATS_D
    assert 2 in H.STATS_B and H.CHUNK_ROWS + 1 in H.STATS_B
    assert {2, H.CHUNK_ROWS, H.CHUNK_ROWS + 1, 2 * H.CHUNK_ROWS + 1} <= set(H.STATS_ROWS) and any(r > 2 * H.CHUNK_ROWS + 1 and r % H.CHUNK_ROWS > 1 for r in H.STATS_ROWS)
    assert any(r * D // 4 % 256 and D % 4 == 0 for r, D in H.NORM_CASES) and any(r * D // 4 > 256 for r, D in H.NORM_CASES)
    rows, Ds = {r for r, _ in H.BWD_CASES}, {D for _, D in H.BWD_CASES}
    assert min(rows) < H.CHUNK_ROWS and H.CHUNK_ROWS + 1 in rows and 2 * H.CHUNK_ROWS + 2 in rows and all(r % 3 == 0 for r in rows)
    assert any(D % 4 for D in Ds) and any(D > H.COLS_PER_BLOCK for D in Ds) and {(1, 1), (1, 5), (3, 1), (3, 5)} == set(H.BWD_FUSED)
    # softmax_xent: 256 rows per trip of the single workgroup
    Bs = {B for B, _ in H.XENT_CASES}
    assert {1, H.XENT_ROWS - 1, H.XENT_ROWS, H.XENT_ROWS + 1} <= Bs and any(B > 2 * H.XENT_ROWS for B in Bs) and {1, 2, 5} == {C for _, C in H.XENT_CASES}
    assert {t for _, t in H.CLIP_CASES} == {4, H.QUAD_BLOCK + 4} and {s for s, _ in H.CLIP_CASES} == {1, 7}
    # dino_loss: 1024 columns per block / per trip of the row statistics
    Ks = {K for _, _, K in H.DINO_CASES}
    assert min(Ks) == 4 and H.DINO_CHUNK in Ks and H.DINO_CHUNK + 4 in Ks and 2 * H.DINO_CHUNK + 4 in Ks and any(H.DINO_CHUNK - 256 < K < H.DINO_CHUNK for K in Ks)
    assert {V for V, _, _ in H.DINO_CASES} == {2, 3, 10} and {B for _, B, _ in H.DINO_CASES} == {1, 3} and all(K % 4 == 0 for K in Ks)
    assert {K for K, _ in H.CENTER_CASES} == {1, H.COLS_PER_BLOCK - 1, H.COLS_PER_BLOCK + 1}


# ---- the GPU test's inputs ------------------------------------------------------------------------------------------------------------
def _small_int(t):
    return bool((t == t.round()).all()) and float(t.abs().max()) <= 5 and torch.equal(t.to(BF16).float(), t)


def test_l2_and_weight_norm_inputs():
    for M, n in H.L2_CASES:
        z = H.l2_inputs(M, n)["z"]
        assert (M > H.L2_ZERO_ROW) == bool((z == 0).all(dim=1).any()) and int((z == 0).all(dim=1).sum()) <= 1
        assert bool((z[:, n - 4:] != 0).any())  # the ragged tail carries weight
    for K, n in H.WN_CASES:
        inp = H.wn_inputs(K, n, "int")
        v, dw = inp["v"], inp["dw"]
        assert bool(((v != 0).sum(1) == 1).all()) and bool((v.abs().sum(1) == 1).all()) and _small_int(dw) and _small_int(inp["g"])
        assert bool((v[1::2, n - 1] != 0).all())  # odd rows: the single term sits in the last column (the last lane of the last trip)
        assert bool(((dw * v).sum(1) != 0).all()) and torch.equal(H.weight_norm_bwd(dw, v, inp["g"], torch.ones(K), order=True)[1], (dw * v).sum(1))


@pytest.mark.parametrize("M,D", H.BNG_CASES)
def test_bn_gelu_inputs(M, D):
    inp = H.bng_inputs(M, D, "normal")
    y = H.bn_gelu(inp["u"].double(), inp["mean"].double(), inp["var"].double(), inp["gamma"].double(), inp["beta"].double(), H.EPS)[1] * inp["gamma"] + inp["beta"]
    assert float(y.min()) < -5.5 and float(y.max()) > 5.5 and float(y.abs().max()) < 7.0 and bool((y[:, 0] > 0.8).all())  # both tails of erf
    inp = H.bng_inputs(M, D, "int")
    assert bool((inp["dact"] == 1).all()) and _small_int(inp["dh"]) and _small_int(inp["xhat"]) and bool((inp["dh"][M - 1] != 0).any())
    sums = H.bn_gelu_bwd_sums(inp["dh"], inp["dact"], inp["xhat"], order=True)
    assert torch.equal(sums.double(), H.bn_gelu_bwd_sums(inp["dh"].double(), inp["dact"].double(), inp["xhat"].double()))


def test_stats_inputs():
    for rows in H.STATS_ROWS:
        for D in H.STATS_D:
            x = H.stats_inputs(rows, D, "int")["x"]
            assert _small_int(x) and float(x.abs().sum(0).max()) < 2 ** 24
            c = H.stats_inputs(rows, D, "centred")
            assert c["x"].shape == (rows, D) and bool((c["rmean"] * c["x"].mean(0) >= 0).all()) and bool((c["rvar"] > 0).all())
            o = H.stats_inputs(rows, D, "offset")["x"].double()
            assert float((o - 100.0).abs().max()) < 0.6 and (rows < 100 or abs(float(o.std()) - 0.1) < 0.02)
    g = H.strided(torch.ones(3, 5), 17)
    assert g.shape == (3, 17) and bool(torch.isnan(g[:, 5:]).all()) and bool((g[:, :5] == 1).all())


@pytest.mark.parametrize("B,C", H.XENT_CASES)
def test_xent_inputs(B, C):
    inp = H.xent_inputs(B, C)
    logits, target = inp["logits"], inp["target"]
    assert bool((logits[B // 2] == logits[B // 2, 0]).all()) and float(logits.abs().max()) <= 80.0 and bool(((target >= 0) & (target < C)).all())
    big = torch.arange(B) % 2 == 0
    big[B // 2] = False
    if B > 2:
        assert float(logits[big].abs().max()) > 40.0  # exp overflows fp32 at 88.7: two such logits without the max subtraction
    if C > 1 and bool(big.any()):
        assert bool((target[big] != logits[big].argmax(dim=1)).all())


def test_dino_inputs():
    for V, B, K in H.DINO_CASES:
        base = H.dino_inputs(V, B, K, "normal", F32)
        assert base["student"].shape == (V * B, K) and base["teacher"].shape == (2 * B, K)
        t = H.dino_inputs(V, B, K, "int", BF16)["teacher"]
        assert t.dtype == BF16 and _small_int(t.float()) and bool((t[:, K - 4:] != 0).any())
        sh = H.dino_inputs(V, B, K, "shifted", F32)
        assert float(sh["student"][-1].mean()) > 29 and float(sh["teacher"][-1].mean()) > 29 and (V * B == 1 or abs(float(sh["student"][0].mean())) < 1)
        pk = H.dino_inputs(V, B, K, "peaked", F32)["teacher"][0]
        assert float(pk.max()) == 8.0 and float(pk.sort().values[-2]) < 0.6
        q = F.softmax((pk.double() - H.dino_inputs(V, B, K, "peaked", F32)["center"].double()) / 0.04, dim=-1)
        assert float(q.max()) > 1 - 1e-9  # nearly one-hot
