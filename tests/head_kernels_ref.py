"""Yardstick of the DINO loss, projection-head and classifier-head kernels (csrc/dino.hip, csrc/heads.hip, csrc/finetune.hip): plain
torch restatements of the definitions at the head of those files and in include/headct_hip.h.  The arithmetic runs in the dtype of
the tensors handed in (the tests hand in float64).  With `order=True` every reduction is taken in the kernel's own order (rows in
index order, 128-row chunks and the Chan fold, a xor-butterfly over 64 lanes that each hold a strided partial): in fp32 that shows
what fp32 arithmetic alone costs, which tests/test_head_kernels_ref_cpu.py holds against the bars of the GPU file.  The second half
builds the inputs of tests/test_head_kernels_gpu.py.  Nothing here calls the code under test."""
import math

import torch
import torch.nn.functional as F

from tests.assembly_ref import U32, gen, rel, sum_bound, values  # noqa: F401  (re-exported for the two test files)

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
FP32_BAR = 1e-5        # test_layernorm_fwd_bwd's bar for fp32 arithmetic on identical inputs
BF16_BAR = 4e-3        # ... and for values stored as bf16
DINO_LOSS_BAR = 2e-5   # test_dino_loss_full_width_vs_oracle: the loss,
DINO_GRAD_BAR = {F32: 1e-4, BF16: 6e-3}  # ... and its gradient, here per (crop, sample) row

# ---- loop limits of the kernels (test_head_kernels_ref_cpu.py asserts that every case list crosses the ones it is there to cross) --
QUAD_BLOCK = 1024      # 256 threads x 4 columns: elements per block of bn_gelu_fwd / bn_gelu_bwd_apply / bn_norm / scale_by / add_f32
QUAD_WAVE = 256        # 64 lanes x 4 columns: one trip of the l2norm / weight_norm lane loops
ROWS_PER_BLOCK = 4     # one wave per row in those kernels: four rows per block
COLS_PER_BLOCK = 256   # one thread per column: bn_gelu_bwd_sums, batch_stats, the chunk and fold kernels, dino_center_update
CHUNK_ROWS = 128       # kChunkRows of csrc/finetune.hip: rows per chunk of bn_stats_rows / bn_bwd_input
DINO_CHUNK = 1024      # columns per block of dino_loss_grad_kernel and per trip of dino_row_stats_kernel
XENT_ROWS = 256        # rows per trip of softmax_xent_kernel's single workgroup


# ---- reductions: torch's own, or (order=True) the kernels' --------------------------------------------------------------------------
def _butterfly(v):
    """wave_sum of common.h over the last axis (64 lanes): v += shfl_xor(v, o) for o = 32 .. 1."""
    idx = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., idx ^ o]
    return v[..., 0]


def _padded(t, block):
    return F.pad(t, (0, -t.shape[-1] % block))  # adding +0 is exact


def sum_wave(t, order=False):
    """Sum over the last axis as one wave does it: lane l adds the quads at columns 4 l + 256 trip, (a + b) + (c + d), then the butterfly."""
    if not order:
        return t.sum(-1)
    q = _padded(t, QUAD_WAVE).reshape(*t.shape[:-1], -1, 64, 4)
    q = (q[..., 0] + q[..., 1]) + (q[..., 2] + q[..., 3])
    acc = torch.zeros_like(q[..., 0, :])
    for trip in range(q.shape[-2]):
        acc = acc + q[..., trip, :]
    return _butterfly(acc)


def sum_block(t, order=False):
    """Sum over the last axis as a 256-thread block does it: thread t adds columns 4 t + 1024 trip one by one, the four waves' butterflies
    are added (w0 + w1) + (w2 + w3)."""
    if not order:
        return t.sum(-1)
    q = _padded(t, QUAD_BLOCK).reshape(*t.shape[:-1], -1, 256, 4)
    acc = torch.zeros_like(q[..., 0, :, 0])
    for trip in range(q.shape[-3]):
        for e in range(4):
            acc = acc + q[..., trip, :, e]
    w = _butterfly(acc.reshape(*acc.shape[:-1], 4, 64))
    return (w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])


def sum_strided(t, order=False):
    """Sum of a vector by 256 threads that each add elements t, t + 256, ..., then `sum_block`'s wave fold (dino_fold_kernel)."""
    if not order:
        return t.sum(-1)
    q = _padded(t, 256).reshape(-1, 256)
    acc = torch.zeros_like(q[0])
    for trip in range(q.shape[0]):
        acc = acc + q[trip]
    w = _butterfly(acc.reshape(4, 64))
    return (w[0] + w[1]) + (w[2] + w[3])


def sum_rows(t, order=False):
    """Sum over axis 0 in index order (one thread per column)."""
    if not order:
        return t.sum(0)
    acc = torch.zeros_like(t[0])
    for r in range(t.shape[0]):
        acc = acc + t[r]
    return acc


def sum_row_chunks(t, order=False):
    """Sum over axis 0 by chunks of CHUNK_ROWS rows in index order, the chunk sums folded in index order (bn_bwd_chunk / _fold)."""
    if not order:
        return t.sum(0)
    acc = torch.zeros_like(t[0])
    for r0 in range(0, t.shape[0], CHUNK_ROWS):
        acc = acc + sum_rows(t[r0:r0 + CHUNK_ROWS], True)
    return acc


# ---- L2 row normalisation, weight normalisation (dino.hip) ------------------------------------------------------------------------
def l2norm(z, order=False):
    """(zn, inv_norm): zn = z / max(||z||, 1e-12), F.normalize(z, dim=-1)."""
    inv = 1.0 / sum_wave(z * z, order).sqrt().clamp(min=1e-12)
    return z * inv[:, None], inv


def l2norm_bwd(dzn, zn, inv_norm, order=False):
    """dz = (dzn - zn (zn . dzn)) * inv_norm with the STORED zn (for bf16 the rounded one, as the kernel reads it)."""
    dot = sum_wave(dzn * zn, order)
    return (dzn - zn * dot[:, None]) * inv_norm[:, None]


def weight_norm(v, g, order=False):
    """(w, inv_norm): w[k] = g[k] v[k] / ||v[k]||  (torch.nn.utils.weight_norm, dim 0)."""
    inv = 1.0 / sum_wave(v * v, order).sqrt()
    return v * (g * inv)[:, None], inv


def weight_norm_bwd(dw, v, g, inv_norm, order=False):
    """(dv, dg): dg = dw . vhat, dv = g / ||v|| (dw - (dw . vhat) vhat), vhat = v / ||v||."""
    vhat = v * inv_norm[:, None]
    dg = sum_wave(dw * vhat, order)
    return (dw - vhat * dg[:, None]) * (g * inv_norm)[:, None], dg


# ---- BatchNorm1d + GELU of the projection head (dino.hip) ---------------------------------------------------------------------------
def bn_gelu(u, mean, var, gamma, beta, eps):
    """(h, xhat, dact): xhat = (u - mean) / sqrt(var + eps), y = gamma xhat + beta, h = gelu(y) with the exact erf, dact = gelu'(y)."""
    xhat = (u - mean) * (1.0 / (var + eps).sqrt())
    y = gamma * xhat + beta
    cdf = 0.5 * (1.0 + torch.erf(y * (1.0 / math.sqrt(2.0))))
    pdf = torch.exp(-0.5 * y * y) * (1.0 / math.sqrt(2.0 * math.pi))
    return y * cdf, xhat, cdf + y * pdf


def bn_gelu_bwd_sums(dh, dact, xhat, order=False):
    """[2, D]: the column sums of dy = dh dact and of dy xhat, rows in index order."""
    dy = dh * dact
    return torch.stack((sum_rows(dy, order), sum_rows(dy * xhat, order)))


def bn_gelu_bwd_apply(dh, dact, xhat, gamma, var, eps, sums, count):
    """du = gamma rstd (dy - sums[0] / count - xhat sums[1] / count)."""
    inv = 1.0 / count
    return gamma * (1.0 / (var + eps).sqrt()) * (dh * dact - sums[0] * inv - xhat * sums[1] * inv)


def bn_gelu_bwd(dh, dact, xhat, gamma, var, eps, count, order=False):
    """(sums [2, D], du) of one rank that holds every row the statistics were taken over (count = rows) or a part of them."""
    sums = bn_gelu_bwd_sums(dh, dact, xhat, order)
    return sums, bn_gelu_bwd_apply(dh, dact, xhat, gamma, var, eps, sums, count)


# ---- BatchNorm1d training statistics, apply, input backward (heads.hip, finetune.hip) ----------------------------------------------
def bn_stats(x, momentum=0.1, running=None, order=False, chunk=CHUNK_ROWS):
    """(mean, biased variance, running mean, running variance) of nn.BatchNorm1d in training mode over the rows of x; the running pair
    (None when `running` is None) moves by `momentum` towards the mean and the UNBIASED variance.  order=True: CHUNK_ROWS-row chunks, each
    with its own mean and sum of squared deviations in index order, merged in index order by Chan's update (one chunk: as it is;
    hct_batchnorm_stats is the single chunk of any length, chunk=None)."""
    n = x.shape[0]
    if not order:
        mean = x.mean(0)
        m2 = ((x - mean) ** 2).sum(0)
    else:
        cnt = 0
        for r0 in range(0, n, chunk or n):
            c = x[r0:r0 + (chunk or n)]
            nc = c.shape[0]
            mc = sum_rows(c, True) / nc
            qc = sum_rows((c - mc) ** 2, True)
            if cnt == 0:
                mean, m2 = mc, qc
            else:
                nt, delta = cnt + nc, mc - mean
                mean = mean + delta * (nc / nt)
                m2 = m2 + (qc + delta * delta * (cnt * nc / nt))
            cnt += nc
    var = m2 / n
    if running is None:
        return mean, var, None, None
    return mean, var, (1.0 - momentum) * running[0] + momentum * mean, (1.0 - momentum) * running[1] + momentum * (m2 / (n - 1))


def bn_norm(x, mean, var, eps):
    return (x - mean) * (1.0 / (var + eps).sqrt())


def bn_bwd_input(x, mean, var, eps, g=None, dlogits=None, W=None, nq=1, order=False):
    """dx of BatchNorm1d(affine=False) in training mode: rstd (g - mean_r g - xhat mean_r(g xhat)).  g is given, or is the dgrad of
    Linear(mean over nq consecutive rows): g[r] = 1/nq dlogits[r // nq] @ W."""
    if g is None:
        g = (dlogits @ W).repeat_interleave(nq, dim=0)
        if nq > 1:
            g = g / nq
    rows = x.shape[0]
    rstd = 1.0 / (var + eps).sqrt()
    xhat = (x - mean) * rstd
    a, b = sum_row_chunks(g, order) / rows, sum_row_chunks(g * xhat, order) / rows
    return rstd * (g - a - xhat * b)


# ---- cross-entropy, total-norm clip ------------------------------------------------------------------------------------------------
def softmax_xent(logits, target, dloss=1.0, order=False):
    """(loss, dlogits) of nn.CrossEntropyLoss(): loss = mean_b(logsumexp(l_b) - l_b[t_b]), dlogits = dloss (softmax - onehot) / B.  A target
    outside [0, C) has no one-hot entry and makes the loss NaN."""
    B, C = logits.shape
    m = logits.max(dim=1).values
    e = (logits - m[:, None]).exp()
    z = sum_rows(e.t(), order)  # classes in index order
    valid = (target >= 0) & (target < C)
    picked = torch.gather(logits, 1, target.clamp(0, C - 1)[:, None])[:, 0]
    term = (z.log() + m) - torch.where(valid, picked, torch.full_like(picked, float("nan")))
    if order:  # thread t adds rows t, t + 256, ...; then the LDS tree red[i] += red[i + o], o = 128 .. 1
        red = sum_rows(_padded(term, XENT_ROWS).reshape(-1, XENT_ROWS), True)
        o = XENT_ROWS // 2
        while o > 0:
            red = red[:o] + red[o:2 * o]
            o //= 2
        total = red[0]
    else:
        total = term.sum()
    onehot = torch.zeros_like(logits)
    onehot[valid, target[valid]] = 1.0
    return total / B, (e * (1.0 / z)[:, None] - onehot) * (dloss / B)


def clip_total_norm(grads, norms, max_norm, order=False):
    """(nrm[0], nrm[1], scaled buffer) of clip_grad_norm_: nrm[0] = sqrt(sum norms^2), nrm[1] = min(1, max_norm / (nrm[0] + 1e-6))."""
    total = sum_rows(norms * norms, order).sqrt()
    coef = (max_norm / (total + 1e-6)).clamp(max=1.0)
    return total, coef, grads * coef


# ---- DINO loss and centre (dino.hip) -----------------------------------------------------------------------------------------------
def dino_loss(student, teacher, center, V, Ts, Tt, dloss=1.0, order=False):
    """(loss, dstudent [V B, K], centre sum [K]) from the formulae at the head of dino.hip.  student [V B, K] (crop v of sample b is row
    v B + b), teacher [2 B, K], center [K]:
        q_i = softmax((teacher_i - center) / Tt), logp_v = log_softmax(student_v / Ts),
        loss = 1 / (n B) sum_i sum_{v != i} sum_b sum_k -q_i logp_v,  n = 2 (V - 1),
        dstudent_v = dloss (c_v softmax(student_v / Ts) - sum_{i != v} q_i) / (n B Ts),  c_v = 1 for v < 2, else 2,
        centre sum = the column sum of the 2 B teacher rows (sample by sample: row b + row B + b, then over b)."""
    dt = student.dtype
    B, K = teacher.shape[0] // 2, teacher.shape[1]
    n = 2 * (V - 1)
    inv_ts, inv_tt = (torch.ones((), dtype=dt) / torch.tensor(T, dtype=dt) for T in (Ts, Tt))

    def log_softmax(x, inv_t):  # x [R, K] -> scaled logit - max - log(sum exp)
        m = x.max(dim=1).values * inv_t
        lse = sum_block((x * inv_t - m[:, None]).exp(), order).log()
        return x * inv_t - m[:, None] - lse[:, None]
    q = log_softmax(teacher - center, inv_tt).exp().reshape(2, B, K)
    logp = log_softmax(student, inv_ts).reshape(V, B, K)
    qs = torch.stack([q[1] if v == 0 else q[0] if v == 1 else q[0] + q[1] for v in range(V)])
    cv = torch.tensor([1.0 if v < 2 else 2.0 for v in range(V)], dtype=dt).reshape(V, 1, 1)
    terms = qs * logp  # the loss is minus their sum over everything, / (n B)
    denom = torch.tensor(float(n), dtype=dt) * torch.tensor(float(B), dtype=dt)
    if order:  # block (b, chunk): thread t takes four columns and every crop, acc -= q logp; the block's sum; then dino_fold_kernel
        t5 = _padded(terms, DINO_CHUNK).reshape(V, B, -1, 256, 4)
        acc = torch.zeros_like(t5[0, ..., 0])
        for v in range(V):
            for e in range(4):
                acc = acc - t5[v, ..., e]
        w = _butterfly(acc.reshape(*acc.shape[:-1], 4, 64))
        partial = (w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])  # [B, nchunk]
        loss = sum_strided(partial.reshape(-1), True) * (1.0 / denom)
    else:
        loss = -terms.sum() / denom
    g = (inv_ts / denom) * dloss
    dstudent = ((cv * logp.exp() - qs) * g).reshape(V * B, K)
    return loss, dstudent, sum_rows(teacher[:B] + teacher[B:], order)


def center_update(center, batch_sum, m, count):
    """fp32 tensors in torch's operation order (losses.py:95-102): 1 - m is formed in double by Python and narrowed by torch."""
    return center * m + (batch_sum / count) * (1 - m)


# ---- error measures ------------------------------------------------------------------------------------------------------------------
def worst_row(got, ref):
    """The largest relative L2 error of a row (last axis) of got against ref; a row whose reference is zero must be zero."""
    g, r = got.detach().double().cpu(), ref.detach().double().cpu()
    g, r = g.reshape(-1, g.shape[-1]), r.reshape(-1, r.shape[-1])
    assert g.shape == r.shape and not bool(torch.isnan(g).any()), "shape mismatch or NaN in the result"
    return float(((g - r).norm(dim=1) / (r.norm(dim=1) + 1e-30)).max())


def worst_col(got, ref, scale=None):
    """Column statistics: the largest error of an element, relative to the reference (or to `scale`, e.g. the mean of |x| for a mean)."""
    g, r = got.detach().double().cpu().flatten(), ref.detach().double().cpu().flatten()
    assert g.shape == r.shape and not bool(torch.isnan(g).any()), "shape mismatch or NaN in the result"
    return float(((g - r).abs() / ((r.abs() if scale is None else scale.double().flatten()) + 1e-30)).max())


def product_sum_bound(n_terms, roundings, abs_sum):
    """Bound of an fp32 sum, in any order, of n terms that are each the rounded product of `roundings` + 1 fp32 factors, against the exact
    sum of the exact products: gamma_(n - 1 + roundings) sum|terms| <= (n + roundings) 2^-24 sum|terms| (Higham, Accuracy and Stability
    of Numerical Algorithms, lemma 3.1 and (4.4); gamma_k = k u / (1 - k u) <= (k + 1) u for k <= 4000)."""
    return (n_terms + roundings) * U32 * abs_sum.double()


# measured: the worst error of the order=True restatement in fp32 against float64, for the cases where it exceeds a tenth of the bar
# that the case would otherwise take (tests/test_head_kernels_ref_cpu.py asserts each entry against the measurement: not below it, not
# above twice it).  The GPU bar of such a case is TEN times the entry: fp32 arithmetic in the kernel's own order cannot be held tighter.
RESTATEMENT = {
    ("batchnorm_stats", 2, 255, "offset", F32, "var"): 1.06e-05,
    ("batchnorm_stats", 2, 257, "offset", F32, "var"): 2.49e-06,
    ("batchnorm_stats", 3, 255, "offset", F32, "var"): 7.76e-06,
    ("batchnorm_stats", 129, 255, "int", F32, "var"): 1.27e-06,
    ("batchnorm_stats", 129, 257, "int", F32, "var"): 1.20e-06,
    ("bn_stats_rows", 2, 255, "offset", F32, "var"): 1.06e-05,
    ("bn_stats_rows", 2, 257, "offset", F32, "var"): 2.49e-06,
    ("bn_stats_rows", 128, 255, "centred", BF16, "var"): 1.86e-06,
    ("bn_stats_rows", 129, 1, "offset", F32, "var"): 4.27e-06,
    ("bn_stats_rows", 129, 255, "centred", BF16, "var"): 2.11e-06,
    ("bn_stats_rows", 129, 255, "offset", F32, "var"): 1.13e-05,
    ("bn_stats_rows", 129, 257, "centred", BF16, "var"): 1.34e-06,
    ("bn_stats_rows", 129, 257, "offset", F32, "var"): 1.19e-05,
    ("bn_stats_rows", 257, 1, "offset", F32, "var"): 1.34e-06,
    ("bn_stats_rows", 257, 255, "centred", BF16, "var"): 1.12e-06,
    ("bn_stats_rows", 257, 255, "offset", F32, "var"): 8.90e-05,   # mean / std = 1000 through the Chan fold: three digits lost
    ("bn_stats_rows", 257, 257, "offset", F32, "var"): 6.61e-05,
    ("bn_stats_rows", 300, 1, "offset", F32, "var"): 1.97e-05,
    ("bn_stats_rows", 300, 1, "offset", BF16, "var"): 1.60e-06,
    ("bn_stats_rows", 300, 255, "offset", F32, "var"): 4.58e-05,
    ("bn_stats_rows", 300, 255, "offset", BF16, "var"): 1.22e-05,
    ("bn_stats_rows", 300, 257, "offset", F32, "var"): 6.94e-05,
    ("bn_stats_rows", 300, 257, "offset", BF16, "var"): 1.23e-05,
    ("bn_bwd_input", 129, 7, "fused", 1, 1, F32, F32, "dx"): 1.33e-06,
    ("bn_bwd_input", 129, 260, "fused", 3, 1, F32, F32, "dx"): 1.40e-06,
    ("bn_bwd_input", 258, 7, "fused", 3, 1, F32, F32, "dx"): 1.15e-06,
    ("softmax_xent", 256, 2, None, "dlogits"): 1.96e-06,   # a row with p = (0.98, 0.02) and target 0: p - 1 at the resolution of 1
    ("softmax_xent", 256, 2, 3.0, "dlogits"): 1.96e-06,
    ("softmax_xent", 600, 2, None, "dlogits"): 2.50e-06,
    ("softmax_xent", 600, 2, 3.0, "dlogits"): 2.45e-06,
    ("dino_loss", 2, 1, 4, "shifted", 0.07, F32, "loss"): 4.09e-06,   # +30 on a row: scaled logits of 300 and 430 before the max leaves
    ("dino_loss", 2, 1, 1024, "shifted", 0.07, F32, "dstudent"): 2.18e-05,
    ("dino_loss", 10, 3, 4, "shifted", 0.07, F32, "dstudent"): 1.43e-05,
    ("dino_loss", 10, 3, 1024, "shifted", 0.07, F32, "dstudent"): 1.31e-05,
}


def bar(key, default):
    """The bar of one figure of one case: `default` (a project bar), or ten times the restatement's recorded error where that is larger
    than a tenth of the default."""
    return 10.0 * RESTATEMENT[key] if key in RESTATEMENT else default


# =================================================================================================================================
# Inputs of tests/test_head_kernels_gpu.py.  Everything is made on the CPU from seeded generators and rounded to its storage type.
# =================================================================================================================================
L2_CASES = [(M, n) for M in (1, 5, 9) for n in (4, 252, 256, 260, 1028)]   # M: the last block has idle waves; n: see QUAD_WAVE
L2_ZERO_ROW = 2                                                            # at M >= 5 this row of z is all zero
WN_CASES = [(K, n) for K in (3, 6, 65) for n in (4, 256, 260)]
BNG_CASES = [(M, D) for M in (2, 10, 131) for D in (4, 48, 260, 1028)]
BNG_NULL_CASE, BNG_WIDEN_CASE, BNG_DP_CASE = (10, 48), (10, 260), (131, 48)   # xhat / dact NULL; fp32 du from bf16 dh; count = 2 M
STATS_D = (1, 255, 257)
STATS_B = (2, 3, 129)                      # hct_batchnorm_stats
STATS_ROWS = (2, 128, 129, 257, 300)       # hct_bn_stats_rows: one chunk, a full chunk, a chunk of one row, three chunks, a ragged third
STATS_KINDS = ("int", "centred", "offset")
NORM_CASES = [(7, 260), (1, 4), (5, 1028)]
BWD_CASES = [(rows, D) for rows in (6, 129, 258) for D in (7, 260)]
BWD_FUSED = [(nq, ncls) for nq in (1, 3) for ncls in (1, 5)]
XENT_CASES = [(B, C) for B in (1, 255, 256, 257, 600) for C in (1, 2, 5)]
CLIP_CASES = [(nseg, total) for nseg in (1, 7) for total in (4, 1028)]
DINO_CASES = [(V, B, K) for V in (2, 3, 10) for B in (1, 3) for K in (4, 1000, 1024, 1028, 2052)]
DINO_TS, DINO_TT = 0.1, (0.04, 0.07)
DINO_KINDS = ("normal", "int", "shifted", "peaked")
CENTER_CASES = [(K, count) for K in (1, 255, 257) for count in (2, 16)]
EPS = 1e-5


def f32_scalar(x):
    """A Python float rounded to fp32, as a c_float argument arrives in the kernel."""
    return float(torch.tensor(x, dtype=F32))


def l2_inputs(M, n):
    g = gen(M, n, 21)
    z, dzn = values((M, n), "normal", g), values((M, n), "normal", g)
    if M > L2_ZERO_ROW:
        z[L2_ZERO_ROW] = 0.0
    return dict(z=z, dzn=dzn)


def wn_inputs(K, n, kind):
    """"int": every row of v holds a single +-1 (odd rows: in the last column), so ||v|| = 1 and dg = dw . v is one term of integer dw."""
    g = gen(K, n, kind == "int", 22)
    dw = values((K, n), kind, g)
    if kind == "int":
        v = torch.zeros(K, n)
        col = torch.randint(0, n, (K,), generator=g)
        col[1::2] = n - 1
        v[torch.arange(K), col] = torch.where(torch.arange(K) % 3 == 0, -1.0, 1.0)
        dw[torch.arange(K), col] = torch.where(torch.arange(K) % 2 == 0, 3.0, -2.0)  # the one term is never zero
        gain = values((K,), "int", g).abs() + 1.0
    else:
        v, gain = values((K, n), kind, g), values((K,), kind, g).abs() + 0.5
    return dict(v=v, g=gain, dw=dw)


def bng_inputs(M, D, kind):
    """u such that y = gamma xhat + beta spans [-6.6, 6.6] with both ends met; statistics are free inputs of the kernel.  Column 0 lies in
    [1, 6]: a row that lies in the left tail as a whole (D = 4) has h = y (1 + erf) / 2 of 1e-6 and less, which fp32 forms from 1 + erf at
    a resolution of 6e-8, so its relative error measures the formula and not the kernel.  The backward's dact and xhat are the forward's
    (fp32-rounded); "int": dact = 1 and integer dh and xhat, whose sums are exact."""
    g = gen(M, D, kind == "int", 23)
    mean, var = torch.randn(D, generator=g), 0.5 + torch.rand(D, generator=g)
    gamma, beta = 1.0 + 0.1 * torch.rand(D, generator=g), 0.1 * torch.randn(D, generator=g)
    t = torch.rand(M, D, generator=g) * 12.0 - 6.0
    t[:, 0] = 1.0 + 5.0 * torch.rand(M, generator=g)
    t[0, 1], t[M - 1, D - 1] = -6.0, 6.0
    u = mean + (var + EPS).sqrt() * t
    h, xhat, dact = bn_gelu(u.double(), mean.double(), var.double(), gamma.double(), beta.double(), EPS)
    dh = values((M, D), kind, g)
    if kind == "int":
        xhat, dact = values((M, D), "int", g), torch.ones(M, D)
    return dict(u=u, mean=mean, var=var, gamma=gamma, beta=beta, dh=dh, xhat=xhat.float(), dact=dact.float())


def stats_inputs(rows, D, kind):
    """"int": integers in [-4, 4]; "centred": unit variance around a column mean of magnitude 0.5 .. 3; "offset": mean 100, std 0.1."""
    g = gen(rows, D, STATS_KINDS.index(kind), 24)
    if kind == "int":
        x = values((rows, D), "int", g)
    elif kind == "centred":
        mu = (0.5 + 2.5 * torch.rand(D, generator=g)) * torch.where(torch.rand(D, generator=g) < 0.5, -1.0, 1.0)
        x = torch.randn(rows, D, generator=g) + mu
    else:
        x = 100.0 + 0.1 * torch.randn(rows, D, generator=g)
    sign = torch.where(x.mean(0) < 0, -1.0, 1.0)  # 0.9 rmean + 0.1 mean does not cancel: the running mean lies on the mean's side
    return dict(x=x, rmean=sign * (1.0 + torch.rand(D, generator=g)), rvar=0.5 + torch.rand(D, generator=g))


def strided(x, ld, fill=float("nan")):
    """x [rows, D] inside a [rows, ld] buffer whose gap columns hold `fill`; returns the buffer."""
    buf = torch.full((x.shape[0], ld), fill, dtype=x.dtype)
    buf[:, :x.shape[1]] = x
    return buf


def bwd_inputs(rows, D, nq, ncls):
    """x with its own batch statistics (fp32-rounded), a given g, and the dlogits / W of the fused form."""
    g = gen(rows, D, nq, ncls, 25)
    x = torch.randn(rows, D, generator=g) * (0.5 + torch.rand(D, generator=g)) + torch.randn(D, generator=g)
    mean, var, _, _ = bn_stats(x.double())
    return dict(x=x, mean=mean.float(), var=var.float(), g=torch.randn(rows, D, generator=g),
                dlogits=torch.randn(rows // nq, ncls, generator=g), W=torch.randn(ncls, D, generator=g))


def xent_inputs(B, C):
    """Even rows: logits uniform in +-80 (without the max subtraction exp overflows); odd rows: in +-2.  Row B // 2 has all logits equal.
    A saturated row whose target is its own maximum has the gradient p - 1 = -e^-gap, below the resolution of fp32 at 1, which no fp32
    arithmetic can produce; so the +-80 rows take another class as target (C = 1: the gradient is exactly zero either way)."""
    g = gen(B, C, 26)
    logits = (torch.rand(B, C, generator=g) * 2.0 - 1.0) * torch.where(torch.arange(B) % 2 == 0, 80.0, 2.0)[:, None]
    logits[B // 2] = 3.5
    target = torch.randint(0, C, (B,), generator=g)
    big = torch.arange(B) % 2 == 0
    target[big] = (logits[big].argmax(dim=1) + 1 + target[big] % max(C - 1, 1)) % C
    return dict(logits=logits, target=target)


def clip_inputs(nseg, total):
    g = gen(nseg, total, 27)
    return dict(grads=torch.randn(total, generator=g), norms=torch.rand(nseg, generator=g) + 0.1)


def dino_inputs(V, B, K, kind, dtype):
    """"normal": unit normal logits; "int": integer teacher logits (the centre sum is exact); "shifted": +30 on every logit of the last
    student row and the last teacher row; "peaked": the first teacher row is 0.1-normal with one logit 8 above.  Rounded to `dtype`.  Below one chunk (K = 4) the student logits
    have a standard deviation of 0.05: unit-normal logits over T = 0.1 and 0.04 make both p and q nearly one-hot among four columns, and where
    they peak on the same column the gradient c p - q is e^-gap, a difference that fp32 cannot resolve in any order."""
    g = gen(V, B, K, DINO_KINDS.index(kind), 28)
    student, teacher = torch.randn(V * B, K, generator=g) * (1.0 if K >= DINO_CHUNK - 24 else 0.05), torch.randn(2 * B, K, generator=g)
    center = 0.1 * torch.randn(K, generator=g)
    if kind == "int":
        teacher = values((2 * B, K), "int", g)
    elif kind == "shifted":
        student[-1] += 30.0
        teacher[-1] += 30.0
    elif kind == "peaked":
        teacher[0] = 0.1 * torch.randn(K, generator=g)
        teacher[0, K // 3] = 8.0
    return dict(student=student.to(dtype), teacher=teacher.to(dtype), center=center)


def center_inputs(K, count):
    g = gen(K, count, 29)
    return dict(center=torch.randn(K, generator=g), sum=torch.randn(K, generator=g) * count)


# =================================================================================================================================
# The cases as both test files walk them: `X_runs(case)` yields (key, inputs, variant) for every call the GPU file makes whose VALUES
# differ, `X_ref(inputs, variant, dtype, order)` the figures of that call, `X_spec(variant)` how each figure is held:
#   ("row" | "col", project bar)   the worst row's relative L2 / the worst element's relative error, `bar(key + (name,), project bar)`
#   ("sum", roundings)             |got - ref| <= product_sum_bound per element (roundings = 0: sum_bound), exact on "int" inputs
# Figures named in `inp["sum_terms"]` carry (n_terms, sum|terms|) for the "sum" kind.
# =================================================================================================================================
def _c(inp, dt, *names):
    return [inp[k].to(dt) for k in names]


def l2_runs(M, n):
    inp = l2_inputs(M, n)
    zn, inv = l2norm(inp["z"].double())
    for zdt in (F32, BF16):
        yield ("l2norm", M, n, zdt), dict(inp, zn_in=zn.float().to(zdt), inv_in=inv.float()), dict(zdt=zdt)


def l2_ref(inp, var, dt=F64, order=False):
    z, dzn, zn_in, inv_in = _c(inp, dt, "z", "dzn", "zn_in", "inv_in")
    zn, inv = l2norm(z, order)
    return dict(zn=zn, inv_norm=inv, dz=l2norm_bwd(dzn, zn_in, inv_in, order))


def l2_spec(var):
    return dict(zn=("row", BF16_BAR if var["zdt"] == BF16 else FP32_BAR), inv_norm=("col", FP32_BAR), dz=("row", FP32_BAR))


def wn_runs(K, n):
    for kind in ("int", "normal"):
        inp = wn_inputs(K, n, kind)
        inv = weight_norm(inp["v"].double(), inp["g"].double())[1].float()
        vhat = inp["v"] * inv[:, None]  # fp32, as the kernel forms it: one rounding, a second in the product with dw
        inp = dict(inp, inv_in=inv, sum_terms=dict(dg=(torch.full((K,), n), (inp["dw"].double() * vhat.double()).abs().sum(1))))
        for wdt in (F32, BF16):
            yield ("weight_norm", K, n, kind, wdt), inp, dict(kind=kind, wdt=wdt)


def wn_ref(inp, var, dt=F64, order=False):
    v, g, dw, inv_in = _c(inp, dt, "v", "g", "dw", "inv_in")
    w, inv = weight_norm(v, g, order)
    dv, dg = weight_norm_bwd(dw, v, g, inv_in, order)
    return dict(w=w, inv_norm=inv, dv=dv, dg=dg)


def wn_spec(var):
    return dict(w=("row", BF16_BAR if var["wdt"] == BF16 else FP32_BAR), inv_norm=("col", FP32_BAR), dv=("row", FP32_BAR), dg=("sum", 2))


def bng_runs(M, D):
    for kind in ("int", "normal"):
        base = bng_inputs(M, D, kind)
        for hdt in (F32, BF16):
            inp = dict(base, dh=base["dh"].to(hdt))
            dy = inp["dh"].double() * inp["dact"].double()
            sums = bn_gelu_bwd_sums(inp["dh"].double(), inp["dact"].double(), inp["xhat"].double())
            n = torch.full((2, D), M)
            inp.update(sums_in=sums.float(), sum_terms=dict(sums=(n, torch.stack((dy.abs().sum(0), (dy * inp["xhat"].double()).abs().sum(0))))))
            dudt = F32 if (M, D) == BNG_WIDEN_CASE else hdt
            yield ("bn_gelu", M, D, kind, hdt), inp, dict(kind=kind, hdt=hdt, dudt=dudt, count=2 * M if (M, D) == BNG_DP_CASE else M)


def bng_ref(inp, var, dt=F64, order=False):
    u, mean, v, gamma, beta, dh, xhat, dact, sums_in = _c(inp, dt, "u", "mean", "var", "gamma", "beta", "dh", "xhat", "dact", "sums_in")
    h, xh, da = bn_gelu(u, mean, v, gamma, beta, EPS)
    return dict(h=h, xhat=xh, dact=da, sums=bn_gelu_bwd_sums(dh, dact, xhat, order),
                du=bn_gelu_bwd_apply(dh, dact, xhat, gamma, v, EPS, sums_in, var["count"]))


def bng_spec(var):
    return dict(h=("row", BF16_BAR if var["hdt"] == BF16 else FP32_BAR), xhat=("row", FP32_BAR), dact=("row", FP32_BAR),
                sums=("sum", 2), du=("row", BF16_BAR if var["dudt"] == BF16 else FP32_BAR))


def stats_runs(rows, D, dtypes=(F32,), family="batchnorm_stats"):
    for kind in STATS_KINDS:
        base = stats_inputs(rows, D, kind)
        for xdt in dtypes:
            inp = dict(base, x=base["x"].to(xdt))
            inp["mean_scale"] = inp["x"].double().abs().mean(0)
            yield (family, rows, D, kind, xdt), inp, dict(kind=kind, xdt=xdt, chunk=CHUNK_ROWS if family == "bn_stats_rows" else None)


def stats_ref(inp, var, dt=F64, order=False):
    x, rmean, rvar = _c(inp, dt, "x", "rmean", "rvar")
    mean, v, rm, rv = bn_stats(x, 0.1, (rmean, rvar), order, var["chunk"])
    return dict(mean=mean, var=v, running_mean=rm, running_var=rv)


def stats_spec(var):
    return dict(mean=("col", FP32_BAR), var=("col", FP32_BAR), running_mean=("col", FP32_BAR), running_var=("col", FP32_BAR))


def norm_runs(rows, D):
    g = gen(rows, D, 30)
    x = torch.randn(rows, D, generator=g) * (0.5 + torch.rand(D, generator=g)) + torch.randn(D, generator=g)
    mean, v = torch.randn(D, generator=g), 0.5 + torch.rand(D, generator=g)
    for xdt in (F32, BF16):
        for odt in (F32, BF16):
            yield ("bn_norm", rows, D, xdt, odt), dict(x=x.to(xdt), mean=mean, var=v), dict(xdt=xdt, odt=odt)


def norm_ref(inp, var, dt=F64, order=False):
    return dict(out=bn_norm(*_c(inp, dt, "x", "mean", "var"), EPS))


def norm_spec(var):
    return dict(out=("row", BF16_BAR if var["odt"] == BF16 else FP32_BAR))


def bwd_runs(rows, D):
    forms = [("g", 1, 1, F32)] + [("fused", nq, ncls, F32) for nq, ncls in BWD_FUSED] + [("g", 1, 1, BF16), ("fused", 3, 5, BF16)]
    for form, nq, ncls, xdt in forms:
        inp = bwd_inputs(rows, D, nq, ncls)
        inp["x"] = inp["x"].to(xdt)
        for odt in (F32, BF16):
            yield ("bn_bwd_input", rows, D, form, nq, ncls, xdt, odt), inp, dict(form=form, nq=nq, ncls=ncls, xdt=xdt, odt=odt)


def bwd_ref(inp, var, dt=F64, order=False):
    x, mean, v, g, dl, W = _c(inp, dt, "x", "mean", "var", "g", "dlogits", "W")
    if var["form"] == "g":
        return dict(dx=bn_bwd_input(x, mean, v, EPS, g=g, order=order))
    return dict(dx=bn_bwd_input(x, mean, v, EPS, dlogits=dl, W=W, nq=var["nq"], order=order))


def bwd_spec(var):
    return dict(dx=("row", BF16_BAR if var["odt"] == BF16 else FP32_BAR))


def xent_runs(B, C):
    inp = xent_inputs(B, C)
    for dloss in (None, 3.0):
        yield ("softmax_xent", B, C, dloss), inp, dict(dloss=dloss)


def xent_ref(inp, var, dt=F64, order=False):
    loss, dlogits = softmax_xent(inp["logits"].to(dt), inp["target"], var["dloss"] or 1.0, order)
    return dict(loss=loss.reshape(1), dlogits=dlogits)


def xent_spec(var):
    return dict(loss=("col", FP32_BAR), dlogits=("row", FP32_BAR))


def clip_runs(nseg, total):
    inp = clip_inputs(nseg, total)
    norm = float(inp["norms"].double().norm())
    for where, factor in (("below", 0.5), ("above", 2.0)):
        yield ("clip_total_norm", nseg, total, where), inp, dict(where=where, max_norm=f32_scalar(norm * factor))


def clip_ref(inp, var, dt=F64, order=False):
    total, coef, _ = clip_total_norm(inp["grads"].to(dt), inp["norms"].to(dt), var["max_norm"], order)
    return dict(nrm=torch.stack((total, coef)))


def clip_spec(var):
    return dict(nrm=("col", FP32_BAR))


def dino_runs(V, B, K):
    for kind, Tt in (("normal", DINO_TT[0]), ("normal", DINO_TT[1]), ("int", DINO_TT[0]), ("shifted", DINO_TT[1]), ("peaked", DINO_TT[0])):
        for dtype in (F32, BF16):
            inp = dino_inputs(V, B, K, kind, dtype)
            inp["sum_terms"] = dict(center_sum=(torch.full((K,), 2 * B), inp["teacher"].double().abs().sum(0)))
            var = dict(kind=kind, dtype=dtype, V=V, Ts=f32_scalar(DINO_TS), Tt=f32_scalar(Tt))
            yield ("dino_loss", V, B, K, kind, Tt, dtype), inp, var


def dino_ref(inp, var, dt=F64, order=False, dloss=1.0):
    student, teacher, center = _c(inp, dt, "student", "teacher", "center")
    loss, dstudent, csum = dino_loss(student, teacher, center, var["V"], var["Ts"], var["Tt"], dloss, order)
    return dict(loss=loss.reshape(1), dstudent=dstudent, center_sum=csum)


def dino_spec(var):
    return dict(loss=("col", DINO_LOSS_BAR), dstudent=("row", DINO_GRAD_BAR[var["dtype"]]), center_sum=("sum", 0))


FAMILIES = {  # name: (cases, runs, ref, spec)
    "l2norm": (L2_CASES, l2_runs, l2_ref, l2_spec),
    "weight_norm": (WN_CASES, wn_runs, wn_ref, wn_spec),
    "bn_gelu": (BNG_CASES, bng_runs, bng_ref, bng_spec),
    "batchnorm_stats": ([(B, D) for B in STATS_B for D in STATS_D], stats_runs, stats_ref, stats_spec),
    "bn_stats_rows": ([(r, D) for r in STATS_ROWS for D in STATS_D], lambda r, D: stats_runs(r, D, (F32, BF16), "bn_stats_rows"), stats_ref, stats_spec),
    "bn_norm": (NORM_CASES, norm_runs, norm_ref, norm_spec),
    "bn_bwd_input": (BWD_CASES, bwd_runs, bwd_ref, bwd_spec),
    "softmax_xent": (XENT_CASES, xent_runs, xent_ref, xent_spec),
    "clip_total_norm": (CLIP_CASES, clip_runs, clip_ref, clip_spec),
    "dino_loss": (DINO_CASES, dino_runs, dino_ref, dino_spec),
}


def errors(key, inp, var, got, ref, spec):
    """{key + (figure,): (error, bar)} of the "row" and "col" figures that `got` holds; the "sum" figures are the caller's to bound."""
    out = {}
    for name, (how, default) in spec.items():
        if how == "sum" or name not in got:
            continue
        if how == "row":
            e = worst_row(got[name], ref[name])
        else:
            e = worst_col(got[name], ref[name], inp.get("mean_scale") if name == "mean" else None)
        out[key + (name,)] = (e, bar(key + (name,), default), default)
    return out


def sum_limits(inp, name, roundings):
    n, mag = inp["sum_terms"][name]
    return n, (sum_bound(n, mag) if roundings == 0 else product_sum_bound(n, roundings, mag))
