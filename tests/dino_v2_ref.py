"""Float64 yardstick of the DINOv2 additions: the Sinkhorn-Knopp teacher (direct exp / normalise form and the log-domain form the
kernels use), this project's DINO pairing and normalisation over a given teacher distribution q, and the KoLeo regulariser with its
gradient; the error bounds the GPU tests hold the kernels to, derived from the fp32 formats; and the inputs the tests share.

Sinkhorn-Knopp (DINOv2 sinkhorn_knopp_teacher): teacher logits t [R, K] on each of W ranks, N = R W rows in all, temperature T.
  direct: Q = exp(t / T)^T; Q /= sum(Q); n times { Q /= rowsum(Q) (over all ranks' samples); Q /= K; Q /= colsum(Q); Q /= N }; Q *= N
  log   : q[b,k] = exp(t[b,k] / T + lr[b] + lc[k] + log N), lr = 0, n times { lc[k] = -log K - logsumexp_b(t[b,k] / T + lr[b]);
          lr[b] = -log N - logsumexp_k(t[b,k] / T + lc[k]) }   (the first global normalisation cancels in the first column pass)
"""
import math

import numpy as np
import torch

EPS32 = 2.0 ** -24  # unit round-off of fp32 (half an ulp of 1)

SK_SHAPES = [(2, 4), (4, 1028), (6, 4100), (130, 2052)]  # K on either side of the 1024-column chunk and the 4-wide vector; R on either side of the 16-row split
KOLEO_SHAPES = [(2, 4), (3, 8), (65, 16), (64, 768), (130, 1028)]


# ---- Sinkhorn-Knopp ---------------------------------------------------------------------------------------------------------------------
def sk_direct(t, temp, n_iters=3, dtype=torch.float64):
    """q [R, K] by the exp / normalise form, one rank, in `dtype` (fp32 overflows once t / T > 88)."""
    Q = torch.exp(t.to(dtype) / temp).t()
    K, N = Q.shape
    Q = Q / Q.sum()
    for _ in range(n_iters):
        Q = Q / Q.sum(dim=1, keepdim=True)
        Q = Q / K
        Q = Q / Q.sum(dim=0, keepdim=True)
        Q = Q / N
    return (Q * N).t()


def sk_log(t, temp, n_iters=3, inv_temp=None):
    """(q [R, K], lr [R], lc [K]) by the log-domain form in float64, one rank.  `inv_temp`: the 1 / T the kernels multiply by (fp32(1) /
    fp32(T)) where the comparison is to be with their arithmetic and not with their rounding of T."""
    z = t.double() * (inv_temp if inv_temp is not None else 1.0 / temp)
    R, K = z.shape
    lr = torch.zeros(R, dtype=torch.float64)
    for _ in range(n_iters):
        lc = -math.log(K) - torch.logsumexp(z + lr[:, None], dim=0)
        lr = -math.log(R) - torch.logsumexp(z + lc[None, :], dim=1)
    return torch.exp(z + lr[:, None] + lc[None, :] + math.log(R)), lr, lc


def inv_temp32(temp):
    """1 / T as the library forms it: fp32(1) / fp32(T)."""
    return float(np.float32(1.0) / np.float32(temp))


def col_lse(t, inv_temp, lr=None):
    z = t.double() * inv_temp + (lr.double()[:, None] if lr is not None else 0.0)
    return torch.logsumexp(z, dim=0)


def row_lse(t, inv_temp, lc):
    return torch.logsumexp(t.double() * inv_temp + lc.double()[None, :], dim=1)


def lse_bound(arg_max, n_serial, lse):
    """Absolute error bound of a kernel's log-sum-exp against float64 on the same inputs.  Every term's argument t * (1 / T) + shift is one
    fused multiply-add of magnitude <= arg_max: one rounding, arg_max * 2^-24; the difference to the running maximum is another rounding of
    at most that size, and the fast exponential scales its argument by log2(e) in fp32, a third.  An absolute error e of an argument
    moves its exp, and so at most the whole sum, by the relative e: 3 arg_max 2^-24.  The sum itself: up to `n_serial` sequential
    additions in one thread, each with a rescaling multiply (2 roundings per step), then log2(256) = 8 merge levels of two multiplies and
    an add, the hardware exp and log at 2 ulp each: (2 n_serial + 3 * 8 + 8) * 2^-24 relative, which is the same absolute error of the
    log.  The result max + log(sum) is rounded once more: |lse| * 2^-24, doubled for the rounding of log(sum) before the add."""
    return (3.0 * arg_max + 2.0 * n_serial + 32.0 + 2.0 * np.abs(lse)) * EPS32


def sk_inputs(R, K, seed, scale=2.0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(R, K, generator=g) * scale).to(dtype)


# ---- this project's DINO loss over a given q ------------------------------------------------------------------------------------------
def dino_loss_from_q(student, q, ncrops, student_temp):
    """(loss, dstudent) of losses.py:63-91 with the teacher distribution q [2B, K] given: student [V B, K] crop-major, pairs (i, v != i),
    mean over the batch, divided by 2 (V - 1)."""
    s = student.double().clone().requires_grad_(True)
    B = q.shape[0] // 2
    logp = torch.log_softmax(s / student_temp, dim=-1).view(ncrops, B, -1)
    qq = q.double().view(2, B, -1)
    total, n = 0.0, 0
    for i in range(2):
        for v in range(ncrops):
            if v == i:
                continue
            total = total + (-(qq[i] * logp[v]).sum(dim=-1)).mean()
            n += 1
    loss = total / n
    (grad,) = torch.autograd.grad(loss, s)
    return loss.detach(), grad


# ---- KoLeo ----------------------------------------------------------------------------------------------------------------------------
def koleo(x, dloss=1.0):
    """(loss, dx, nn_index, dist, margin) in float64: DINOv2's KoLeoLoss written out, the gradient with the neighbour indices held constant,
    and the smallest best-minus-second-best cosine over the rows (how clear the reference's own choice of neighbours is; inf at n = 2)."""
    x = x.double()
    n = x.shape[0]
    norm = x.norm(dim=1).clamp_min(1e-8)
    xh = x / norm[:, None]
    dots = xh @ xh.t()
    dots.fill_diagonal_(-1.0)
    idx = dots.argmax(dim=1)  # torch: the first of equal maxima
    top = dots.topk(min(2, n - 1), dim=1).values
    margin = float((top[:, 0] - top[:, 1]).min()) if n > 2 else math.inf
    u = xh - xh[idx] + 1e-8
    d = u.norm(dim=1)
    loss = -torch.log(d + 1e-8).mean()
    G = (-dloss / (n * (d + 1e-8) * d))[:, None] * u
    dxh = G.clone()
    dxh.index_add_(0, idx, -G)  # the neighbour receives the negated gradient; several rows may share one
    dx = (dxh - xh * (xh * dxh).sum(dim=1, keepdim=True)) / norm[:, None]
    return loss, dx, idx, d, margin


KOLEO_BAR = {torch.float32: 1e-5, torch.bfloat16: 4e-3}  # the project's bars for a row kernel: fp32 arithmetic, values stored as bf16
UNIT_ROW_ERR = 8 * EPS32  # relative error of a normalised row: the sum of squares (rounded products, a short serial part, a tree), sqrt, reciprocal, scale


def koleo_bound(d_min, stored=torch.float32):
    """Relative error bound (against the row's largest element) of a KoLeo figure that depends on distances >= d_min.  The project's bar
    for a row kernel covers the norms, dots and rescaling of rows of unit scale.  KoLeo adds a difference of two unit rows, u = xh_i -
    xh_nn with |u| = d: the relative error UNIT_ROW_ERR of each unit row becomes UNIT_ROW_ERR / d relative in u, and the gradient holds
    d three times (u / ((d + eps) d)): 3 UNIT_ROW_ERR / d_min on top of the bar.  log(d) in the loss moves by the relative error of d."""
    return KOLEO_BAR[stored] + 3.0 * UNIT_ROW_ERR / float(d_min)


def koleo_inputs(n, D, seed, dtype=torch.float32, fan=True):
    """Rows with planted pairs, x_{2i+1} = x_{2i} + 0.3 noise (odd n: one free row), so that the nearest neighbour is clear; with `fan` and
    n >= 6 rows 1, 2 and 3 are row 0 plus steps of 0.10, 0.16 and 0.22 of its length instead, at right angles to it and to one another
    (cosines to row 0 of 0.995, 0.987, 0.977; to one another at most 0.983): each is closer to row 0 than to the others and row 0's own
    nearest is row 1, so row 0 is chosen by three rows (the gather path of the backward)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, D, generator=g)
    for i in range(n // 2):
        x[2 * i + 1] = x[2 * i] + 0.3 * torch.randn(D, generator=g)
    if fan and n >= 6:
        basis = [x[0].double() / x[0].double().norm()]
        for r, step in ((1, 0.10), (2, 0.16), (3, 0.22)):
            v = torch.randn(D, generator=g).double()
            for b in basis:
                v = v - (v @ b) * b
            basis.append(v / v.norm())
            x[r] = (x[0].double() + step * x[0].double().norm() * basis[-1]).float()
    return x.to(dtype)
