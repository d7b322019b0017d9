"""Yardstick of the iBOT masked patch-token loss on the HIP path: the masked input assembly and its backward in numpy, the loss and its
gradient in both teacher forms in float64 torch, the mask generator's contract, the backbone's masked forward in plain torch on
tests/dropout_ref.block (autograd supplies the gradients), and the loop limits of the new kernels.  Nothing here calls the code under
test.

Definitions.
  assembly   h0[b, 0] = cls;  h0[b, 1 + r] = reg[r];  h0[b, 1 + R + l] = (mask[b, l] ? mask_token : tok[b L + l]) + pos[l]
  backward   dtok[b L + l] = mask ? 0 : dh0[b, 1 + R + l];  dmask_token = sum over the masked (b, l) of dh0[b, 1 + R + l];
             dcls / dreg / dpos = the batch sums of the class / register / patch rows (the mask does not enter them)
  loss       q_i = softmax((t_i - center) / T_t)   or   q_i = exp(t_i / T_t + lr[i] + lc + log N)
             loss = -(1 / n_g) sum_i w_i sum_k q_ik log_softmax(s_i / T_s)_k
             ds_ik = dloss w_i / (n_g T_s) (softmax(s_i / T_s)_k - q_ik);   center_sum[k] = sum_i t_ik
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import mae_oracle as O
from tests import dropout_ref as R

F64 = torch.float64

# loop limits of the kernels (csrc/elementwise.hip, csrc/dino.hip)
ASM_FWD_BLOCK = 256         # float4s per block of the forward: a row of D / 4 float4s may straddle two blocks
ASM_COLS_PER_TRIP = 1024    # 256 threads x 4 columns: D above it takes a second trip of the per-row column loops
MASK_ROWS_PER_BLOCK = 128   # level 1 of the dmask_token reduction: patch rows one block adds in row order
MASK_FOLD_BATCH = 8         # level 2: partials loaded per trip of the in-order fold
LOSS_CHUNK = 1024           # columns per block of ibot_loss_grad_kernel and per trip of dino_row_stats_kernel
LOSS_ROWS_PER_SPLIT = 64    # rows one block of ibot_loss_grad_kernel walks; the splits' partials are folded in order
HEAD_ROW_MULTIPLE = 16


# ---- assembly ------------------------------------------------------------------------------------------------------------------------
def assemble_fwd(tok, cls, reg, pos, mask_token, mask):
    """fp32 numpy.  tok [B*L, D] (fp32 values), cls [D], reg [R, D] or None, pos [L, D] or None, mask_token [D], mask [B, L] -> h0
    [B, 1 + R + L, D]: one fp32 add per patch element."""
    tok = np.asarray(tok, dtype=np.float32)
    B, L = mask.shape
    D = tok.shape[1]
    Rn = 0 if reg is None else reg.shape[0]
    h0 = np.zeros((B, 1 + Rn + L, D), dtype=np.float32)
    for b in range(B):
        h0[b, 0] = cls
        for r in range(Rn):
            h0[b, 1 + r] = reg[r]
        for l in range(L):
            row = np.asarray(mask_token, dtype=np.float32) if mask[b, l] else tok[b * L + l]
            h0[b, 1 + Rn + l] = row if pos is None else row + np.asarray(pos, dtype=np.float32)[l]
    return h0


def assemble_bwd(dh0, mask, Rn):
    """dh0 [B, 1 + R + L, D], mask [B, L] -> dict(dtok [B*L, D], dcls, dreg, dpos, dmask_token) in float64 and `abs`, the same sums over
    |terms| (what product_sum_bound takes), and `n_masked`."""
    dh0 = np.asarray(dh0, dtype=np.float64)
    B, L = mask.shape
    D = dh0.shape[2]
    patch = dh0[:, 1 + Rn:, :]
    m = np.asarray(mask, dtype=bool)
    out = dict(dtok=np.where(m[:, :, None], 0.0, patch).reshape(B * L, D), dcls=dh0[:, 0].sum(0), dreg=dh0[:, 1:1 + Rn].sum(0), dpos=patch.sum(0),
               dmask_token=(patch * m[:, :, None]).sum((0, 1)))
    out["abs"] = dict(dcls=np.abs(dh0[:, 0]).sum(0), dreg=np.abs(dh0[:, 1:1 + Rn]).sum(0), dpos=np.abs(patch).sum(0),
                      dmask_token=(np.abs(patch) * m[:, :, None]).sum((0, 1)))
    out["n_masked"] = int(m.sum())
    return out


MASK_PATTERNS = ("none", "one", "sample", "never", "all")


def mask_pattern(kind, B, L, seed=0):
    """uint8 [B, L].  none: nothing masked; one: a single patch; sample: all of one sample and nothing else; never: random, but one
    position that no sample masks (and one that all do, for L > 2); all: everything."""
    g = np.random.default_rng(seed)
    m = np.zeros((B, L), dtype=np.uint8)
    if kind == "one":
        m[B - 1, L // 2] = 1
    elif kind == "sample":
        m[B // 2] = 1
    elif kind == "never":
        m = (g.random((B, L)) < 0.5).astype(np.uint8)
        m[:, L // 3] = 0
        if L > 2:
            m[:, L - 1] = 1
    elif kind == "all":
        m[:] = 1
    elif kind != "none":
        raise ValueError(kind)
    return m


ASM_B, ASM_L, ASM_R, ASM_D = 3, 27, (0, 2), (4, 260)
# crosses both levels of the dmask_token reduction and the column trip: 5 * 216 = 1080 patch rows = 9 blocks of 128 (the last one ragged,
# 56 rows), 9 partials = one full fold batch of 8 and a ragged one; D = 1028 = a second trip of the 256-thread column loop
ASM_BIG = dict(B=5, L=216, R=1, D=1028)


# ---- loss ------------------------------------------------------------------------------------------------------------------------------
def inv_temp32(temp):
    """1 / T as the library forms it, fp32(1) / fp32(T), where the comparison is to be with the kernels' arithmetic and not with their
    rounding of T (tests/dino_v2_ref.py does the same)."""
    return float(np.float32(1.0) / np.float32(temp))


def ibot_loss(student, teacher, weight, inv_images, Ts, Tt, center=None, sk=None, dloss=1.0, inv32=False):
    """(loss, dstudent [M, K], center_sum [K]) in the dtype of `student` (float64 for the reference).  `center` [K]: the centering form;
    `sk` = (lc [K], lr [M], log_n): the Sinkhorn-Knopp form (q is not renormalised, as the formula says).  `inv32`: multiply by
    inv_temp32(T) in the place of dividing by T."""
    dt = student.dtype
    s, t, w = student, teacher.to(dt), weight.to(dt)
    its, itt = (inv_temp32(Ts), inv_temp32(Tt)) if inv32 else (1.0 / Ts, 1.0 / Tt)
    logp = torch.log_softmax(s * its, dim=1)
    if sk is None:
        q = torch.softmax((t - center.to(dt)) * itt, dim=1)
    else:
        lc, lr, log_n = sk
        q = torch.exp(t * itt + lr.to(dt)[:, None] + lc.to(dt)[None, :] + log_n)
    loss = -(inv_images) * (w * (q * logp).sum(dim=1)).sum()
    ds = dloss * (w * inv_images * its)[:, None] * (logp.exp() - q)
    return loss, ds, t.sum(dim=0)


def sk_logs(teacher, Tt, n_iters, n_total=None, inv32=False):
    """(lc, lr, log N) of the Sinkhorn-Knopp teacher in float64, alternating from lr = 0 (csrc/dino.hip's definition)."""
    t = teacher.double() * (inv_temp32(Tt) if inv32 else 1.0 / Tt)
    M, K = t.shape
    log_n = math.log(M if n_total is None else n_total)
    lr = torch.zeros(M, dtype=F64)
    for _ in range(n_iters):
        lc = -math.log(K) - torch.logsumexp(t + lr[:, None], dim=0)
        lr = -log_n - torch.logsumexp(t + lc[None, :], dim=1)
    return lc, lr, log_n


LOSS_SHAPES = [(1, 4), (3, 1028), (37, 2052), (130, 2052),
               (64, 1024), (65, 1024)]  # one full row split and one chunk exactly; one row into the second split
LOSS_SCALES = (1.0, 8.0)


def loss_inputs(M, K, scale, dtype, seed=0):
    """Logits rounded to `dtype` (the reference reads the rounded values), weights that differ per row with one of them 0 (M > 1), a
    centre of realistic size."""
    g = torch.Generator().manual_seed(1000 * M + K + seed)
    amp = scale * (1.0 if K >= 1000 else 0.05)  # four columns: unit logits over T = 0.04 are one-hot and c p - q cancels (head_kernels_ref.dino_inputs)
    student = (torch.randn(M, K, generator=g) * amp).to(dtype)
    teacher = (torch.randn(M, K, generator=g) * amp).to(dtype)
    weight = 1.0 / torch.randint(1, 60, (M,), generator=g).float()
    if M > 1:
        weight[M // 2] = 0.0
    center = 0.1 * torch.randn(K, generator=g)
    return dict(student=student, teacher=teacher, weight=weight, center=center)


# ---- generator -------------------------------------------------------------------------------------------------------------------------
def generator_contract(masks, n_g, L, ratio, sample_prob):
    """Checks one draw against the contract; returns the sorted counts of the masked samples."""
    masks = np.asarray(masks)
    assert masks.shape == (n_g, L) and masks.dtype == np.uint8 and set(np.unique(masks)) <= {0, 1}
    n_m = int(n_g * sample_prob)
    counts = masks.sum(axis=1)
    got = np.sort(counts[counts > 0])
    assert len(got) == n_m, (got, n_m)
    edges = np.linspace(ratio[0], ratio[1], n_m + 1)
    for j, c in enumerate(got):  # the sub-intervals rise, so do the targets: sorted counts meet them one by one
        lo, hi = max(1, int(L * edges[j])), max(1, int(L * edges[j + 1]))
        assert lo <= c <= hi, (j, c, lo, hi)
    return got


def rows_and_weights(masks, Rn):
    """Brute force: (rows, weights) of the masked tokens, (b, l) in row-major order."""
    n_g, L = masks.shape
    rows, weights = [], []
    for b in range(n_g):
        c = int(masks[b].sum())
        for l in range(L):
            if masks[b, l]:
                rows.append(b * (1 + Rn + L) + 1 + Rn + l)
                weights.append(np.float32(1.0 / c))
    return np.asarray(rows, dtype=np.int32), np.asarray(weights, dtype=np.float32)


# ---- the backbone ----------------------------------------------------------------------------------------------------------------------
def vit_forward_masked(p, x, mask, patch_size, heads, layers, masks):
    """Forward of the backbone with masked patches: tokens [B, 1 + R + L, D].  `mask` [B, L] bool tensor or None; `masks` the dropout /
    drop-path masks as in dropout_ref.  With mask None this is patch_dropout_ref.vit_forward_keep at rate 0 term for term.  Under O._EMU
    the values the bf16 path stores are rounded where it stores them; mask_token, like cls_token, stays fp32."""
    B = x.shape[0]
    r = O._r
    tok = F.conv3d(r(x), r(p["patch_embedding.patch_embeddings.weight"]), p["patch_embedding.patch_embeddings.bias"], stride=patch_size)
    tok = r(tok.flatten(2).transpose(-1, -2))
    L, D = tok.shape[1], tok.shape[2]
    if mask is not None:
        tok = torch.where(mask[:, :, None], p["mask_token"].reshape(1, 1, D).expand(B, L, D), tok)
    if "patch_embedding.position_embeddings" in p:
        tok = tok + p["patch_embedding.position_embeddings"]
    Rn = p["register_tokens"].shape[1] if "register_tokens" in p else 0
    z0 = masks.stream(0, (B, 1 + Rn + L, D))
    tok = tok * (z0[:, 1 + Rn:, :] if z0.dim() else z0)
    h = torch.cat((p["cls_token"].expand(B, -1, -1), tok), dim=1)
    if Rn:
        h = torch.cat((h[:, :1], p["register_tokens"].expand(B, -1, -1), h[:, 1:]), dim=1)
    for i in range(layers):
        h = R.block(p, f"blocks.{i}", h, heads, masks, 1 + 4 * i)
    return r(F.layer_norm(h, (h.shape[-1],), p["norm.weight"], p["norm.bias"], 1e-6))


# 24^3 volumes, patch 12 (8 patches), width 48, two blocks: the tiny backbone of tests/test_patch_dropout_gpu.py's entry-point test
TINY_CASE = dict(in_chans=1, img_size=24, patch_size=12, hidden_size=48, mlp_dim=96, num_layers=2, num_heads=3, num_register_tokens=1,
                 qkv_bias=True, batch=3, seed=512, x_seed=91)


def case_mask(case, L, seed=3):
    """bool [B, L]: sample 0 unmasked, the others at random with at least one masked and one seen patch each."""
    g = torch.Generator().manual_seed(seed + L)
    m = torch.rand(case["batch"], L, generator=g) < 0.4
    m[0] = False
    m[1:, 0] = True
    m[1:, 1] = False
    return m
