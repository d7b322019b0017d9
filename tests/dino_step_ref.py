"""The DINO step held per row and per column: a float64 restatement of engine_pretrain_dino._forward_loss plus the backward, with every
switch the engine offers (BatchNorm heads, Sinkhorn-Knopp centering, the iBOT patch loss on explicit masks, KoLeo, the last layer
frozen or trained), its yardsticks and the inputs the tests share.  The measure is tests/step_ref.py's, unchanged: E, E_rows, ratios,
worst and plant are imported from there.  Nothing here calls the code under test.

Composition.  backbone: `tokens` = step_ref.vit_tokens with ibot_ref.vit_forward_masked's assembly (a masked patch enters as mask_token +
pos) on lora_ref.block, the block of the plan that runs without dropout;  head: dino_oracle.dino_head_forward's arithmetic with the
device's storage points;  losses: dino_oracle.dino_loss's pairing over a teacher distribution q (softmax((t - c) / T) or the
Sinkhorn-Knopp q of ibot_ref.sk_logs), ibot_ref.ibot_loss, dino_v2_ref.koleo's formula.  The three helpers that dino_v2_ref / ibot_ref
only have in float64 (`sk_logs`, `dino_from_q`, `koleo`) are restated here in the caller's dtype, because the fp32 yardstick needs the
whole step in fp32; tests/test_dino_step_ref_cpu.py ties each of them to its float64 original at 1e-12.

bf16-storage emulation (`emulate=True`): values are rounded to bfloat16 exactly where the device's FORWARD stores bf16.
  backbone   the points step_ref.vit_tokens documents (patch-embedding operands and output, the blocks' stores, the final norm's output);
             cls_token, register_tokens, mask_token and the position table stay fp32
  head       (_HeadFunction.forward) the input rows; the working weights W of the three Linears; u1 / u2 = x W^T + b as the GELU's SAVED
             input (the GELU itself is evaluated on the unrounded accumulator, its derivative in the backward on the stored bf16 value:
             `_GeluSavedRounded`); h1, h2; zn = z / |z|; wn = g v / |v|; the logits.  z stays fp32.  Under BatchNorm the Linear's
             output, the statistics, xhat and the saved GELU derivative stay fp32 and only h1 / h2 are rounded.
  teacher    the same.  The losses read the logits as stored, KoLeo the class tokens as stored.
The device also rounds backward intermediates (dlogits, dz, du); the emulation does not, as in step_ref.

Yardsticks as in step_ref: Y32 = E(this file in fp32, in fp64); Ybf = E(bf16-storage run in fp64, plain run in fp64).  Margins below.

Scalars (the loss and its parts).  A scalar has one slice, so its yardstick is a single draw of a difference, and a draw can fall far below
the sites it stands for: measured on the device, the fp32 runs' losses lay within 3.4e-7 of the reference while Y32 came to 3.6e-9 in one
setting (E / Y 95), and in bf16 mode within 1.3e-5 while Ybf came to 4e-8 to 7e-7 in the Sinkhorn-Knopp and iBOT settings (E / Y up to 58),
below even what one fp32 rounding of the loss costs.  The gradients of the same runs stayed within 2.9 x Y32 and 1.1 x Ybf.  What the draw
understates are legitimate rounding sites, and the scalar yardsticks gain them, from the reference side alone:
  fp32 mode   + 2^-25: the loss is stored as one fp32 number, and a correctly rounded copy of the reference lies up to there in E's terms.
  bf16 mode   + E(bf16-storage run in fp32, the same in fp64): the fp32 arithmetic between the bf16 stores, which now and then tips a store to
              the neighbouring bf16 value (tests/test_step_ref_cpu.py leaves the scalar out of its stand-in check for this reason);
              + the RMS cost of the last stores the part reads (the student's and the teacher's logits for the DINO and iBOT terms, the class
              tokens for KoLeo):
              sqrt(sum_ij (d part / d x_ij * spacing(x_ij) / sqrt(12))^2) / (2 |part|), a derived figure that is no draw (`bf16_store_rms`).
Tensors with more than one slice keep the yardstick of step_ref unchanged: their worst slice is a maximum over many draws.

Mathematically-zero tensors.  With use_bn the gradient of a Linear bias b in front of a BatchNorm is zero in exact arithmetic: BatchNorm
subtracts the batch mean, so the loss does not depend on b, and db[k] = sum_r du[r, k] with du the gradient at the Linear's output.
step_ref._family would measure such a tensor on its own scale, which is zero.  They are held absolutely (`zero_bias_bounds`):
  fp32 mode   max |g| <= M32_DINO * max |g of this file run in fp32|: the fp32 run's own round-off of the same column sums.
  bf16 mode   the device stores du in bf16 before hct_colsum adds its rows.  Write the stored value du'[r, k] = du[r, k] (1 + d_rk) with
              |d_rk| <= u = 2^-8, the unit round-off of bfloat16 (8 significant bits, round to nearest).  The BatchNorm backward makes
              sum_r du[r, k] = 0 whatever its input (sum_r xhat = 0 and sum_r xhat^2 = n), so
                  |db[k]| = |sum_r du[r, k] d_rk| <= u sum_r |du[r, k]|
              and the fp32 additions of at most n <= 16 terms add n 2^-24 of the same sum, 1/4096 of the bound.  du is taken from the
              reference (the bf16-storage run in fp64); the device's du is its own, within the distance that MBF_DINO allows every other
              tensor, so the bound is beta[k] = MBF_DINO * u * sum_r |du_ref[r, k]| per column k.
              backbone.norm.bias: the class-token rows are the only rows of the final norm's output with a gradient, dx = du' W0' (fp32),
              so sum_r dx[r, j] = sum_k db0[k] W0'[k, j], at most sum_k beta[k] |W0'[k, j]|; the backbone's backward then reads dx in bf16,
              which adds u sum_r |dx[r, j]| in the same way:  MBF_DINO * u * sum_r |dx_ref[r, j]| + sum_k beta[k] |W0'[k, j]|.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import dino_oracle as D
from oracle import mae_oracle as O
from tests import ibot_ref as IR
from tests import lora_ref
from tests.step_ref import E, E_rows, plant, ratios, worst  # noqa: F401  (the measure, re-exported unchanged)

# Margins (E <= M * Y), the rule of step_ref: start at 4 / 2; raised to the next power of two at or above twice the worst ratio measured
# on the device, never above the caps, which are conditions (tests/test_dino_step_ref_cpu.py re-proves the planted faults at them).
# Measured ratios (worst fp32 10.18, a scalar; worst bf16 3.34): the docstring of tests/test_dino_step_rows_gpu.py and DESIGN.md section 3.
M32_DINO, MBF_DINO = 32.0, 4.0
M32_DINO_CAP, MBF_DINO_CAP = 256.0, 4.0
START_M32, START_MBF = 4.0, 2.0

U_BF16 = 2.0 ** -8  # unit round-off of bfloat16
STUDENT_TEMP, TEACHER_TEMP, CENTER_MOMENTUM, SK_ITERS = 0.1, 0.04, 0.9, 3  # (epoch 0 of DINOLoss(.., 0.04, 0.07, 3, 10))

# ---- cases -------------------------------------------------------------------------------------------------------------------------------
_SMALL_VIT = dict(in_chans=3, img_size=24, patch_size=12, hidden_size=48, mlp_dim=96, num_layers=2, num_heads=3, pos_embed="sincos",
                  num_register_tokens=4, qkv_bias=True)  # the backbone of tests/golden/dino.json["step"]
_TILE_VIT = dict(in_chans=1, img_size=48, patch_size=16, hidden_size=768, mlp_dim=3072, num_layers=1, num_heads=12, pos_embed="learnable",
                 num_register_tokens=2, qkv_bias=True)  # step_ref.VIT_TILE_CASE's backbone
# x4 on the qkv matrices of the one-block backbone (U(-0.08, 0.08), about Xavier's bound at width 768): at make_vit_params' 0.02 its
# attention is uniform, every patch token reaches the class token alike, the rows of the position table's gradient agree to 8 % and two
# swapped rows are a fault too small for any check.  The width-48 backbone takes x8 on all four matrices of a block (U(-0.16, 0.16); Xavier's
# bound at that width is 0.25): at x1 its class-token rows are parallel to 6e-4 in the cosine, a BatchNorm over 8 such rows divides by
# almost nothing, and the bf16 stores alone then move the gradients by twice their size (Ybf 2.2), a yardstick that holds nothing.
QKV_SCALE = {"small": 8.0, "tile16": 4.0, "tile15": 4.0}
BLOCK_SCALE = {"small": 8.0, "tile16": 1.0, "tile15": 1.0}  # on the blocks' other matrices (proj, linear1, linear2)
_TILE_HEAD = dict(hidden_dim=2048, bottleneck_dim=256, out_dim=4100)  # past the loss kernels' 1024-column chunks, a 4-wide tail
CASES = {
    "small": dict(vit=_SMALL_VIT, head=dict(hidden_dim=64, bottleneck_dim=32, out_dim=128), crops=4, batch=2, seed=40),
    "tile16": dict(vit=_TILE_VIT, head=_TILE_HEAD, crops=4, batch=4, seed=50),  # 16 head rows: the split-K dgrad of the prototype layer in bf16
    "tile15": dict(vit=_TILE_VIT, head=_TILE_HEAD, crops=3, batch=5, seed=60),  # 15 head rows: the NT fallback
}
# masked patches per global sample (2 * batch of them): sample 0 unmasked, sample 1 a single patch, the rest about a third of L.
#   "ragged": class rows + masked rows is no multiple of 16 (padding repeats);  "exact": it is one
MASK_COUNTS = {
    ("small", "ragged"): [0, 1, 3, 3],                          # 8 + 7 = 15
    ("small", "exact"): [0, 1, 3, 4],                           # 8 + 8 = 16
    ("tile16", "ragged"): [0, 1, 9, 9, 9, 9, 9, 9],             # 16 + 55 = 71
    ("tile16", "exact"): [0, 1, 10, 10, 11, 11, 10, 11],        # 16 + 64 = 80
    ("tile15", "ragged"): [0, 1, 9, 9, 9, 9, 9, 9, 9, 9],       # 15 + 73 = 88 = 5.5 * 16
    ("tile15", "exact"): [0, 1, 10, 10, 10, 10, 10, 10, 10, 10],  # 15 + 81 = 96
}
IBOT_WEIGHT, KOLEO_WEIGHT = 1.0, 0.1
SETTINGS = {
    "plain": dict(),
    "bn": dict(use_bn=True),
    "sk": dict(centering="sinkhorn_knopp"),
    "ibot-ragged": dict(ibot_weight=IBOT_WEIGHT, masks="ragged"),
    "ibot-exact": dict(ibot_weight=IBOT_WEIGHT, masks="exact"),
    "ibot-sk-ragged": dict(ibot_weight=IBOT_WEIGHT, masks="ragged", centering="sinkhorn_knopp"),
    "ibot-sk-exact": dict(ibot_weight=IBOT_WEIGHT, masks="exact", centering="sinkhorn_knopp"),
    "koleo": dict(koleo_weight=KOLEO_WEIGHT),
    "v2": dict(centering="sinkhorn_knopp", ibot_weight=IBOT_WEIGHT, masks="ragged", koleo_weight=KOLEO_WEIGHT),  # the DINOv2 recipe
}


def num_patches(vit):
    return (vit["img_size"] // vit["patch_size"]) ** 3


def backbone_shapes(vit, mask_token=False):
    """Names and shapes of ViTBackbone's state dict (the reference ViT's), written out so that the CPU tests need no device module; the
    GPU test asserts that the module's own state dict has exactly these."""
    Dm, Md, P, C = vit["hidden_size"], vit["mlp_dim"], vit["patch_size"], vit["in_chans"]
    out = {"cls_token": (1, 1, Dm), "register_tokens": (1, vit["num_register_tokens"], Dm),
           "patch_embedding.position_embeddings": (1, num_patches(vit), Dm),
           "patch_embedding.patch_embeddings.weight": (Dm, C, P, P, P), "patch_embedding.patch_embeddings.bias": (Dm,),
           "norm.weight": (Dm,), "norm.bias": (Dm,)}
    for i in range(vit["num_layers"]):
        b = f"blocks.{i}."
        out.update({b + "mlp.linear1.weight": (Md, Dm), b + "mlp.linear1.bias": (Md,), b + "mlp.linear2.weight": (Dm, Md), b + "mlp.linear2.bias": (Dm,),
                    b + "att_norm.weight": (Dm,), b + "att_norm.bias": (Dm,), b + "ffn_norm.weight": (Dm,), b + "ffn_norm.bias": (Dm,),
                    b + "attn.qkv.weight": (3 * Dm, Dm), b + "attn.qkv.bias": (3 * Dm,), b + "attn.proj.weight": (Dm, Dm), b + "attn.proj.bias": (Dm,)})
    if mask_token:
        out["mask_token"] = (1, Dm)
    return out


def make_backbone_params(vit, seed, mask_token=False, qkv_scale=1.0, block_scale=1.0):
    """O.make_vit_params by seed; the register and mask tokens x5 (tokens of the embeddings' size, as tests/test_ibot_gpu.py).  The class
    token keeps its size: at x5 it outweighs what one block adds to its row, and the class-token rows of all samples come out parallel
    to 1e-4 in the cosine, which leaves KoLeo no clear neighbour.  `qkv_scale`: QKV_SCALE."""
    p = O.make_vit_params(backbone_shapes(vit, mask_token), seed)
    for k in p:
        if k in ("register_tokens", "mask_token"):
            p[k] = p[k] * 5.0
        if k.endswith("attn.qkv.weight"):
            p[k] = p[k] * qkv_scale
        if k.endswith(("attn.proj.weight", "mlp.linear1.weight", "mlp.linear2.weight")):
            p[k] = p[k] * block_scale
    return p


def head_keys(use_bn):
    lin = (0, 3, 6) if use_bn else (0, 2, 4)
    return lin, ((1, 4) if use_bn else ())


def make_head_params_scaled(in_dim, head, seed0, use_bn=False):
    """DINOHead state dict in the module's key order with zero-mean, fan-in-scaled matrices: W = U(-1, 1) / sqrt(fan_in / 3), unit
    variance per output for unit-variance inputs, so the GELUs stay alive at any width (dino_oracle.make_head_params draws from
    [-0.6, 0.2), mean -0.2: at hidden 2048 every GELU input lies below -6 and the gradient is exactly zero from mlp.4.weight back).
    Vectors U(-0.05, 0.05), BatchNorm weights U(0.5, 1.5), weight_g = 1, BatchNorm buffers at their initial values."""
    H, Bn, K = head["hidden_dim"], head["bottleneck_dim"], head["out_dim"]
    lin, bn = head_keys(use_bn)
    dims = {lin[0]: (H, in_dim), lin[1]: (H, H), lin[2]: (Bn, H)}
    out, i = {}, 0

    def u(shape):
        nonlocal i
        i += 1
        return torch.from_numpy(O.hash_uniform(int(np.prod(shape)), seed0 + i)).float().reshape(shape)

    for j in range(lin[2] + 1):
        if j in dims:
            out[f"mlp.{j}.weight"] = u(dims[j]) / (dims[j][1] / 3.0) ** 0.5
            out[f"mlp.{j}.bias"] = u((dims[j][0],)) * 0.05
        elif j in bn:
            out[f"mlp.{j}.weight"] = 1.0 + 0.5 * u((H,))
            out[f"mlp.{j}.bias"] = u((H,)) * 0.05
            out[f"mlp.{j}.running_mean"], out[f"mlp.{j}.running_var"] = torch.zeros(H), torch.ones(H)
            out[f"mlp.{j}.num_batches_tracked"] = torch.tensor(0, dtype=torch.long)
    out["last_layer.weight_g"] = torch.ones(K, 1)
    out["last_layer.weight_v"] = u((K, Bn)) / (Bn / 3.0) ** 0.5
    return out


def hu(shape, seed, lo, hi):
    """tests/test_dino_gpu.py::_hu: hash_uniform * (hi - lo) + lo."""
    return torch.from_numpy(O.hash_uniform(int(np.prod(shape)), seed)).float().reshape(shape) * (hi - lo) + lo


def make_crops(case, seed0):
    """V crops [B, C, S, S, S] in [-1, 1) (zero-mean, as the fixture's: a common mean would make every token alike).  Even samples are hash noise; an odd sample b is 0.6 * sample b - 1 + 0.4 * its own noise (cosine 0.83 to its partner), and the last
    sample of an odd batch, which has no partner, 0.5 * its predecessor + 0.5 * noise (cosine 0.71 to it, 0.59 to that one's partner):
    every sample has one clearly nearest neighbour (1 <-> 0, 3 <-> 2, 4 -> 3), as dino_v2_ref.koleo_inputs plants pairs, so that KoLeo's
    choice does not hang on the rounding."""
    vit, B = case["vit"], case["batch"]
    shape = (B, vit["in_chans"]) + (vit["img_size"],) * 3
    out = []
    for v in range(case["crops"]):
        x = hu(shape, seed0 + v, 0.0, 1.0)
        for b in range(1, B):
            a = 0.6 if b % 2 else (0.5 if b == B - 1 else 0.0)
            x[b] = a * x[b - 1] + (1.0 - a) * x[b]
        out.append(x)
    return out


def make_masks(case_name, variant):
    """Explicit host masks uint8 [2 * batch, L] with MASK_COUNTS[case, variant] masked patches per sample, positions by a seeded draw."""
    case = CASES[case_name]
    L, counts = num_patches(case["vit"]), MASK_COUNTS[(case_name, variant)]
    assert len(counts) == 2 * case["batch"]
    g = np.random.default_rng(1000 + case["seed"])
    m = np.zeros((len(counts), L), dtype=np.uint8)
    for b, c in enumerate(counts):
        m[b, g.permutation(L)[:c]] = 1
    return m


# ---- pieces in the caller's dtype ---------------------------------------------------------------------------------------------------------
class _GeluSavedRounded(torch.autograd.Function):
    """gelu(u) in the forward; the backward multiplies by gelu'(bf16(u)): the device keeps the pre-activation in bf16 for its backward."""

    @staticmethod
    def forward(ctx, u):
        ctx.save_for_backward(u.bfloat16().to(u.dtype))
        return F.gelu(u)

    @staticmethod
    def backward(ctx, g):
        (us,) = ctx.saved_tensors
        cdf = 0.5 * (1.0 + torch.erf(us * 2.0 ** -0.5))
        pdf = torch.exp(-0.5 * us * us) * (2.0 * np.pi) ** -0.5
        return g * (cdf + us * pdf)


def bf16_store_rms(x):
    """RMS error of rounding x to bfloat16, element by element: the spacing at x is 2^(floor(log2 |x|) - 7), round to nearest leaves an
    error uniform in +- half of it, whose RMS is the spacing / sqrt(12)."""
    return torch.where(x == 0, torch.zeros_like(x), torch.exp2(torch.floor(torch.log2(x.abs().clamp_min(1e-300))) - 7.0) / 12.0 ** 0.5)


def tokens(p, x, vit, mask=None, emulate=False):
    """step_ref.vit_tokens (LayerNorm) with ibot_ref.vit_forward_masked's assembly: `mask` bool [B, L] or None."""
    old_emu, old_block = O._EMU[0], O._block
    O._EMU[0], O._block = bool(emulate), lora_ref.block
    try:
        B = x.shape[0]
        pe = "patch_embedding.patch_embeddings"
        tok = F.conv3d(O._r(x), O._r(p[pe + ".weight"]), p[pe + ".bias"], stride=vit["patch_size"])
        tok = O._r(tok.flatten(2).transpose(-1, -2))
        if mask is not None:
            tok = torch.where(mask[:, :, None], p["mask_token"].reshape(1, 1, -1).expand_as(tok), tok)
        tok = tok + p["patch_embedding.position_embeddings"]
        h = torch.cat((p["cls_token"].expand(B, -1, -1), p["register_tokens"].expand(B, -1, -1), tok), dim=1)
        for i in range(vit["num_layers"]):
            h = O._block(p, f"blocks.{i}", h, vit["num_heads"], None, "")
        return O._r(F.layer_norm(h, (h.shape[-1],), p["norm.weight"], p["norm.bias"], 1e-6))
    finally:
        O._EMU[0], O._block = old_emu, old_block


def head_forward(p, x, emulate=False, keep=None):
    """dino_oracle.dino_head_forward in training mode, in x's dtype, with the storage points of the module docstring.  BatchNorm buffers in
    `p` move in place (pass copies).  `keep`, a dict, receives "u": the two Linear outputs in front of the BatchNorms / GELUs (their .grad
    is d loss / du after the backward) and "gelu_in": what the two GELUs read."""
    r = (lambda t: t.bfloat16().to(t.dtype)) if emulate else (lambda t: t)
    use_bn = "mlp.1.weight" in p
    lin, bn = head_keys(use_bn)
    h = r(x)
    for li in lin[:2]:
        u = a = F.linear(h, r(p[f"mlp.{li}.weight"]), p[f"mlp.{li}.bias"])
        if use_bn:
            b = f"mlp.{li + 1}."
            a = D.batchnorm_train(u, p[b + "weight"], p[b + "bias"], p[b + "running_mean"], p[b + "running_var"])
            h = r(F.gelu(a))
        else:
            h = r(_GeluSavedRounded.apply(u) if emulate else F.gelu(u))
        if keep is not None:
            if u.requires_grad:
                u.retain_grad()
            keep.setdefault("u", []).append(u)
            keep.setdefault("gelu_in", []).append(a.detach())
    z = F.linear(h, r(p[f"mlp.{lin[2]}.weight"]), p[f"mlp.{lin[2]}.bias"])
    zn = r(F.normalize(z, dim=-1, p=2))
    v, g = p["last_layer.weight_v"], p["last_layer.weight_g"]
    wn = r(g * v / v.norm(dim=1, keepdim=True))
    return r(F.linear(zn, wn))


def sk_logs(t, temp, n_iters, n_total=None):
    """ibot_ref.sk_logs (= dino_v2_ref.sk_log's lr, lc) in t's dtype."""
    z = t / temp
    M, K = z.shape
    log_n, log_k = float(np.log(M if n_total is None else n_total)), float(np.log(K))
    lr = torch.zeros(M, dtype=t.dtype)
    for _ in range(n_iters):
        lc = -log_k - torch.logsumexp(z + lr[:, None], dim=0)
        lr = -log_n - torch.logsumexp(z + lc[None, :], dim=1)
    return lc, lr, log_n


def teacher_q(t, temp, center=None, sk_iters=None):
    """The DINO term's teacher distribution [2B, K]: softmax((t - center) / T), or the Sinkhorn-Knopp q over the 2B rows."""
    if sk_iters is None:
        return F.softmax((t - center) / temp, dim=-1)
    lc, lr, log_n = sk_logs(t, temp, sk_iters)
    return torch.exp(t / temp + lr[:, None] + lc[None, :] + log_n)


def dino_from_q(student, q, ncrops, student_temp):
    """dino_oracle.dino_loss's pairing over a given q (dino_v2_ref.dino_loss_from_q), differentiable, in the student's dtype."""
    s = (student / student_temp).chunk(ncrops)
    total, n = 0.0, 0
    for iq, qi in enumerate(q.chunk(2)):
        for v in range(ncrops):
            if v == iq:
                continue
            total = total + torch.sum(-qi * F.log_softmax(s[v], dim=-1), dim=-1).mean()
            n += 1
    return total / n


def koleo(x):
    """(loss, nearest-neighbour index, smallest best-minus-second cosine, the cosines with -1 on the diagonal) of dino_v2_ref.koleo,
    differentiable (the neighbours constant), in x's dtype."""
    n = x.shape[0]
    xh = x / x.norm(dim=1).clamp_min(1e-8)[:, None]
    dots = (xh @ xh.t()).detach().clone()
    dots.fill_diagonal_(-1.0)
    idx = dots.argmax(dim=1)
    top = dots.topk(min(2, n - 1), dim=1).values
    margin = float((top[:, 0] - top[:, 1]).min()) if n > 2 else float("inf")
    d = (xh - xh[idx] + 1e-8).norm(dim=1)
    return -torch.log(d + 1e-8).mean(), idx, margin, dots


# ---- the case object ----------------------------------------------------------------------------------------------------------------------
_REF = {}
_RUNS = {}  # (case, setting) -> {(precision, emulate): run}: the frozen and the trained last layer share their runs


class DinoRef:
    """One case in one setting.  Switches: use_bn, centering, ibot_weight (+ the masks' variant), koleo_weight, freeze_last_layer.
    `params`: None (this file's initialisers by the case's seed) or dict(student_backbone, student_head, teacher_backbone, teacher_head,
    crops, center) to run somebody else's inputs (the fixture's, for the agreement test)."""

    def __init__(self, case_name, use_bn=False, centering="centering", ibot_weight=0.0, masks=None, koleo_weight=0.0, freeze_last_layer=True,
                 params=None, runs=None):
        case = CASES[case_name]
        self.name, self.case, self.vit, self.head = case_name, case, case["vit"], case["head"]
        self.V, self.B = case["crops"], case["batch"]
        self.use_bn, self.centering, self.ibot_weight, self.koleo_weight = bool(use_bn), centering, float(ibot_weight), float(koleo_weight)
        self.freeze_last_layer = bool(freeze_last_layer)
        assert not (self.use_bn and self.ibot_weight > 0), "MultiCropWrapper refuses BatchNorm heads under the iBOT loss"
        Dm, K, s = self.vit["hidden_size"], self.head["out_dim"], case["seed"]
        ibot = self.ibot_weight > 0
        self.masks = make_masks(case_name, masks) if ibot else None
        if params is None:
            params = dict(student_backbone=make_backbone_params(self.vit, 100 * s, ibot, QKV_SCALE[case_name], BLOCK_SCALE[case_name]),
                          teacher_backbone=make_backbone_params(self.vit, 100 * s + 50, ibot, QKV_SCALE[case_name], BLOCK_SCALE[case_name]),
                          student_head=make_head_params_scaled(Dm, self.head, 100 * s + 20, use_bn),
                          teacher_head=make_head_params_scaled(Dm, self.head, 100 * s + 70, use_bn),
                          crops=make_crops(case, 100 * s + 90),
                          center=hu((1, K), 100 * s + 98, -0.2, 0.2))
        self.sb, self.sh, self.tb, self.th = (params[k] for k in ("student_backbone", "student_head", "teacher_backbone", "teacher_head"))
        self.crops, self.center0 = params["crops"], params["center"]
        self.ibot_center0 = hu((1, K), 100 * s + 99, -0.2, 0.2)
        self._runs = {} if runs is None else runs
        self._y, self._per_sample = {}, None

    # -- one run ---------------------------------------------------------------------------------------------------------------------------
    def _step(self, dt, emulate, crops=None, koleo_weight=None, student_rows=None):
        """The step on `crops` (default: the case's).  `koleo_weight` / `student_rows` override the setting's (the two DINO-specific planted
        faults: a step whose KoLeo gradient is missing, a step whose student gathers -- and so scatters back to -- other patch rows)."""
        crops = self.crops if crops is None else crops
        kw = self.koleo_weight if koleo_weight is None else koleo_weight
        V, B = len(crops), int(crops[0].shape[0])
        fl = lambda d: {k: (v.to(dt).clone() if v.is_floating_point() else v.clone()) for k, v in d.items()}
        sb = {k: v.requires_grad_(True) for k, v in fl(self.sb).items()}
        sh = {k: (v.requires_grad_(True) if v.is_floating_point() and "running" not in k and not k.endswith("weight_g") else v) for k, v in fl(self.sh).items()}
        tb, th = fl(self.tb), fl(self.th)
        x = [c.to(dt) for c in crops]
        ibot = self.ibot_weight > 0
        sk = SK_ITERS if self.centering == "sinkhorn_knopp" else None
        rows = weights = mask_all = None
        if ibot:
            rows, weights = IR.rows_and_weights(self.masks, self.vit["num_register_tokens"])
            rows = torch.from_numpy(rows).long()
            s_rows = rows if student_rows is None else torch.as_tensor(student_rows).long()
            weights = torch.from_numpy(weights).to(dt)
            mask_all = torch.cat((torch.from_numpy(self.masks).bool(), torch.zeros((V - 2) * B, self.masks.shape[1], dtype=torch.bool)))
        Dm = self.vit["hidden_size"]
        with torch.no_grad():
            t_tok = tokens(tb, torch.cat(x[:2]), self.vit, None, emulate)
            t_in = t_tok[:, 0, :] if not ibot else torch.cat((t_tok[:, 0, :], t_tok.reshape(-1, Dm)[rows]))
            t_keep = {}
            t_log = head_forward(th, t_in, emulate, t_keep)
        t_log.requires_grad_(True)  # (no parameter behind it: only the store cost of the scalars reads this gradient)
        s_tok = tokens(sb, torch.cat(x), self.vit, mask_all, emulate)
        cls = s_tok[:, 0, :]
        s_in = cls if not ibot else torch.cat((cls, s_tok.reshape(-1, Dm)[s_rows]))
        s_in.retain_grad()
        keep = {}
        s_log = head_forward(sh, s_in, emulate, keep)
        n = V * B
        center = self.center0.to(dt)
        q = teacher_q(t_log[:2 * B], TEACHER_TEMP, center, sk)
        dino = dino_from_q(s_log[:n], q, V, STUDENT_TEMP)
        out = {"loss:dino": dino.detach()}
        loss = dino
        centers = {"center": center if sk else D.update_center(center, t_log[:2 * B].detach(), CENTER_MOMENTUM)}
        patch = None
        if ibot:
            ic = self.ibot_center0.to(dt)
            t_rows = t_log[2 * B:]
            sk_i = sk_logs(t_rows, TEACHER_TEMP, SK_ITERS, n_total=t_rows.shape[0]) if sk else None
            patch, _, csum = IR.ibot_loss(s_log[n:], t_rows, weights, 1.0 / (2 * B), STUDENT_TEMP, TEACHER_TEMP, center=ic[0], sk=sk_i)
            out["loss:ibot"] = patch.detach()
            loss = loss + self.ibot_weight * patch
            centers["ibot_center"] = ic if sk else ic * CENTER_MOMENTUM + (csum.detach() / t_rows.shape[0])[None, :] * (1 - CENTER_MOMENTUM)
        nn_idx, nn_margin, nn_dots = [], float("inf"), []
        if kw > 0:
            ka, kb = koleo(cls[:B]), koleo(cls[B:2 * B])
            out["loss:koleo"] = (ka[0] + kb[0]).detach()
            loss = loss + kw * (ka[0] + kb[0])
            nn_idx, nn_margin, nn_dots = [ka[1], kb[1]], min(ka[2], kb[2]), [ka[3], kb[3]]
        store = {}  # RMS cost, to each part, of the bf16 store it reads last (module docstring, "Scalars")
        for k, part, xs in (("loss:dino", dino, (s_log, t_log)), ("loss:ibot", patch, (s_log, t_log)), ("loss:koleo", (ka[0] + kb[0]) if kw > 0 else None, (cls,))):
            if part is not None:
                gs = torch.autograd.grad(part, xs, retain_graph=True)
                store[k] = float(sum((g * bf16_store_rms(x.detach())).square().sum() for g, x in zip(gs, xs)).sqrt())
        store["loss"] = (store["loss:dino"] ** 2 + (self.ibot_weight * store.get("loss:ibot", 0.0)) ** 2 + (kw * store.get("loss:koleo", 0.0)) ** 2) ** 0.5
        loss.backward()
        out["loss"] = loss.detach()
        grads = {"backbone." + k: v.grad for k, v in sb.items()}
        grads.update({"head." + k: v.grad for k, v in sh.items() if v.requires_grad})
        acts = {"logits": s_log[:n].detach(), "cls_tokens": cls.detach()}
        if ibot:
            acts["ibot_logits"] = s_log[n:].detach()
        stats = {"head." + k: v for k, v in sh.items() if "running" in k}
        every = list(out.values()) + list(grads.values()) + list(acts.values()) + list(centers.values()) + list(stats.values())
        assert all(t is not None and t.dtype == dt for t in every), "the restatement left its precision"
        return dict(losses=out, store={k: v / (2.0 * abs(float(out[k]))) for k, v in store.items()}, grads=grads, acts=acts, centers=centers,
                    stats=stats, du=[u.grad for u in keep["u"]], d_in=s_in.grad, gelu_in=keep["gelu_in"] + t_keep["gelu_in"], nn_idx=nn_idx,
                    nn_margin=nn_margin, nn_dots=nn_dots)

    def run(self, precision, emulate=False):
        key = (precision, bool(emulate))
        if key not in self._runs:
            self._runs[key] = self._step(torch.float64 if precision == "f64" else torch.float32, emulate)
        return self._runs[key]

    def reference(self, mode):
        """What the device is compared with: fp32 mode -> the plain run in fp64; bf16 mode -> the bf16-storage run in fp64."""
        return self.run("f64", mode == "bf16")

    # -- views -----------------------------------------------------------------------------------------------------------------------------
    def zero_names(self):
        """Tensors whose gradient is zero in exact arithmetic: the biases in front of a BatchNorm -- the head's two Linear biases and the
        backbone's final norm.bias, which shifts every class-token row, and so every column of the first Linear's output, by a constant."""
        return ["head.mlp.0.bias", "head.mlp.3.bias", "backbone.norm.bias"] if self.use_bn else []

    def grad_names(self):
        """The gradients the step leaves: every trainable tensor; without the prototype layer while it is frozen (weight_g never trains)."""
        names = list(self.run("f64")["grads"])
        return [k for k in names if not (self.freeze_last_layer and "last_layer" in k)]

    def flat(self, run, mode):
        """{name: tensor} of what is held by E <= M * Y: loss and parts, gradients (not the mathematically-zero ones), the centres an EMA
        moves, running statistics, and in fp32 mode the activations as "act:<key>"."""
        out = dict(run["losses"])
        out.update({k: run["grads"][k] for k in self.grad_names() if k not in self.zero_names()})
        if self.centering == "centering":  # (Sinkhorn-Knopp leaves the centres alone: held bit for bit by the GPU test, no yardstick)
            out.update({"centre:" + k: v for k, v in run["centers"].items()})
        out.update({"stat:" + k: v for k, v in run["stats"].items()})
        if mode == "fp32":
            out.update({"act:" + k: v for k, v in run["acts"].items()})
        return out

    def yardstick(self, mode):
        """{name: Y} over flat()'s names: Y32 (fp32 mode) or Ybf (bf16 mode)."""
        if mode not in self._y:
            a, b = (self.run("f32"), self.run("f64")) if mode == "fp32" else (self.run("f64", True), self.run("f64"))
            fa, fb = self.flat(a, "fp32"), self.flat(b, "fp32")
            y = {k: (E_rows(fa[k], o) if k.startswith("act:") else E(fa[k], o)) for k, o in fb.items()}
            for k in [k for k in y if k.startswith("loss")]:  # (module docstring, "Scalars")
                if mode == "fp32":
                    y[k] += 2.0 ** -25
                else:
                    y[k] += E(self.run("f32", True)["losses"][k], a["losses"][k]) + a["store"][k]
            self._y[mode] = y
        return self._y[mode]

    def zero_bias_bounds(self, mode):
        """{name: bound}: fp32 mode a scalar on max |g|; bf16 mode a vector, one bound per column (module docstring)."""
        if not self.use_bn:
            return {}
        if mode == "fp32":
            g = self.run("f32")["grads"]
            return {k: M32_DINO * float(g[k].abs().max()) for k in self.zero_names()}
        ref = self.reference("bf16")
        out = {k: MBF_DINO * U_BF16 * d.abs().sum(dim=0) for k, d in zip(self.zero_names()[:2], ref["du"])}
        w0 = self.sh["mlp.0.weight"].bfloat16().double()
        out["backbone.norm.bias"] = out["head.mlp.0.bias"] @ w0.abs() + MBF_DINO * U_BF16 * ref["d_in"].abs().sum(dim=0)
        return out

    def per_sample(self):
        """[{name: contribution of sample b}] in fp64, plain setting only (EMA centre, no BatchNorm, no KoLeo, no Sinkhorn-Knopp: the samples do
        not interact): the one-sample step's gradient / B (every pair term is a mean over the batch)."""
        assert not self.use_bn and self.centering == "centering" and self.koleo_weight == 0 and self.ibot_weight == 0
        if self._per_sample is None:
            self._per_sample = []
            for b in range(self.B):
                g = self._step(torch.float64, False, crops=[c[b:b + 1] for c in self.crops])["grads"]
                self._per_sample.append({k: v / self.B for k, v in g.items()})
        return self._per_sample


def dino_ref(case_name, setting, freeze_last_layer=True) -> DinoRef:
    runs = _RUNS.setdefault((case_name, setting), {})
    key = (case_name, setting, bool(freeze_last_layer))
    if key not in _REF:
        _REF[key] = DinoRef(case_name, freeze_last_layer=freeze_last_layer, runs=runs, **SETTINGS[setting])
    return _REF[key]
