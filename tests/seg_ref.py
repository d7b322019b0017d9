"""Float64 restatement of the segmentation path (csrc/segmentation.hip, headct_foundation_amd/segmentation.py) and the error bounds
its kernels are held to.  Nothing here is taken from a kernel's output.

Layout.  Logits are [B, T, K * P^3] in token layout: column c * P^3 + v is class c at voxel v = (pz * P + py) * P + px of the patch,
patch l = (lz * G + ly) * G + lx of sample b is token first + l and covers z = lz * P + pz (likewise y, x).  Labels are uint8
[B, S, S, S], S = G * P, values 0 .. K-1, 255 = ignore.

Loss.  loss = w_ce CE + w_dice Dice; CE = sum_valid w_y nll / sum_valid w_y (0 with no valid voxel); Dice is MONAI's
DiceLoss(softmax=True, include_background=True, batch=False) over the valid voxels: dice_bc = (2 I + eps) / (Pc + Y + eps),
eps = 1e-5, Dice = mean_bc (1 - dice_bc).  A sample with no valid voxel has I = Pc = Y = 0, so dice_bc = eps / eps = 1 and it adds
nothing; a batch with no valid voxel at all has loss 0 and a zero gradient.

Bounds.  u = 2^-24 is the unit roundoff of fp32.  The kernel forms, per valid voxel and in fp32,
    d_k = x_k - m            one rounding: absolute error u |d_k|
    e_k = expf(d_k)          the library's expf is good to 1 ulp = 2 u relative; the error of d_k adds |d_k| u relative, and since
                             |d| exp(-|d|) <= 1 / e the absolute error of e_k is at most (2 e_k + 0.37) u
    s   = sum_k e_k          K - 1 additions; s >= 1 (the maximum's term is exactly 1), so rel(s) <= (2 + 1.37 (K - 1)) u
    p_k = e_k * (1 / s)      one division (2 u allowed), one product (u)
so |p_k - p_k*| <= u (A_P + C_P p_k) with A_P = 0.5 and C_P = 2 K + 8 (2 + 2 + 1 + 1.37 (K - 1) + 2 rounded up, slack included).
The cross-entropy term is t = w_y (logf(s) - (x_y - m)): rel(s) becomes an absolute error of the logarithm, logf adds 2 u |log s|
with log s <= log K, the difference x_y - m adds u |d_y| <= u nll, the subtraction u nll, the weight u |t|:
|t - t*| <= u (w_y A_CE + 3 |t|) with A_CE = 2 K + 2.
A sum of N such terms taken by one thread over `run` voxels, a 6-step lane butterfly, 3 additions over the waves and a double
accumulation of the block partials passes each term through at most depth = run + 9 fp32 additions:
    |sum - sum*| <= u (sum of the terms' own error constants + depth * sum |t|)
which is the "constant times 2^-24 times the sum of magnitudes entering the last reduction" form of tests/optim_kernel_ref.py and
tests/gemm_ref.py.  Everything after the partials is double and rounded to fp32 once (u |value|).  The quotients CE = N / W and
dice = num / den take first-order propagation with the denominators' bounds.  A bf16 output adds half a bf16 ulp, at most
2^-8 |value|; fp32 denormals may be flushed, which the floor 2^-126 covers."""
from __future__ import annotations

import numpy as np
import torch

U = 2.0 ** -24
EPS = 1e-5
IGNORE = 255
FLOOR = 2.0 ** -126
A_P = 0.5


def c_p(K: int) -> float:
    return 2.0 * K + 8.0


def a_ce(K: int) -> float:
    return 2.0 * K + 2.0


def work_split(S: int, vec: int):
    """(items, trips, blocks per sample) of the kernels' work split, restated: a sample has S^3 / vec items, a block takes `trips`
    rounds of 256 consecutive items, trips the least for which a sample has at most 64 blocks.  One thread adds trips * vec voxels."""
    items = S ** 3 // vec
    rounds = -(-items // 256)
    trips = -(-rounds // 64)
    return items, trips, -(-rounds // trips)


# name: P, G, first, B, K, pad columns of the logits' rows (pad % 4 != 0 takes the kernels off their 4-wide path)
LOSS_CASES = {
    "odd_K_first2": dict(P=4, G=2, first=2, B=3, K=3, pad=8),          # odd K, class token + one register
    "P12_vector_tail": dict(P=12, G=2, first=1, B=2, K=2, pad=4),      # P^3 = 1728, no power of two
    "two_partials": dict(P=4, G=3, first=1, B=5, K=2, pad=8),          # S^3 / 4 = 432 items: a second block per sample
    "no_leading_rows": dict(P=4, G=2, first=0, B=2, K=2, pad=0),       # first = 0, T = L
    "second_finalize_trip": dict(P=4, G=1, first=0, B=90, K=3, pad=4), # B * K = 270 > 256 finalize threads
    "one_voxel_access": dict(P=4, G=2, first=1, B=2, K=2, pad=3),      # odd row stride: one voxel per access, two blocks
    "K_below_bound": dict(P=4, G=1, first=1, B=2, K=5, pad=4),         # K = 5 runs in the kernels compiled for 6 classes
    "K16": dict(P=4, G=1, first=0, B=2, K=16, pad=0),                  # the widest class count
}


# ---- layout ------------------------------------------------------------------------------------------------------------------
def unpatchify(tok: torch.Tensor, first: int, G: int, P: int, K: int) -> torch.Tensor:
    """[B, T, K * P^3] token layout -> [B, K, S, S, S]."""
    B = tok.shape[0]
    L = G ** 3
    x = tok[:, first:first + L, :K * P ** 3].reshape(B, G, G, G, K, P, P, P)
    return x.permute(0, 4, 1, 5, 2, 6, 3, 7).reshape(B, K, G * P, G * P, G * P)


def patchify(vol: torch.Tensor, first: int, T: int, G: int, P: int) -> torch.Tensor:
    """[B, K, S, S, S] -> [B, T, K * P^3] with zeros in the rows outside first .. first + G^3."""
    B, K = vol.shape[:2]
    x = vol.reshape(B, K, G, P, G, P, G, P).permute(0, 2, 4, 6, 1, 3, 5, 7).reshape(B, G ** 3, K * P ** 3)
    out = torch.zeros(B, T, K * P ** 3, dtype=vol.dtype)
    out[:, first:first + G ** 3] = x
    return out


def column_of(c: int, pz: int, py: int, px: int, P: int) -> int:
    return c * P ** 3 + (pz * P + py) * P + px


def row_of(b: int, z: int, y: int, x: int, T: int, first: int, G: int, P: int) -> int:
    return b * T + first + ((z // P) * G + (y // P)) * G + (x // P)


# ---- loss ---------------------------------------------------------------------------------------------------------------------
def _prep(x: torch.Tensor, y: torch.Tensor, class_weight):
    B, K = x.shape[:2]
    x = x.to(torch.float64)
    yl = y.to(torch.int64)
    valid = yl < K
    onehot = torch.zeros_like(x)
    onehot.scatter_(1, torch.where(valid, yl, torch.zeros_like(yl)).unsqueeze(1), 1.0)
    onehot = onehot * valid.unsqueeze(1)
    w = torch.ones(K, dtype=torch.float64) if class_weight is None else torch.as_tensor(class_weight, dtype=torch.float64)
    wy = (onehot * w.view(1, K, 1, 1, 1)).sum(1)  # 0 at ignored voxels
    return x, valid, onehot, w, wy


def loss_parts(x: torch.Tensor, y: torch.Tensor, w_ce: float = 1.0, w_dice: float = 1.0, class_weight=None) -> dict:
    """x [B, K, S, S, S] (any float dtype, widened), y uint8 [B, S, S, S] -> the loss, its parts, the closed-form gradient
    with respect to x, and the sums the bounds need."""
    B, K = x.shape[:2]
    x, valid, onehot, w, wy = _prep(x, y, class_weight)
    p = torch.softmax(x, dim=1)
    logp = torch.log_softmax(x, dim=1)
    vm = valid.unsqueeze(1).to(torch.float64)
    nll = -(logp * onehot).sum(1)                       # 0 at ignored voxels
    N, W = (wy * nll).sum(), wy.sum()
    ce = N / W if float(W) > 0 else torch.zeros((), dtype=torch.float64)
    I = (p * onehot).flatten(2).sum(2)
    Pc = (p * vm).flatten(2).sum(2)
    Y = onehot.flatten(2).sum(2)
    num, den = 2 * I + EPS, Pc + Y + EPS
    dice_bc = num / den
    dice = (1 - dice_bc).mean()
    loss = w_ce * ce + w_dice * dice
    # closed form: dDice/dp_c = alpha_bc [y = c] + beta_bc; through the softmax dx_k = p_k (g_k - sum_c g_c p_c)
    alpha = w_dice * (-2.0 / (B * K * den))
    beta = w_dice * (num / (B * K * den * den))
    g = (alpha.view(B, K, 1, 1, 1) * onehot + beta.view(B, K, 1, 1, 1))
    dot = (g * p).sum(1, keepdim=True)
    ces = w_ce / W if float(W) > 0 else torch.zeros((), dtype=torch.float64)
    grad = (p * (g - dot) + (wy * ces).unsqueeze(1) * (p - onehot)) * vm
    return dict(loss=loss, ce=ce, dice=dice, dice_bc=dice_bc, grad=grad, p=p, onehot=onehot, valid=valid, wy=wy, nll=nll, N=N, W=W, I=I, Pc=Pc,
                Y=Y, num=num, den=den, alpha=alpha, beta=beta, g=g, dot=dot, ces=ces, nvalid=valid.flatten(1).sum(1).to(torch.float64))


def loss_composed(x: torch.Tensor, y: torch.Tensor, w_ce: float = 1.0, w_dice: float = 1.0, class_weight=None) -> torch.Tensor:
    """The plain torch composition (log_softmax, one-hot, MONAI's formula written out), differentiable in x; x's dtype is kept."""
    B, K = x.shape[:2]
    yl = y.to(torch.int64)
    valid = yl < K
    oh = torch.nn.functional.one_hot(torch.where(valid, yl, torch.zeros_like(yl)), K).movedim(-1, 1).to(x.dtype) * valid.unsqueeze(1)
    w = torch.ones(K, dtype=x.dtype) if class_weight is None else torch.as_tensor(class_weight, dtype=x.dtype)
    logp = torch.log_softmax(x, dim=1)
    wy = (oh * w.view(1, K, 1, 1, 1)).sum(1)
    W = wy.sum()
    ce = (-(logp * oh).sum(1) * wy).sum() / W if float(W) > 0 else x.sum() * 0
    p = torch.softmax(x, dim=1) * valid.unsqueeze(1)
    I, Pc, Y = (p * oh).flatten(2).sum(2), p.flatten(2).sum(2), oh.flatten(2).sum(2)
    dice = (1 - (2 * I + EPS) / (Pc + Y + EPS)).mean()
    return w_ce * ce + w_dice * dice


def constant_prediction(y: torch.Tensor, K: int, w_ce: float = 1.0, w_dice: float = 1.0, class_weight=None) -> dict:
    """Loss and foreground Dice of the best constant prediction: softmax at the class prior of the valid voxels at every voxel
    (its arg-max is the most frequent class everywhere)."""
    yl = y.to(torch.int64)
    valid = yl < K
    cnt = torch.bincount(yl[valid], minlength=K).to(torch.float64)
    prior = cnt / cnt.sum()
    logit = torch.log(prior.clamp_min(1e-300))
    x = logit.view(1, K, 1, 1, 1).expand(y.shape[0], K, *y.shape[1:])
    r = loss_parts(x, y, w_ce, w_dice, class_weight)
    pred = torch.full_like(yl, int(prior.argmax())).to(torch.uint8)
    m = metrics(counts(pred, y, K))
    return dict(loss=float(r["loss"]), fg_dice=float(np.nan_to_num(m["dice_global"][1:]).mean()))


# ---- bounds -------------------------------------------------------------------------------------------------------------------
def loss_bounds(r: dict, K: int, w_ce: float, w_dice: float, run: int, out_bf16: bool = False) -> dict:
    """Bounds on loss, ce, dice, dice_bc [B, K] and grad (per element, [B, K, S, S, S]) of a kernel evaluation against `r`
    (loss_parts of the same stored logits).  run: the voxels one thread adds before the block tree (trips * V)."""
    depth = run + 9.0
    cp, ace = c_p(K), a_ce(K)
    p, oh, wy, nll = r["p"], r["onehot"], r["wy"], r["nll"]
    vm = r["valid"].unsqueeze(1).to(torch.float64)
    nv = r["nvalid"].view(-1, 1)
    eI = U * (A_P * r["Y"] + (cp + depth) * r["I"])
    ePc = U * (A_P * nv + (cp + depth) * r["Pc"])
    eN = U * (ace * r["W"] + (3 + depth) * r["N"])
    eW = U * depth * r["W"]
    W = float(r["W"])
    if W > 0:
        e_ce = eN / W + r["N"] * eW / W ** 2 + U * abs(r["ce"])
        rel_ces = eW / W + U
    else:
        e_ce, rel_ces = torch.zeros((), dtype=torch.float64), torch.zeros((), dtype=torch.float64)
    num, den = r["num"], r["den"]
    e_d = 2 * eI / den + num * ePc / den ** 2 + U * r["dice_bc"]
    e_dice = e_d.mean() + U * abs(r["dice"])
    e_loss = w_ce * e_ce + w_dice * e_dice + U * abs(r["loss"])
    # gradient: coefficients alpha, beta from the sums (double, then one rounding to fp32)
    e_al = r["alpha"].abs() * (ePc / den + U)
    e_be = r["beta"].abs() * (2 * eI / num + 2 * ePc / den + U)
    B = p.shape[0]
    e_p = U * (A_P + cp * p)
    g, dot = r["g"], r["dot"]
    e_g = e_al.view(B, K, 1, 1, 1) * oh + e_be.view(B, K, 1, 1, 1) + U * g.abs()
    gp = (g * p).abs()
    e_dot = (e_g * p + g.abs() * e_p + U * gp).sum(1, keepdim=True) + (K - 1) * U * gp.sum(1, keepdim=True)
    diff = (g - dot).abs()
    t1 = p * (g - dot)
    e_t1 = e_p * diff + p * (e_g + e_dot + U * diff) + U * t1.abs()
    cs = (wy * r["ces"]).unsqueeze(1)
    e_cs = cs * (rel_ces + U)
    pd = (p - oh).abs()
    t2 = cs * (p - oh)
    e_t2 = e_cs * pd + cs * (e_p + U * pd) + U * t2.abs()
    grad = r["grad"]
    e_grad = (e_t1 + e_t2 + 2 * U * (t1.abs() + t2.abs())) * vm
    if out_bf16:
        e_grad = e_grad + 2.0 ** -8 * grad.abs()
    e_grad = e_grad + FLOOR
    return dict(loss=e_loss + FLOOR, ce=e_ce + FLOOR, dice=e_dice + FLOOR, dice_bc=e_d + FLOOR, grad=e_grad)


# ---- prediction and metrics ---------------------------------------------------------------------------------------------------------
def predict(x: torch.Tensor) -> torch.Tensor:
    """arg-max over the class axis of [B, K, S, S, S], ties to the lowest class."""
    xn = x.to(torch.float64).numpy()
    return torch.from_numpy(np.argmax(xn, axis=1).astype(np.uint8))  # numpy's argmax returns the first maximum


def counts(pred: torch.Tensor, y: torch.Tensor, K: int) -> np.ndarray:
    """int64 [B, K, 3] = TP, FP, FN per sample and class over the valid voxels."""
    pr, yl = pred.to(torch.int64).numpy(), y.to(torch.int64).numpy()
    B = pr.shape[0]
    out = np.zeros((B, K, 3), dtype=np.int64)
    for b in range(B):
        v = yl[b] < K
        for c in range(K):
            a, t = (pr[b] == c) & v, (yl[b] == c) & v
            out[b, c] = ((a & t).sum(), (a & ~t).sum(), (~a & t).sum())
    return out


def metrics(cnt: np.ndarray) -> dict:
    """Dataset-level ("global") Dice and IoU per class from summed counts, and the mean of the per-scan Dice over the scans where the
    class is present (TP + FN > 0).  An empty denominator gives nan."""
    cnt = np.asarray(cnt, dtype=np.float64)
    tot = cnt.sum(0)
    tp, fp, fn = tot[:, 0], tot[:, 1], tot[:, 2]
    with np.errstate(invalid="ignore", divide="ignore"):
        dice_g = 2 * tp / (2 * tp + fp + fn)
        iou_g = tp / (tp + fp + fn)
        per = 2 * cnt[:, :, 0] / (2 * cnt[:, :, 0] + cnt[:, :, 1] + cnt[:, :, 2])
    present = (cnt[:, :, 0] + cnt[:, :, 2]) > 0
    dice_s = np.array([per[present[:, c], c].mean() if present[:, c].any() else np.nan for c in range(cnt.shape[1])])
    return dict(dice_global=dice_g, iou_global=iou_g, dice_scan=dice_s)


# ---- label flips ---------------------------------------------------------------------------------------------------------------
def flip_labels(pool: torch.Tensor, slots, flip) -> torch.Tensor:
    """out[b] = flips(pool[slots[b]]): bit a of flip[b] reverses spatial axis a; slot -1 gives an all-ignore volume."""
    out = []
    for s, f in zip([int(v) for v in slots], [int(v) for v in flip]):
        v = pool[s] if s >= 0 else torch.full_like(pool[0], IGNORE)
        dims = [a for a in range(3) if f >> a & 1]
        out.append(torch.flip(v, dims) if dims else v.clone())
    return torch.stack(out)


# ---- the label item: nearest neighbour through the image's geometry ------------------------------------------------------------------
def nearest_axis(d: int, m: int, step: float) -> np.ndarray:
    """Resampled voxel j of an axis (m of them, reading input coordinate j * step) shows mask voxel clamp(floor(j step + 0.5), 0, d - 1)."""
    return np.clip(np.floor(np.arange(m, dtype=np.float64) * step + 0.5), 0, d - 1).astype(np.int64)


def cell_centres(start: int, size: int, R: int) -> np.ndarray:
    """The resampled cell under the centre of each of the R bins the resize cuts a box axis [start, start + size) into, in integers:
    start + min(size - 1, ((2 o + 1) size) // (2 R))."""
    o = np.arange(R, dtype=np.int64)
    return start + np.minimum(size - 1, ((2 * o + 1) * size) // (2 * R))


def label_item(mask_ras: np.ndarray, m, steps, box_start, box_size, roi) -> np.ndarray:
    """uint8 [*roi] of a mask in RAS order [d0, d1, d2] through the image's geometry (resampled shape m, spacing steps, foreground
    box, roi); a value that is no integer in [0, 254] raises ValueError."""
    idx = [nearest_axis(mask_ras.shape[a], m[a], steps[a])[cell_centres(int(box_start[a]), int(box_size[a]), roi[a])] for a in range(3)]
    v = np.asarray(mask_ras, dtype=np.float64)[np.ix_(*idx)]
    if not bool(((v >= 0) & (v <= 254) & (v == np.floor(v))).all()):
        raise ValueError("a mask value is no integer in [0, 254]")
    return v.astype(np.uint8)


# ---- inputs shared by the CPU and GPU tests -------------------------------------------------------------------------------------
def make_case(B: int, G: int, P: int, K: int, first: int, seed: int = 0, pad: int = 0, dtype=torch.float32):
    """Token-layout logits [B, T, K * P^3 + pad] (T = first + G^3; stored in `dtype`, NaN in the leading rows and the pad columns) and
    labels with: a logit gap of +-60 at some voxels (a saturated softmax), class K - 1 absent from sample 0, sample B - 1 all
    ignored, ignore voxels scattered elsewhere."""
    gen = torch.Generator().manual_seed(seed)
    S, L, T = G * P, G ** 3, first + G ** 3
    vol = torch.randn(B, K, S, S, S, generator=gen, dtype=torch.float64) * 2
    y = torch.randint(0, K, (B, S, S, S), generator=gen, dtype=torch.int64)
    y[0][y[0] == K - 1] = 0
    y[torch.rand(B, S, S, S, generator=gen) < 0.1] = IGNORE
    y[B - 1] = IGNORE
    vol[:, 0, 0, 0, :] += 60.0   # saturated towards class 0 along one edge
    vol[:, 1, 1, :, 0] += 60.0   # and towards class 1 along another
    tok = torch.full((B, T, K * P ** 3 + pad), float("nan"), dtype=torch.float64)
    tok[:, :, :K * P ** 3] = patchify(vol, first, T, G, P)
    if first:
        tok[:, :first] = float("nan")
    return tok.to(dtype), y.to(torch.uint8)
