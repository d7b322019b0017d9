"""Yardstick of the MAE data-path kernels (csrc/elementwise.hip: masking, patch gather, encoder / decoder / ViT input assembly and
their backwards, masked MSE, unpatchify): plain torch restatements of the definitions in include/headct_hip.h.  The arithmetic runs
in the dtype of the tensors handed in (the tests hand in float64); the backwards of the three assemblies are autograd through the
forwards.  The second half builds the inputs of tests/test_assembly_kernels_gpu.py, so that tests/test_assembly_ref_cpu.py can
assert their stated properties without a GPU.  Nothing here calls the code under test."""
import torch

U32 = 2.0 ** -24  # unit roundoff of fp32
U16 = 2.0 ** -9   # relative storage rounding of bf16 (8 significand bits, round to nearest)


# ---- masking -------------------------------------------------------------------------------------------------------------------
def mask_rank(noise, K):
    """(ids_restore, ids_shuffle, mask) of hct_mask_rank: stable ranking, ties -> lower index first; mask 0 keep, 1 masked."""
    ids_shuffle = torch.argsort(noise, dim=1, stable=True)
    ids_restore = torch.argsort(ids_shuffle, dim=1, stable=True)
    return ids_restore, ids_shuffle, (ids_restore >= K).to(torch.float32)


# ---- patches -------------------------------------------------------------------------------------------------------------------
def patch_rows(x, P):
    """[B, C, S, S, S] -> [B, L, C P^3], every patch in grid order, columns in Conv3d weight order (c, ph, pw, pd)."""
    B, C, S = x.shape[:3]
    g = S // P
    return x.reshape(B, C, g, P, g, P, g, P).permute(0, 2, 4, 6, 1, 3, 5, 7).reshape(B, g ** 3, C * P ** 3)


def patch_gather(x, ids_shuffle, P, K):
    """rows [B K, C P^3] of hct_patch_gather: patch ids_shuffle[b, j] for j < K (ids_shuffle None: every patch, K = L)."""
    rows = patch_rows(x, P)
    if ids_shuffle is not None:
        rows = torch.gather(rows, 1, ids_shuffle[:, :K].long().unsqueeze(-1).expand(-1, -1, rows.shape[-1]))
    return rows.reshape(-1, rows.shape[-1])


def patchify(x, P):
    """[B, C, S, S, S] -> [B, L, P^3 C] in the loss's order (ph, pw, pd, c), c fastest."""
    B, C, S = x.shape[:3]
    g = S // P
    return x.reshape(B, C, g, P, g, P, g, P).permute(0, 2, 4, 6, 3, 5, 7, 1).reshape(B, g ** 3, P ** 3 * C)


def unpatchify(rows, C, S, P):
    """[B, L, P^3 C] -> [B, C, S, S, S]: the inverse of `patchify` (hct_unpatchify without the class rows)."""
    B = rows.shape[0]
    g = S // P
    return rows.reshape(B, g, g, g, P, P, P, C).permute(0, 7, 1, 4, 2, 5, 3, 6).reshape(B, C, S, S, S)


# ---- assembly forwards (differentiable torch) ------------------------------------------------------------------------------------
def encoder_assemble(tok, cls, pos, ids_shuffle, B, K):
    """h0 [B, K+1, D]: h0[b, 0] = cls; h0[b, 1+j] = tok[b K + j] + pos[ids_shuffle[b, j]] (pos None: no position term)."""
    D = tok.shape[-1]
    body = tok.reshape(B, K, D)
    if pos is not None:
        body = body + pos[ids_shuffle[:, :K].long()]
    return torch.cat((cls.reshape(1, 1, D).expand(B, 1, D), body), dim=1)


def decoder_assemble(e, mask_token, dec_cls, dec_pos, ids_restore, K):
    """y [B, L+1, D]: y[b, 0] = e[b, 0] + dec_cls; y[b, 1+l] = (rank < K ? e[b, 1+rank] : mask_token) + dec_pos[l], rank = ids_restore[b, l]."""
    B, L = ids_restore.shape
    D = e.shape[-1]
    pool = torch.cat((e[:, 1:], mask_token.reshape(1, 1, D).expand(B, L - K, D)), dim=1)  # rank >= K: any of the L - K copies
    body = torch.gather(pool, 1, ids_restore.long().unsqueeze(-1).expand(B, L, D)) + dec_pos
    return torch.cat((e[:, :1] + dec_cls.reshape(1, 1, D), body), dim=1)


def vit_assemble(tok, cls, reg, pos, B):
    """h [B, 1+R+L, D]: class token, the R register tokens (reg None: R = 0), tok[b L + l] + pos[l] (pos None: no position term)."""
    D = tok.shape[-1]
    body = tok.reshape(B, -1, D)
    if pos is not None:
        body = body + pos
    parts = [cls.reshape(1, 1, D).expand(B, 1, D)]
    if reg is not None:
        parts.append(reg.reshape(1, -1, D).expand(B, -1, D))
    return torch.cat(parts + [body], dim=1)


def vjp(fwd, inputs, dout):
    """Gradients of sum(fwd(*leaves) * dout) with respect to every entry of `inputs` that is not None (None stays None)."""
    leaves = [None if t is None else t.detach().clone().requires_grad_(True) for t in inputs]
    out = fwd(*leaves)
    (out * dout).sum().backward()
    return [None if t is None else t.grad for t in leaves]


# ---- loss ------------------------------------------------------------------------------------------------------------------------
def loss_target(x, P, norm_pix):
    t = patchify(x, P)
    if norm_pix:
        t = (t - t.mean(dim=-1, keepdim=True)) / (t.var(dim=-1, keepdim=True) + 1.0e-6) ** 0.5  # unbiased variance
    return t


def masked_mse(pred, x, mask, P, norm_pix, scale=1.0):
    """hct_masked_mse: pred [B, L+1, pd] (row 0 of a volume is the class row and is never read), x [B, C, S, S, S], mask [B, L].
    Returns (loss, row_loss [B, L], dpred [B, L+1, pd]) in pred's dtype; dpred = scale * d loss / d pred, written by hand:
    scale * 2 * mask * (pred - target) / (pd * sum(mask)), zero on the class rows."""
    mask = mask.to(pred.dtype)
    diff = pred[:, 1:] - loss_target(x.to(pred.dtype), P, norm_pix)
    pd = diff.shape[-1]
    row_loss = (diff ** 2).mean(dim=-1) * mask
    loss = row_loss.sum() / mask.sum()
    dbody = scale * 2.0 * mask.unsqueeze(-1) * diff / (pd * mask.sum())
    return loss, row_loss, torch.cat((torch.zeros_like(pred[:, :1]), dbody), dim=1)


def rel(a, b):
    """Relative L2 error of a against b (both widened to float64)."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def sum_bound(n_terms, abs_sum):
    """Element-wise bound of recursive fp32 summation in ANY order against the exact sum: (n - 1) 2^-24 sum|terms|."""
    return (n_terms.double() - 1).clamp(min=0) * U32 * abs_sum.double()


# =================================================================================================================================
# Inputs of tests/test_assembly_kernels_gpu.py.  Everything is made on the CPU from seeded generators.
# =================================================================================================================================
S_ASM, P_ASM, L_ASM = 32, 8, 64          # the assembly geometry: a 32^3 volume in 8^3 patches
KS = (16, 13)                            # 48 masked rows = whole trips of 8; 51 = six trips and a ragged tail of 3
DS = (48, 260, 1028)                     # D/4 = 12: 64 threads; 65: 128 threads; 257: 256 threads and a second trip
K_ASM_BLOCKS = 256                       # kAsmBlocks of csrc/elementwise.hip: one reduce block per volume up to here
ENC_CASES = [(D, B) for D in DS for B in (1, 9, 17)] + [(48, 33)]
DEC_CASES = [(48, B) for B in (1, 9, 33, 257, 261)] + [(D, B) for D in DS[1:] for B in (1, 9, 33)]
VIT_L = 27
VIT_CASES = [(D, B) for D in (48, 1028) for B in (1, 17, 33)]
MSE_CASES = [(4, 1, 8, 3), (8, 1, 16, 3), (12, 1, 24, 3), (4, 3, 8, 3), (12, 3, 24, 3), (8, 1, 32, 33)]  # (P, C, S, B)
MSE_K = {8: 2, 64: 16}                   # kept patches per volume at L = 8 / L = 64 (mask ratio 0.75)


def gen(*key):
    return torch.Generator().manual_seed(sum(int(k) * 1000003 ** i for i, k in enumerate(key)) % (2 ** 31))


def values(shape, kind, g):
    """"int": integers in [-4, 4] (exact in bf16, sums of up to 2^21 of them exact in fp32); "normal": standard normal."""
    if kind == "int":
        return torch.randint(-4, 5, shape, generator=g).to(torch.float32)
    return torch.randn(shape, generator=g)


def permutations(B, L, K, seed):
    """A different random permutation per volume, as hct_mask_rank ranks seeded uniform noise."""
    noise = torch.rand(B, L, generator=gen(B, L, K, seed))
    return (noise,) + mask_rank(noise, K)


def rank_noise(B, L, seed):
    """Noise rows with ties: a tie of the two smallest at the row's start, of the two largest at its end, and a constant row."""
    noise = torch.rand(B, L, generator=gen(B, L, seed)) * 0.5 + 0.25
    noise[0, 0] = noise[0, 1] = 0.0
    noise[0, L - 1] = noise[0, L - 2] = 1.0
    noise[1, 0] = noise[1, L - 1] = 0.0    # lowest value at both ends: index 0 first
    noise[1, 1] = noise[1, L - 2] = 1.0
    noise[B - 1] = 0.5                     # all ties: identity
    return noise


def mse_inputs(P, C, S, B, x_dtype, pred_dtype):
    """Volume, prediction (class rows NaN) and mask of one hct_masked_mse case, rounded to the storage types.  Patch 0 of volume 0
    is all zero (variance 0) and patch 1 has a single non-zero voxel; both are masked (largest noise)."""
    L = (S // P) ** 3
    K, pd = MSE_K[L], P ** 3 * C
    g = gen(P, C, S, B)
    xp = torch.rand(B, L, pd, generator=g)
    xp[0, 0] = 0.0
    xp[0, 1] = 0.0
    xp[0, 1, pd // 3] = 0.625
    x = unpatchify(xp, C, S, P).contiguous().to(x_dtype)
    pred = torch.randn(B, L + 1, pd, generator=g)
    pred[:, 0] = float("nan")
    noise = torch.rand(B, L, generator=g)
    noise[0, 0], noise[0, 1] = 2.0, 3.0
    ids_restore, ids_shuffle, mask = mask_rank(noise, K)
    return x, pred.to(pred_dtype), mask, K


def degenerate_rows(B, L):
    """[B, L] bool: the two patches whose norm_pix target divides by a (nearly) vanishing variance."""
    d = torch.zeros(B, L, dtype=torch.bool)
    d[0, 0] = d[0, 1] = True
    return d


def encoder_inputs(D, B, K, kind):
    _, ids_restore, ids_shuffle, _ = permutations(B, L_ASM, K, 5)
    g = gen(D, B, K, kind == "int", 1)
    return dict(ids_restore=ids_restore, ids_shuffle=ids_shuffle, cls=values((D,), kind, g), pos=values((L_ASM, D), kind, g),
                tok=values((B * K, D), kind, g), dh0=values((B, K + 1, D), kind, g))


def decoder_inputs(D, B, K, kind):
    _, ids_restore, ids_shuffle, _ = permutations(B, L_ASM, K, 5)
    g = gen(D, B, K, kind == "int", 2)
    return dict(ids_restore=ids_restore, ids_shuffle=ids_shuffle, mask_token=values((D,), kind, g), dec_cls=values((D,), kind, g),
                dec_pos=values((L_ASM, D), kind, g), e=values((B, K + 1, D), kind, g), dy=values((B, L_ASM + 1, D), kind, g))


def vit_inputs(D, B, R, kind):
    g = gen(D, B, R, kind == "int", 3)
    return dict(cls=values((D,), kind, g), pos=values((VIT_L, D), kind, g), reg=values((R, D), kind, g) if R else None,
                tok=values((B * VIT_L, D), kind, g), dh=values((B, 1 + R + VIT_L, D), kind, g))


def _three(fwd, zeros, dout, names):
    """(sums, term counts, sums of |terms|) of the backward of the linear map `fwd`, each a dict by gradient name; float64 unless
    `dout` is fp32 (the CPU test's fp32 evaluation)."""
    zeros = [None if z is None else z.to(dout.dtype) for z in zeros]
    return tuple(dict(zip(names, vjp(fwd, zeros, d))) for d in (dout, torch.ones_like(dout), dout.abs()))


def encoder_bwd(inp, B, K, dtype=torch.float64):
    D = inp["cls"].shape[0]
    zeros = [torch.zeros(B * K, D), torch.zeros(D), torch.zeros(L_ASM, D)]
    return _three(lambda t, c, p: encoder_assemble(t, c, p, inp["ids_shuffle"], B, K), zeros, inp["dh0"].to(dtype), ("dtok", "dcls", "dpos"))


def decoder_bwd(inp, B, K, dtype=torch.float64):
    D = inp["dec_cls"].shape[0]
    zeros = [torch.zeros(B, K + 1, D), torch.zeros(D), torch.zeros(D)]
    pos = torch.zeros(L_ASM, D, dtype=dtype)
    return _three(lambda e, m, c: decoder_assemble(e, m, c, pos, inp["ids_restore"], K), zeros, inp["dy"].to(dtype),
                  ("de", "dmask_token", "ddec_cls"))


def vit_bwd(inp, B, R, dtype=torch.float64):
    D = inp["cls"].shape[0]
    zeros = [torch.zeros(B * VIT_L, D), torch.zeros(D), torch.zeros(R, D) if R else None, torch.zeros(VIT_L, D)]
    return _three(lambda t, c, r, p: vit_assemble(t, c, r, p, B), zeros, inp["dh"].to(dtype), ("dtok", "dcls", "dreg", "dpos"))
