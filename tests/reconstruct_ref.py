"""Yardstick of the MAE reconstruction path: a float64 torch restatement of the mask schedule, the accumulation over passes and the
finish of headct_foundation_amd/reconstruct.py, on top of the oracle's forward (`pred`, `mask` from injected noise), `patchify`
and `unpatchify`.  Nothing here calls the code under test."""
import math

import torch

from oracle import mae_oracle as O


def geometry(S, P, C, norm_pix=False, mask_ratio=0.75):
    """An oracle configuration that carries only the patch geometry (for the kernel tests)."""
    return O.MAEConfig(input_size=S, patch_size=P, in_chans=C, norm_pix_loss=norm_pix, mask_ratio=mask_ratio)


# ---- schedule ------------------------------------------------------------------------------------------------------------------
def cover_passes(L, K):
    return math.ceil(L / (L - K))


def slots(B, L, seed):
    """slot[b, l]: position of patch l in volume b's permutation = argsort of torch.rand(B, L) from a CPU generator seeded `seed`."""
    return torch.argsort(torch.rand(B, L, generator=torch.Generator().manual_seed(seed)), dim=1)


def window_masks(slot, n, K):
    """[n, B, L] uint8: pass p masks the ring window {(start_p + j) mod L : j < M}, start_p = (p L) // n."""
    B, L = slot.shape
    M = L - K
    out = torch.zeros(n, B, L, dtype=torch.uint8)
    for p in range(n):
        window = {((p * L) // n + j) % L for j in range(M)}
        for b in range(B):
            for l in range(L):
                out[p, b, l] = int(int(slot[b, l]) in window)
    return out


def noise_of(slot, p, n, K):
    L = slot.shape[1]
    return ((slot - (p * L) // n - (L - K)) % L).to(torch.float32)


# ---- accumulation ---------------------------------------------------------------------------------------------------------------
class State:
    def __init__(self, cfg, B):
        S, L = cfg.input_size, cfg.num_patches
        self.recon_sum = torch.zeros(B, cfg.in_chans, S, S, S, dtype=torch.float64)
        self.err_sum = torch.zeros(B, L, dtype=torch.float64)
        self.cnt = torch.zeros(B, L, dtype=torch.int64)


def patch_terms(cfg, pred, x):
    """(v [B, L, pd] de-normalised prediction, e [B, L] per-patch loss term) in float64; mae.py:290-296."""
    pred, t = pred.double(), O.patchify(cfg, x.double())
    if cfg.norm_pix_loss:
        mu = t.mean(dim=-1, keepdim=True)
        sd = (t.var(dim=-1, keepdim=True) + 1.0e-6) ** 0.5
        target, v = (t - mu) / sd, pred * sd + mu
    else:
        target, v = t, pred
    return v, ((pred - target) ** 2).mean(dim=-1)


def accumulate(cfg, st, pred, x, mask):
    """One pass: pred [B, L, pd], x [B, C, S, S, S], mask [B, L] (non-zero = masked)."""
    v, e = patch_terms(cfg, pred, x)
    m = (mask != 0)
    st.recon_sum += O.unpatchify(cfg, v * m.unsqueeze(-1))
    st.err_sum += e * m
    st.cnt += m.to(torch.int64)
    return e


def finish(cfg, st, x):
    """(recon [B, C, S, S, S], err [B, L], cnt [B, L], err_vol [B, S, S, S]) float64."""
    B, L, pd = st.cnt.shape[0], cfg.num_patches, cfg.patch_dim
    seen = st.cnt > 0
    c = st.cnt.clamp(min=1).double()
    seen_vox = O.unpatchify(cfg, seen.unsqueeze(-1).expand(B, L, pd).double()) > 0
    recon = torch.where(seen_vox, st.recon_sum / O.unpatchify(cfg, c.unsqueeze(-1).expand(B, L, pd)), x.double())
    err = torch.where(seen, st.err_sum / c, torch.zeros_like(st.err_sum))
    one = O.MAEConfig(input_size=cfg.input_size, patch_size=cfg.patch_size, in_chans=1)
    err_vol = O.unpatchify(one, err.unsqueeze(-1).expand(B, L, one.patch_dim))[:, 0]
    return recon, err, st.cnt.clone(), err_vol


# ---- end to end -----------------------------------------------------------------------------------------------------------------
def oracle_predictor(params, emulate_bf16=False):
    """(loss, pred, mask) of the oracle's forward: in float64 throughout, or with `emulate_bf16` in fp32 with the HIP bf16 path's
    roundings (the emulation itself works in fp32)."""
    def run(cfg, x, noise):
        if emulate_bf16:
            loss, pred, mask, _ = O.forward(cfg, params, x.float(), noise, emulate_bf16=True)
        else:
            loss, pred, mask, _ = O.forward(cfg, {k: v.double() for k, v in params.items()}, x.double(), noise)
        return loss, pred, mask
    return run


def perfect_predictor(cfg, x, noise):
    """pred := target: the reconstruction must give the scan back and the error must vanish."""
    t = O.patchify(cfg, x.double())
    if cfg.norm_pix_loss:
        t = (t - t.mean(dim=-1, keepdim=True)) / (t.var(dim=-1, keepdim=True) + 1.0e-6) ** 0.5
    mask = O.random_masking_from_noise(cfg, noise)[3]
    return torch.zeros((), dtype=torch.float64), t, mask


def reconstruct(cfg, predictor, x, passes=None, seed=0, noise=None):
    """dict(recon, error [B, g, g, g], count, error_volume, loss [n], masks [n, B, L] uint8, patch_err [n, B, L]) in float64."""
    B, L, K, g = x.shape[0], cfg.num_patches, cfg.len_keep, cfg.grid
    n = cover_passes(L, K) if passes is None else passes
    if noise is not None:
        assert n == 1
        noises = [noise.float()]
    else:
        slot = slots(B, L, seed)
        noises = [noise_of(slot, p, n, K) for p in range(n)]
    st = State(cfg, B)
    losses, masks, perr = [], [], []
    for nz in noises:
        loss, pred, mask = predictor(cfg, x, nz)
        perr.append(accumulate(cfg, st, pred, x, mask))
        losses.append(float(loss))
        masks.append(mask.to(torch.uint8))
    recon, err, cnt, err_vol = finish(cfg, st, x)
    return dict(recon=recon, error=err.view(B, g, g, g), count=cnt.view(B, g, g, g), error_volume=err_vol,
                loss=torch.tensor(losses, dtype=torch.float64), masks=torch.stack(masks), patch_err=torch.stack(perr))
