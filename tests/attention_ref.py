"""Yardstick of the attention kernel tests: seeded input generators that make a padded key, a skipped online-softmax rescale or one wrong
keep decision visible, the operation restated in fp64 (`exact`), the same with the roundings a bf16-storage kernel cannot avoid
(`rounded`, only there to measure how large an error those roundings produce on a given input), and the error measures.  CPU, torch
and numpy only; nothing here calls the code under test.

Layout as in the kernels: qkv [B, N, 3 * H * dh] = [B, N, 3, H, dh], o and d_o [B, N, H * dh], lse [B, H, N].  A row is one (batch,
token, head) slice of dh values."""
import functools

import torch

from tests import dropout_ref as R
from tests.util import rel_err  # noqa: F401  (the global measure, re-exported beside row_err)

KINDS = ("gaussian", "flat", "deep_negative", "rising", "falling")
STEP = 32  # keys per step of the online-softmax forward

# dropout cases: the seed and site of tests/test_dropout_gpu.py
SEED = 0x9E3779B97F4A7C15
SITE = 9


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
def make_inputs(kind, B, N, H, dh, dtype, seed=0):
    """(qkv, d_o) on the CPU in `dtype`: the values are rounded to the storage type first, so the reference sees what the kernel sees.
    v and d_o are unit Gaussian.  With n unit Gaussian noise and u one fixed unit vector per head:
        gaussian       q, k unit Gaussian (one draw for the whole qkv tensor, as the older tests do)
        flat           q = 0.05 n, k = n: nearly flat logits, every key carries about 1 / N of a row
        deep_negative  q = c u + 0.5 n, k = -c u + 0.5 n, c^2 = 110 sqrt(dh): logits about -110 with a spread of a few units, so that
                       every row's lse stays under -89, past the range of the fp32 exponential (with c^2 = 100 sqrt(dh) the rows of the
                       longer shapes reach -85: log N and the spread of u.n eat the margin)
        rising         q = c u + 0.5 n, key j = (j / (N - 1)) c u + 0.5 n, c^2 = 80 sqrt(dh): logits climb from 0 to about +80
        falling        rising with the keys reversed"""
    assert kind in KINDS, kind
    g = torch.Generator().manual_seed(seed)
    if kind == "gaussian":
        qkv = torch.randn(B, N, 3 * H * dh, generator=g)
        d_o = torch.randn(B, N, H * dh, generator=torch.Generator().manual_seed(seed + 1))
        return qkv.to(dtype), d_o.to(dtype)
    nq, nk, v = (torch.randn(B, N, H, dh, generator=g) for _ in range(3))
    d_o = torch.randn(B, N, H * dh, generator=g)
    u = torch.randn(H, dh, generator=g)
    u = u / u.norm(dim=-1, keepdim=True)
    if kind == "flat":
        q, k = 0.05 * nq, nk
    elif kind == "deep_negative":
        c = (110.0 * dh ** 0.5) ** 0.5
        q, k = c * u + 0.5 * nq, -c * u + 0.5 * nk
    else:
        c = (80.0 * dh ** 0.5) ** 0.5
        ramp = torch.arange(N, dtype=torch.float32) / max(N - 1, 1)
        if kind == "falling":
            ramp = ramp.flip(0)
        q, k = c * u + 0.5 * nq, ramp.view(1, N, 1, 1) * (c * u) + 0.5 * nk
    return torch.stack((q, k, v), dim=2).reshape(B, N, 3 * H * dh).to(dtype), d_o.to(dtype)


def keep_multiplier(B, H, N, p, seed=SEED, site=SITE):
    """Z [B, H, N, N] in fp64: the numpy keep mask of (seed, site) times 1 / (1 - p)."""
    return torch.from_numpy(R.attn_mask(seed, site, B, H, N, p)).double() * R.scale(p)


# ---- the operation -------------------------------------------------------------------------------------------------------------------
def _bf16(t):
    return t.to(torch.bfloat16).double()


def _attention(qkv, d_o, B, N, H, dh, Z, r):
    """Forward and backward in fp64, by hand (so that `rounded` shares every line with `exact`); r rounds where a bf16 kernel must.
    Returns o [B, N, H * dh], lse [B, H, N] of the UNDROPPED row, dqkv [B, N, 3 * H * dh], and the probabilities P [B, H, N, N]."""
    q, k, v = qkv.detach().double().cpu().view(B, N, 3, H, dh).permute(2, 0, 3, 1, 4)
    dO = d_o.detach().double().cpu().view(B, N, H, dh).transpose(1, 2)
    scale = dh ** -0.5
    s = (q @ k.transpose(-1, -2)) * scale
    lse = torch.logsumexp(s, dim=-1)
    P = torch.exp(s - lse.unsqueeze(-1))
    PZ = r(P if Z is None else P * Z)
    o = r(PZ @ v)
    dP = dO @ v.transpose(-1, -2)
    if Z is not None:
        dP = dP * Z
    delta = (o * dO).sum(-1, keepdim=True)
    dS = r(P * (dP - delta))
    dv = PZ.transpose(-1, -2) @ dO
    dq = (dS @ k) * scale
    dk = (dS.transpose(-1, -2) @ q) * scale
    dqkv = r(torch.stack((dq, dk, dv), dim=0).permute(1, 3, 0, 2, 4).reshape(B, N, 3 * H * dh))
    return o.transpose(1, 2).reshape(B, N, H * dh), lse, dqkv, P


def exact(qkv, d_o, B, N, H, dh, Z=None):
    """(o, lse, dqkv) of (softmax(q k^T dh^-1/2) o Z) v and its gradient under d_o, in fp64 on the storage values.  Z is an optional
    keep mask times 1 / (1 - p), broadcastable to [B, H, N, N]; lse is that of the undropped row, as in the kernels."""
    return _attention(qkv, d_o, B, N, H, dh, Z, lambda t: t)[:3]


def rounded(qkv, d_o, B, N, H, dh, Z=None):
    """`exact` with the roundings no bf16-storage kernel avoids: P o Z to bf16 before P.V, o to bf16, delta from that o, P o Z and dS
    to bf16 before the gradient products, outputs to bf16.  lse stays fp64 (the kernels store it in fp32)."""
    return _attention(qkv, d_o, B, N, H, dh, Z, _bf16)[:3]


# ---- error measures ------------------------------------------------------------------------------------------------------------------
def row_err(a, b, dh):
    """max over rows of |a_row - b_row| / |b_row|; the last dimension holds whole rows of dh values."""
    a, b = a.detach().double().cpu().reshape(-1, dh), b.detach().double().cpu().reshape(-1, dh)
    return float(((a - b).norm(dim=-1) / (b.norm(dim=-1) + 1e-300)).max())


def parts(dqkv, B, N, H, dh):
    """dq, dk, dv [B, N, H * dh] of a dqkv tensor."""
    return dqkv.view(B, N, 3, H * dh).unbind(2)


# ---- the per-row dropout table -------------------------------------------------------------------------------------------------------
# (B, H, N, dh, p) of the flat-input cases whose rows of o and dV are held against the reference one by one
# (tests/test_dropout_gpu.py::test_attention_dropout_every_instance); tests/test_attention_ref_cpu.py proves for each entry that three
# times the unavoidable rounding noise stays under half the smallest move one inverted keep decision makes.
EVERY_INSTANCE = [(1, 2, N, dh) for N in (64, 217, 256, 288, 289, 513, 608) for dh in (48, 64)] + [(1, 2, 609, 48), (3, 3, 65, 48), (3, 3, 65, 64)]


def flat_rates(N):
    return (0.1, 0.5) if N <= 289 else (0.5,)


ROW_CASES = [(B, H, N, dh, p) for (B, H, N, dh) in EVERY_INSTANCE for p in flat_rates(N)]
ROW_MARGIN = 3.0  # the kernels round the unnormalised exponentials rather than P: other elements round, not more of them


class RowCase:
    """One entry of ROW_CASES: inputs, the fp64 reference, and per output (o, dV) the rounding noise, the per-row bar and the smallest
    single-flip move."""

    def __init__(self, B, H, N, dh, p):
        self.shape = (B, N, H, dh)
        self.qkv, self.d_o = make_inputs("flat", B, N, H, dh, torch.bfloat16, seed=31)
        Z = keep_multiplier(B, H, N, p)
        self.o, self.lse, self.dqkv, P = _attention(self.qkv, self.d_o, B, N, H, dh, Z, lambda t: t)
        o_r, _, dqkv_r = rounded(self.qkv, self.d_o, B, N, H, dh, Z)
        self.dv = parts(self.dqkv, B, N, H, dh)[2]
        self.noise = {"o": row_err(o_r, self.o, dh), "dv": row_err(parts(dqkv_r, B, N, H, dh)[2], self.dv, dh)}
        self.bar = {k: ROW_MARGIN * e for k, e in self.noise.items()}
        # one inverted keep decision changes Z[q, k] by 1 / (1 - p) either way: o_q moves by that times P[q, k] |v_k|, dV_k by that times
        # P[q, k] |dO_q|.  Per row of o the key with the smallest weight is inverted, per row of dV the query with the smallest weight.
        zs = R.scale(p)
        _, k, v = self.qkv.double().view(B, N, 3, H, dh).permute(2, 0, 3, 1, 4)
        dO = self.d_o.double().view(B, N, H, dh).transpose(1, 2)
        o_rows = self.o.view(B, N, H, dh).transpose(1, 2).norm(dim=-1)   # [B, H, N]
        dv_rows = self.dv.view(B, N, H, dh).transpose(1, 2).norm(dim=-1)
        pk, ik = P.min(dim=-1)  # per query: its lightest key
        pq, iq = P.min(dim=-2)  # per key: its lightest query
        move_o = zs * pk * torch.gather(v.norm(dim=-1), -1, ik) / o_rows
        move_dv = zs * pq * torch.gather(dO.norm(dim=-1), -1, iq) / dv_rows
        self.flip = {"o": float(move_o.min()), "dv": float(move_dv.min())}


@functools.lru_cache(maxsize=None)
def row_case(B, H, N, dh, p):
    return RowCase(B, H, N, dh, p)


# ---- the structured inputs of the plain kernels --------------------------------------------------------------------------------------
STRUCTURED_KINDS = ("deep_negative", "rising", "falling")
# (N, dh) at B = 2, H = 3, bf16: one shape per instance the dispatch of attention_mfma.hip can pick
STRUCTURED_SHAPES = [(55, 64),   # row-4 forward, bwd3
                     (129, 64),  # row-10, bwd4<64, 160>
                     (217, 48),  # row-14, bwd4<48, 224>
                     (200, 48),  # bwd4 with a key tile wholly past N
                     (288, 48),  # row-18, bwd2 with 8 waves
                     (300, 48),  # row-34, bwd2 with 16 waves
                     (513, 48),  # bwd5
                     (517, 64),  # bwd2 with 16 waves at head dim 64
                     (608, 48)]  # the limit: past the full-row forwards, the online-softmax forward by default
STRUCTURED_FP32 = (2, 65, 3, 64)
STRUCTURED_MARGIN = 4.0  # accumulation order and the fast exp on top of the roundings `rounded` models


class StructuredCase:
    """Inputs of one kind and shape, the fp64 reference, rel_err(rounded, exact) of o, dq, dk, dv, and where the rows' weight lies."""

    def __init__(self, kind, B, N, H, dh, dtype):
        self.qkv, self.d_o = make_inputs(kind, B, N, H, dh, dtype, seed=41)
        self.o, self.lse, self.dqkv, P = _attention(self.qkv, self.d_o, B, N, H, dh, None, lambda t: t)
        # per row: its heaviest key, and the weight held by the first and by the last of the kernels' 32-key steps (which start at key 0)
        self.peak = P.argmax(dim=-1)
        self.first_step = P[..., :STEP].sum(-1)
        self.last_step = P[..., (N - 1) // STEP * STEP:].sum(-1)
        o_r, _, dqkv_r = rounded(self.qkv, self.d_o, B, N, H, dh)
        self.noise = {"o": rel_err(o_r, self.o)}
        for name, a, b in zip(("dq", "dk", "dv"), parts(dqkv_r, B, N, H, dh), parts(self.dqkv, B, N, H, dh)):
            self.noise[name] = rel_err(a, b)


@functools.lru_cache(maxsize=None)
def structured_case(kind, B, N, H, dh, dtype):
    return StructuredCase(kind, B, N, H, dh, dtype)
