"""Yardstick of the attention kernel tests: seeded input generators that make a padded key, a skipped online-softmax rescale or one wrong
keep decision visible, the operation restated in fp64 (`exact`), the same with the roundings a bf16-storage kernel cannot avoid
(`rounded`, only there to measure how large an error those roundings produce on a given input), and the error measures.  CPU, torch
and numpy only; nothing here calls the code under test.

Layout as in the kernels: qkv [B, N, 3 * H * dh] = [B, N, 3, H, dh], o and d_o [B, N, H * dh], lse [B, H, N].  A row is one (batch,
token, head) slice of dh values."""
import functools

import numpy as np
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


# ---- the per-row table of the plain kernels ------------------------------------------------------------------------------------------
def row_errs(a, b, dh):
    """|a_row - b_row| / |b_row| of every row, shaped like a with the last dimension counted in rows of dh values."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    lead = a.shape[:-1] + (a.shape[-1] // dh,)
    a, b = a.reshape(-1, dh), b.reshape(-1, dh)
    return ((a - b).norm(dim=-1) / (b.norm(dim=-1) + 1e-300)).view(lead)


def npad(N):
    return (N + 31) // 32 * 32  # the kernels pad a sequence to whole 32-key steps


def plain_instances(N, dh, mode=0):
    """(forward, backward) kernel of the plain attention at N tokens and head dim dh (48 or 64) under hct_debug_force_simple_attention(mode),
    restated from attention_fwd_mfma and attention_bwd_mfma (attention_mfma.hip)."""
    if mode == 1:
        return "simple_fwd", "simple_bwd"
    Np = npad(N)
    waves = 4 if N <= 64 else 8 if 264 * Np <= 81408 else 16  # bwd2_lds: two 128-byte images and two floats per padded row
    bwd2 = f"bwd2<{dh},{waves}>"
    if mode == 2:
        return f"online<{dh}>", bwd2
    fwd = next((f"row<{dh},{nt}>" for nt in (4, 10, 14, 18, 34) if Np // 16 <= nt), f"online<{dh}>")
    if dh == 64 and Np == 160:
        return fwd, "bwd4<64,160>"
    if dh == 48 and Np == 224:
        return fwd, "bwd4<48,224>"
    if dh == 64 and Np <= 64:
        return fwd, "bwd3<64>"
    if dh == 48 and 448 < Np <= 576:
        return fwd, "bwd5<48>"
    return fwd, bwd2


# One length per edge of every instance, for dh in (48, 64); Npad = npad(N).  The dispatch by default (mode 0):
#   forward   row<dh,4> 1..64, row<dh,10> 65..160, row<dh,14> 161..224, row<dh,18> 225..288, row<dh,34> 289..544, online 545..608
#   backward  dh 64: bwd3 1..64, bwd4<64,160> 129..160, bwd2 elsewhere;  dh 48: bwd4<48,224> 193..224, bwd5 449..576, bwd2 elsewhere
#   bwd2      4 waves 1..64, 8 waves 65..288, 16 waves 289..608 (mode 2 takes it and the online forward at every length)
PLAIN_N = (1,    # lowest of row-4, bwd3, bwd2 with 4 waves: one key, 31 padded ones
           17,   # row-4, bwd3 / bwd2-4: one key in the second tile
           33,   # row-4, bwd3 / bwd2-4: Npad 64, the tile 48..63 wholly past N
           64,   # highest of row-4, bwd3, bwd2-4: no padded key
           65,   # lowest of row-10 and of bwd2 with 8 waves: Npad 96, the tile 80..95 wholly past N
           129,  # row-10; lowest of bwd4<64,160> (bwd2-8 at dh 48): the tile 144..159 wholly past N
           160,  # highest of row-10 and of bwd4<64,160>: no padded key
           161,  # lowest of row-14: the tile 176..191 wholly past N; bwd2-8
           193,  # row-14; lowest of bwd4<48,224> (bwd2-8 at dh 64): the tile 208..223 wholly past N
           209,  # row-14, bwd4<48,224>: one key in the last tile
           224,  # highest of row-14 and of bwd4<48,224>: no padded key
           225,  # lowest of row-18: the tile 240..255 wholly past N; bwd2-8
           288,  # highest of row-18 and of bwd2 with 8 waves: no padded key
           289,  # lowest of row-34 and of bwd2 with 16 waves: the tile 304..319 wholly past N
           449,  # row-34; lowest of bwd5 (bwd2-16 at dh 64): the tile 464..479 wholly past N
           513,  # row-34, bwd5: the tile 528..543 wholly past N (the ViT-L decoder's length)
           544,  # highest of row-34: no padded key; bwd5
           545,  # lowest length the online-softmax forward takes by default: the tile 560..575 wholly past N; bwd5
           576,  # highest of bwd5: no padded key; online forward
           577,  # first length past bwd5, bwd2-16 again: the tile 592..607 wholly past N
           608)  # highest of the online forward and of bwd2-16, the limit of attention_mfma_supported: no padded key
PLAIN_ROW_CASES = [(N, dh) for dh in (48, 64) for N in PLAIN_N]
PLAIN_DEEP_CASES = [(N, dh) for N, dh in PLAIN_ROW_CASES if N % 32]  # the lengths with padded keys
PLAIN_FP32_CASES = [(2, 65, 3, 64), (2, 33, 3, 16), (1, 1, 2, 48)]   # fp32 storage: the fp32-math kernels
PLAIN_B, PLAIN_H, PLAIN_SEED = 2, 3, 51
PLAIN_FP32_BAR = {"o": 2e-5, "dq": 4e-5, "dk": 4e-5, "dv": 4e-5}  # the fp32 figures of tests/test_kernels_gpu.py, here per row
PLAIN_LSE_BAR = {torch.bfloat16: 2e-2, torch.float32: 1e-4}        # per element, as there
# instance -> margin where an instance needs more than ROW_MARGIN (DESIGN.md has the measurement and the reading of the kernel behind
# each entry); tests/test_attention_ref_cpu.py holds every table entry's fault conditions at the largest margin any mode applies to it
PLAIN_MARGIN = {}
OUTPUTS = ("o", "dq", "dk", "dv")


def plain_margin(N, dh, name, mode):
    fwd, bwd = plain_instances(N, dh, mode)
    return PLAIN_MARGIN.get(fwd if name == "o" else bwd, ROW_MARGIN)


def plain_margin_max(N, dh, name):
    return max(plain_margin(N, dh, name, mode) for mode in (0, 1, 2))


def plain_reference(qkv, d_o, B, N, H, dh, chunk=None, noise=True):
    """exact's o, lse, dqkv and, per output, row_err(rounded, exact), taken `chunk` batch items at a time."""
    chunk = chunk or B
    os_, ls, ds, worst = [], [], [], dict.fromkeys(OUTPUTS, 0.0)
    for b0 in range(0, B, chunk):
        q, d = qkv[b0:b0 + chunk], d_o[b0:b0 + chunk]
        n = q.shape[0]
        o, lse, dqkv = exact(q, d, n, N, H, dh)
        os_.append(o), ls.append(lse), ds.append(dqkv)
        if noise:
            o_r, _, dqkv_r = rounded(q, d, n, N, H, dh)
            for name, a, b in zip(OUTPUTS, (o_r,) + tuple(parts(dqkv_r, n, N, H, dh)), (o,) + tuple(parts(dqkv, n, N, H, dh))):
                worst[name] = max(worst[name], row_err(a, b, dh))
    return torch.cat(os_), torch.cat(ls), torch.cat(ds), worst


class PlainRowCase:
    """Inputs of one kind and shape and the fp64 reference of o, lse, dq, dk, dv.  bf16 storage: per output the worst row's error under
    the roundings no bf16 kernel avoids (`noise`); a row's bar is margin x noise.  fp32 storage: PLAIN_FP32_BAR.
    At N = 1 the softmax has one key and no gradient: dq and dk are zero whatever the inputs, and nothing is relative to a zero row.
    There a row is held absolutely: dS = dO.v - o.dO is the difference of two dh-term dot products of the same numbers (o = v exactly),
    which fp32 sums in any order keep within 2 dh 2^-24 |dO| |v|, and dq = dS k dh^-1/2, dk = dS q dh^-1/2."""

    def __init__(self, kind, B, N, H, dh, dtype=torch.bfloat16, chunk=None):
        self.kind, self.shape, self.dtype = kind, (B, N, H, dh), dtype
        self.qkv, self.d_o = make_inputs(kind, B, N, H, dh, dtype, seed=PLAIN_SEED)
        bf = dtype == torch.bfloat16
        self.o, self.lse, self.dqkv, noise = plain_reference(self.qkv, self.d_o, B, N, H, dh, chunk, noise=bf)
        self.ref = dict(zip(OUTPUTS, (self.o,) + tuple(parts(self.dqkv, B, N, H, dh))))
        self.noise = noise if bf else None
        self.lse_bar = PLAIN_LSE_BAR[dtype]
        self.abs_bar = {}
        if N == 1:
            if bf:
                self.noise["dq"] = self.noise["dk"] = 0.0  # (relative to a zero row: not a figure)
            q, k, v = (t.norm(dim=-1) for t in self.qkv.double().view(B, N, 3, H, dh).unbind(2))  # [B, N, H]
            ds = 2 * dh * 2.0 ** -24 * self.d_o.double().view(B, N, H, dh).norm(dim=-1) * v
            self.abs_bar = {"dq": ds * k * dh ** -0.5, "dk": ds * q * dh ** -0.5}

    def bar(self, name, margin=ROW_MARGIN):
        return margin * self.noise[name] if self.noise is not None else PLAIN_FP32_BAR[name]

    def ratios(self, name, got, margin=ROW_MARGIN, ref=None):
        """error / bar of every row of output `name`, [B, N, H]; `got` is [B, N, H * dh]."""
        B, N, H, dh = self.shape
        ref = self.ref[name] if ref is None else ref
        if name in self.abs_bar:
            err = (got.detach().double().cpu() - ref).view(B, N, H, dh).norm(dim=-1)
            return err / self.abs_bar[name]
        bar = self.bar(name, margin)
        e = row_errs(got, ref, dh)
        if bar == 0:  # no rounding at all in the reference (o and dv at N = 1 are v and dO): the row has to be exact
            return torch.where(e == 0, torch.zeros_like(e), torch.full_like(e, float("inf")))
        return e / bar

    def moves(self, name, other):
        """|other_row - reference row| / |reference row| of every row, [B, N, H]: what a fault planted in the reference moves a row by."""
        return row_errs(other, self.ref[name], self.shape[3])


def worst_row(ratios):
    """(ratio, (batch, token, head)) of the worst row; a NaN row is the worst of all."""
    r = torch.nan_to_num(ratios, nan=float("inf"))
    i = int(r.argmax())
    return float(r.flatten()[i]), tuple(int(x) for x in np.unravel_index(i, tuple(r.shape)))


def bwd4_walk(nbh, grid):
    """The persistent backward's walk, restated: workgroup w takes the items w, w + grid, w + 2 grid, ... below nbh, and item i works
    on (batch, head) pair bh(i), a permutation that hands each of the 8 XCDs (item % 8) one contiguous run of pairs, the first
    nbh % 8 runs one pair longer.  Returns (bh of every item, the turn -- 0, 1, 2, ... -- at which every bh is taken), as tensors."""
    q, r = divmod(nbh, 8)
    item = torch.arange(nbh)
    xcd = item % 8
    bh = torch.where(xcd < r, xcd * (q + 1), r * (q + 1) + (xcd - r) * q) + item // 8
    turn = torch.empty(nbh, dtype=torch.long)
    turn[bh] = item // grid
    return bh, turn


@functools.lru_cache(maxsize=None)
def plain_row_case(kind, N, dh):
    return PlainRowCase(kind, PLAIN_B, N, PLAIN_H, dh)


@functools.lru_cache(maxsize=None)
def plain_fp32_case(B, N, H, dh):
    return PlainRowCase("flat", B, N, H, dh, torch.float32)


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
