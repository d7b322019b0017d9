"""Yardstick of the attentive classification head (csrc/heads.hip: query attention, head_linear, channel_norm; csrc/finetune.hip: the
query attention backward) and of the copy passes its training step launches (csrc/elementwise.hip: cast, transpose-cast, column sum,
row gather): plain torch restatements of the definitions in include/headct_hip.h and at the head of the kernels.  The arithmetic runs in
the dtype of the tensors handed in (the tests hand in float64).  With `order=True` every reduction is taken in the kernel's own order; in
fp32 that shows what fp32 arithmetic alone costs, which tests/test_attn_head_ref_cpu.py holds against the bars of the GPU file.  The
second half holds the loop limits, the case lists and the input builders of tests/test_attn_head_kernels_gpu.py.  Nothing here calls the
code under test."""
import torch
import torch.nn.functional as F

from tests import head_kernels_ref as H
from tests.head_kernels_ref import (BF16, BF16_BAR, EPS, F32, F64, FP32_BAR, _butterfly, f32_scalar, gen, product_sum_bound, strided,  # noqa: F401
                                    sum_bound, sum_rows, values, worst_col, worst_row)

# ---- loop limits of the kernels (test_attn_head_ref_cpu.py asserts that every case list crosses the ones it is there to cross) ----
LANES = 64             # one wave: the lane loops of query_attention_kernel (n = lane, lane + 64, ...) and head_linear_kernel (k = lane, ...)
WAVES = 4              # waves per workgroup: the P V loop (n = wave, wave + 4, ...), the wave-per-query loop, head_linear's waves per block
LDS_FLOATS = 16384     # 64 KiB: Q N + 4 Q dh + Q (forward), 6 Q dh + 2 Q (backward)
MAX_DH = 2 * LANES     # the backward's two lane slots: d = lane and d = lane + 64
WGRAD_BLOCK = 256      # head_linear_wgrad_kernel: one thread per (c, k)
QUAD_BLOCK = H.QUAD_BLOCK   # channel_norm_kernel: 256 threads x 4 columns
CAST_TRIP = 1024       # cast_kernel: 256 threads x 4 elements per block and trip,
CAST_BLOCKS = 2048     # ... at most this many blocks: n > 2048 * 1024 takes the grid-stride loop a second time
TILE = 64              # transpose_cast_kernel: 64 x 64 tiles
COLSUM_COLS = 256      # colsum_partial_kernel: columns per block,
COLSUM_TRIP = 32       # ... rows per trip of its row loop (4 waves x 8 loads),
COLSUM_MIN_ROWS = 16   # ... and colsum_chunks: no chunk shorter than this, about COLSUM_BLOCKS blocks in all
COLSUM_BLOCKS = 1024
FOLD_GROUPS = 16       # fold_partials_kernel: chunk b is added by row group b % 16
GATHER_BLOCKS = 8192   # gather_rows16_kernel: at most this many blocks of 256 threads, one 16-byte piece per thread and trip
GATHER_THREADS = 256


def fma(a, b, c):
    """fmaf: a b + c with one rounding.  fp32: the product is exact in float64 and the sum is rounded once there, then to fp32."""
    if a.dtype == F32:
        return (a.double() * b.double() + c.double()).float()
    return a * b + c


def _pad_axis(t, axis, block):
    """`axis` padded with zeros to a multiple of `block` (a product with +0 and a sum with +0 are exact)."""
    pad = [0, 0] * (t.dim() - 1 - axis % t.dim()) + [0, -t.shape[axis] % block]
    return F.pad(t, pad)


def _lane_dot(a, b):
    """<a, b> over the last axis (<= 128) as the backward takes it: lane l holds d = l and d = l + 64, fmaf(a1, b1, a0 b0), the butterfly."""
    a, b = torch.broadcast_tensors(_pad_axis(a, -1, MAX_DH), _pad_axis(b, -1, MAX_DH))
    return _butterfly(fma(a[..., LANES:], b[..., LANES:], a[..., :LANES] * b[..., :LANES]))


def _wave_fold(acc):
    """[..., 4, dh] -> [..., dh]: (w0 + w1) + (w2 + w3)."""
    return (acc[..., 0, :] + acc[..., 1, :]) + (acc[..., 2, :] + acc[..., 3, :])


def _by_wave(w, x):
    """sum_n w[..., q, n] x[..., n, :] with wave v adding n = v, v + 4, ... by fmaf: [B, H, Q, 4, dh] before the fold."""
    wp, xp = _pad_axis(w, -1, WAVES), _pad_axis(x, -2, WAVES)
    wp = wp.reshape(*wp.shape[:-1], -1, WAVES)                    # [B, H, Q, T, 4]
    xp = xp.reshape(*xp.shape[:-2], -1, WAVES, xp.shape[-1])      # [B, H, T, 4, dh]
    acc = torch.zeros(*wp.shape[:-2], WAVES, xp.shape[-1], dtype=w.dtype)
    for t in range(wp.shape[-2]):
        acc = fma(wp[..., t, :, None], xp[:, :, None, t], acc)
    return acc


def _split(q, kv):
    """q [Q, H dh], kv [B, N, 2, H, dh] -> q [H, Q, dh], k and v [B, H, N, dh]."""
    H_, dh = kv.shape[3], kv.shape[4]
    return q.reshape(q.shape[0], H_, dh).permute(1, 0, 2), kv[:, :, 0].permute(0, 2, 1, 3), kv[:, :, 1].permute(0, 2, 1, 3)


# ---- query attention (heads.hip, finetune.hip) --------------------------------------------------------------------------------------
def logits(q, kv, logit_scale):
    qh, k, _ = _split(q, kv)
    return torch.einsum("hqd,bhnd->bhqn", qh, k) * logit_scale


def query_attention(q, kv, logit_scale, order=False):
    """(out [B, H, Q, dh], lse [B, H, Q]): out[b, h, q] = softmax_n(logit_scale <q[q, h], K[b, n, h]>) @ V[b, :, h], lse = m + log(z).
    order=True: the score is serial over d by fmaf; z is per lane over n = lane, lane + 64, ... and then the butterfly; P V is per wave
    over n = wave, wave + 4, ... by fmaf, the waves folded (w0 + w1) + (w2 + w3), and scaled by 1 / z last."""
    qh, k, v = _split(q, kv)
    if not order:
        s = logits(q, kv, logit_scale)
    else:
        s = torch.zeros(k.shape[0], k.shape[1], qh.shape[1], k.shape[2], dtype=q.dtype)
        for d in range(qh.shape[-1]):
            s = fma(qh[None, :, :, None, d], k[:, :, None, :, d], s)
        s = s * logit_scale
    m = s.max(-1).values
    p = (s - m[..., None]).exp()
    if not order:
        z, acc = p.sum(-1), torch.einsum("bhqn,bhnd->bhqd", p, v)
    else:
        lanes = _pad_axis(p, -1, LANES).reshape(*p.shape[:-1], -1, LANES)
        z = torch.zeros_like(lanes[..., 0, :])
        for trip in range(lanes.shape[-2]):
            z = z + lanes[..., trip, :]
        z, acc = _butterfly(z), _wave_fold(_by_wave(p, v))
    return acc * (1.0 / z)[..., None], m + z.log()


def query_attention_bwd(q, kv, logit_scale, out, lse, dout, order=False):
    """dict(dk, dv [B, N, H, dh], dq [Q, H dh], dk_mag, dq_mag) from out, lse and dout as handed in:
        p = exp(logit_scale <q, k> - lse),  dp = <dout, v>,  delta = <dout, out>,  ds = p (dp - delta)
        dV[n] = sum_q p dout[q],  dK[n] = logit_scale sum_q ds q[q],  dq[q] = logit_scale sum_b sum_n ds k[n]
    and the un-cancelled magnitudes logit_scale sum p (|dp| + |delta|) |q| (of dK) and ... |k| (of dq): the scale on which a row of dK
    or dq is measured, since dp - delta cancels.  order=True: both dot products and delta as 64-lane butterflies over lanes that hold
    d and d + 64; dV and dK serial over q by fmaf; dq per wave over n = wave, wave + 4, ..., folded (w0 + w1) + (w2 + w3), scaled, then
    over the batch in index order."""
    qh, k, v = _split(q, kv)
    if not order:
        s = torch.einsum("hqd,bhnd->bhqn", qh, k)
        dp = torch.einsum("bhqd,bhnd->bhqn", dout, v)
        delta = (dout * out).sum(-1)
    else:
        s = _lane_dot(qh[None, :, :, None, :], k[:, :, None, :, :])
        dp = _lane_dot(dout[:, :, :, None, :], v[:, :, None, :, :])
        delta = _lane_dot(dout, out)
    p = (s * logit_scale - lse[..., None]).exp()
    ds = p * (dp - delta[..., None])
    if not order:
        dv = torch.einsum("bhqn,bhqd->bhnd", p, dout)
        dk = torch.einsum("bhqn,hqd->bhnd", ds, qh) * logit_scale
        dq = torch.einsum("bhqn,bhnd->hqd", ds, k) * logit_scale
    else:
        dv, dk = torch.zeros_like(v), torch.zeros_like(k)
        for i in range(qh.shape[1]):
            dv = fma(p[:, :, i, :, None], dout[:, :, i, None, :], dv)
            dk = fma(ds[:, :, i, :, None], qh[None, :, i, None, :], dk)
        dk = dk * logit_scale
        dq = sum_rows(_wave_fold(_by_wave(ds, k)) * logit_scale, True)   # [B, H, Q, dh] -> [H, Q, dh], batch in index order
    w = p * (dp.abs() + delta.abs()[..., None])
    dk_mag = torch.einsum("bhqn,hqd->bhnd", w, qh.abs()) * logit_scale
    dq_mag = torch.einsum("bhqn,bhnd->hqd", w, k.abs()) * logit_scale
    flat = lambda t: t.permute(1, 0, 2).reshape(t.shape[1], -1)  # noqa: E731  [H, Q, dh] -> [Q, H dh]
    return dict(dk=dk.permute(0, 2, 1, 3), dv=dv.permute(0, 2, 1, 3), dq=flat(dq), dk_mag=dk_mag.permute(0, 2, 1, 3), dq_mag=flat(dq_mag))


def exponent_allowance(q, kv, logit_scale):
    """The fast exponential: __expf(x) is the hardware exp2 of x log2(e) rounded to fp32, an absolute error of |x| 2^-24 and more in the
    argument and so a relative one in p that grows with |x|, which no CPU restatement shows.  max |x| 2^-22 over the case's own float64
    exponent arguments x = s - max_n s (the backward's s - lse lies within the same range)."""
    s = logits(q.double(), kv.double(), logit_scale)
    return float((s.max(-1).values - s.min(-1).values).max()) * 2.0 ** -22


def worst_row_scaled(got, ref, scale):
    """The largest L2 error of a row (last axis) of got against ref, relative to the L2 norm of the same row of `scale`."""
    g, r, s = (t.detach().double().cpu() for t in (got, ref, scale))
    g, r, s = (t.reshape(-1, t.shape[-1]) for t in (g, r, s))
    assert g.shape == r.shape == s.shape and not bool(torch.isnan(g).any()), "shape mismatch or NaN in the result"
    return float(((g - r).norm(dim=1) / (s.norm(dim=1) + 1e-30)).max())


# ---- head_linear and its weight gradient, channel_norm (heads.hip) ----------------------------------------------------------------
def _mean_q(x, mean, var, eps):
    """x [rows, nq, D] -> [rows, D]: 1/nq sum_q (x - mean) (1 / sqrt(var + eps)), queries in index order (mean None: no normalisation)."""
    nq = x.shape[1]
    v = torch.zeros_like(x[:, 0])
    for i in range(nq):
        v = v + (x[:, i] if mean is None else (x[:, i] - mean) * (1.0 / (var + eps).sqrt()))
    return v / nq if nq > 1 else v


def head_linear(x, mean, var, eps, W, bias, tanh=False, order=False):
    """out [rows, n_out] = act(mean_q(norm(x)) @ W^T + bias), x [rows, nq, D].  order=True: lane l adds k = l, l + 64, ... by fmaf, then
    the butterfly, then the bias."""
    v = _mean_q(x, mean, var, eps)
    if not order:
        acc = v @ W.t()
    else:
        vp, wp = _pad_axis(v, -1, LANES), _pad_axis(W, -1, LANES)
        vp, wp = vp.reshape(vp.shape[0], 1, -1, LANES), wp.reshape(1, wp.shape[0], -1, LANES)
        acc = torch.zeros(vp.shape[0], wp.shape[1], LANES, dtype=x.dtype)
        for trip in range(vp.shape[2]):
            acc = fma(vp[:, :, trip], wp[:, :, trip], acc)
        acc = _butterfly(acc)
    if bias is not None:
        acc = acc + bias
    return acc.tanh() if tanh else acc


def head_linear_wgrad(x, mean, var, eps, dlogits, order=False):
    """(dW [n_out, D], db [n_out]): dW[c, k] = sum_b dlogits[b, c] mean_q(norm(x))[b, k], db[c] = sum_b dlogits[b, c], rows in index order."""
    v = _mean_q(x, mean, var, eps)
    if not order:
        return dlogits.t() @ v, dlogits.sum(0)
    dW = torch.zeros(dlogits.shape[1], v.shape[1], dtype=x.dtype)
    for b in range(v.shape[0]):
        dW = fma(dlogits[b][:, None], v[b][None, :], dW)
    return dW, sum_rows(dlogits, True)


def channel_norm(x, mean, var, eps):
    return (x - mean) * (1.0 / (var + eps).sqrt())


# ---- the copy passes (elementwise.hip) -----------------------------------------------------------------------------------------------
def cast(x, dtype):
    return x.to(dtype)


def transpose_cast(x, dtype):
    return x.t().contiguous().to(dtype)


def gather_rows(src, idx):
    """dst row r = src row idx[r], zeros where idx[r] < 0."""
    out = src[idx.clamp(min=0).long()]
    out[idx < 0] = 0
    return out


def colsum_chunks(rows, cols):
    """colsum_chunks of csrc/gemm_plan.h: about COLSUM_BLOCKS blocks in all, no chunk shorter than COLSUM_MIN_ROWS rows."""
    colblk = -(-cols // COLSUM_COLS)
    return max(1, min(-(-COLSUM_BLOCKS // colblk), -(-rows // COLSUM_MIN_ROWS)))


def colsum(x, order=False):
    """Column sums of x [rows, cols].  order=True: colsum_chunks chunks of ceil(rows / chunks) rows; in a chunk wave w adds rows w, w + 4,
    ... and the waves fold (0 + 1) + (2 + 3); chunk b goes to row group b % 16 of fold_partials_kernel, the groups are added in order."""
    if not order:
        return x.sum(0)
    rows, cols = x.shape
    chunks = colsum_chunks(rows, cols)
    rpc = -(-rows // chunks)
    xc = _pad_axis(_pad_axis(x, 0, chunks * rpc)[:chunks * rpc].reshape(chunks, rpc, cols), 1, WAVES).reshape(chunks, -1, WAVES, cols)
    acc = torch.zeros(chunks, WAVES, cols, dtype=x.dtype)
    for t in range(xc.shape[1]):
        acc = acc + xc[:, t]
    part = _pad_axis(_wave_fold(acc), 0, FOLD_GROUPS).reshape(-1, FOLD_GROUPS, cols)
    grp = torch.zeros(FOLD_GROUPS, cols, dtype=x.dtype)
    for t in range(part.shape[0]):
        grp = grp + part[t]
    return sum_rows(grp, True)


# measured: the worst error of the order=True restatement in fp32 against float64, for the cases where it exceeds a tenth of the bar that
# the case would otherwise take (tests/test_attn_head_ref_cpu.py asserts each entry against the measurement: not below it, not above
# twice it).  The GPU bar of such a case is TEN times the entry (H.bar, whose table these entries join).  A "peaked" case adds its
# exponent allowance to that bar; the comment beside it holds the allowance and the error the kernel showed on an MI355X.
RESTATEMENT = {
    # Q = 1: dK[n] = ls ds q is a single term, and on a token whose dp and delta both happen to be small the dot products' own rounding shows
    ("query_attention", 2, 64, 1, 4, "moderate", F32, "dk"): 3.92e-06,
    ("query_attention", 2, 217, 1, 4, "moderate", F32, "dk"): 4.17e-06,
    ("query_attention", 2, 65, 1, 16, "moderate", F32, "dk"): 2.30e-06,
    ("query_attention", 2, 217, 1, 16, "moderate", F32, "dk"): 1.58e-06,
    ("query_attention", 2, 65, 1, 48, "moderate", F32, "dk"): 1.74e-06,
    ("query_attention", 2, 217, 1, 48, "moderate", F32, "dk"): 2.96e-06,
    ("query_attention", 2, 5, 1, 64, "moderate", F32, "dk"): 2.29e-06,
    ("query_attention", 2, 64, 1, 64, "moderate", F32, "dk"): 1.43e-06,
    ("query_attention", 2, 65, 1, 64, "moderate", F32, "dk"): 3.28e-06,
    ("query_attention", 2, 217, 1, 64, "moderate", F32, "dk"): 3.40e-06,
    ("query_attention", 2, 64, 1, 72, "moderate", F32, "dk"): 1.46e-06,
    ("query_attention", 2, 65, 1, 72, "moderate", F32, "dk"): 2.67e-06,
    ("query_attention", 2, 217, 1, 72, "moderate", F32, "dk"): 1.24e-05,
    ("query_attention", 2, 64, 1, 128, "moderate", F32, "dk"): 3.04e-06,
    ("query_attention", 2, 65, 1, 128, "moderate", F32, "dk"): 4.39e-06,
    ("query_attention", 2, 217, 1, 128, "moderate", F32, "dk"): 5.24e-06,
    ("query_attention", 2, 65, 4, 4, "moderate", F32, "dv"): 1.33e-06,
    ("query_attention", 2, 217, 4, 4, "moderate", F32, "out"): 1.84e-06,
    # logits of +-22, exponent arguments down to -39.5: the allowance is 9.4e-6 on top of ten times the entry.  On an MI355X the kernel
    # showed, fp32 kv: out 2.1e-6, dV 1.8e-6, dK 1.6e-6, dq 9.6e-8; bf16 kv: out 2.5e-6, dq 1.1e-7 (dV and dK there are the bf16 store, 2.4e-3)
    ("query_attention", 2, 217, 4, 64, "peaked", F32, "out"): 2.75e-06,
    ("query_attention", 2, 217, 4, 64, "peaked", F32, "dv"): 2.13e-06,
    ("query_attention", 2, 217, 4, 64, "peaked", F32, "dk"): 2.12e-06,
    ("query_attention", 2, 217, 4, 64, "peaked", BF16, "out"): 3.28e-06,
    ("query_attention", 2, 217, 4, 128, "moderate", F32, "out"): 1.30e-06,
    ("query_attention", 1, 16319, 1, 16, "moderate", BF16, "out"): 2.00e-06,   # the LDS boundary: a mean of 16319 values
}
H.RESTATEMENT.update(RESTATEMENT)


def bar(key, default, allowance=0.0):
    return H.bar(key, default) + allowance


# =================================================================================================================================
# Inputs and cases of tests/test_attn_head_kernels_gpu.py.  Everything is made on the CPU from seeded generators.
# =================================================================================================================================
ATTN_N = (1, 3, 4, 5, 64, 65, 217)      # idle waves in P V; a whole trip of them; a ragged one; a lane trip; its second trip; three and a ragged fourth
ATTN_Q = (1, 4, 5)                      # 5: a second trip of the wave-per-query loop
ATTN_DH = (4, 16, 48, 64, 72, 128)      # 48: sixteen idle lanes in the backward; 64: the first slot full; 72, 128: the second slot
ATTN_B, ATTN_H = 2, 3
ATTN_CASES = [(N, Q, dh) for Q in ATTN_Q for dh in ATTN_DH for N in ATTN_N]
ATTN_GROUPS = [(Q, dh) for Q in ATTN_Q for dh in ATTN_DH]
ATTN_PEAKED_CASE = (217, 4, 64)
ATTN_CHAINED_N = (65, 217)              # the backward also run after the kernel's own forward
ATTN_BATCH_CASE, ATTN_BATCHES = (65, 4, 72), (1, 2, 5)
ATTN_LDS_CASES = [(1, 16, 16319), (4, 64, 3839)]   # (Q, dh, N) with Q N + 4 Q dh + Q = LDS_FLOATS exactly, B = H = 1
ATTN_EQUAL_KEY_N = (1, 4, 64)           # powers of two: p = 1 / N exactly
ATTN_KINDS = ("moderate", "peaked", "int")


def attn_inputs(B, N, H_, Q, dh, kind, kv_dtype):
    """"moderate": randn q / k / v with logit_scale = dh^-0.5; "peaked": q scaled so that max |logit| = 22 on the rounded kv."""
    g = gen(B, N, H_, Q, dh, ATTN_KINDS.index(kind), 41)
    q, kv = torch.randn(Q, H_ * dh, generator=g), torch.randn(B, N, 2, H_, dh, generator=g).to(kv_dtype)
    dout = torch.randn(B, H_, Q, dh, generator=g)
    ls = f32_scalar(dh ** -0.5)
    if kind == "peaked":
        q = (q.double() * (22.0 / float(logits(q.double(), kv.double(), ls).abs().max()))).float()
    return dict(q=q, kv=kv, dout=dout, ls=ls)


def attn_equal_key_inputs(N, kv_dtype):
    """Q = 1, integer-valued, every key of a (volume, head) the same vector and orthogonal to the query: every logit is exactly 0, p = 1 / N,
    out the plain mean of V, lse = log N, and dV[n] = dout / N."""
    B, H_, dh = 2, 3, 16
    g = gen(N, 42)
    q = torch.zeros(H_, dh)
    q[:, 0], q[:, 1] = torch.arange(1.0, H_ + 1), -torch.arange(1.0, H_ + 1)
    kv = values((B, N, 2, H_, dh), "int", g)
    kv[:, :, 0] = torch.arange(1.0, B * H_ + 1).reshape(B, 1, H_, 1)
    return dict(q=q.reshape(1, H_ * dh), kv=kv.to(kv_dtype), dout=values((B, H_, 1, dh), "int", g), ls=0.25)


def attn_runs(Q, dh):
    """(key, inputs, variant) of every forward / backward case of one (Q, dh) group."""
    for N, q_, d_ in ATTN_CASES:
        if (q_, d_) != (Q, dh):
            continue
        for kv_dtype in (F32, BF16):
            for kind in ("moderate", "peaked") if (N, Q, dh) == ATTN_PEAKED_CASE else ("moderate",):
                for B in ATTN_BATCHES if (N, Q, dh) == ATTN_BATCH_CASE and kind == "moderate" else (ATTN_B,):
                    inp = attn_inputs(B, N, ATTN_H, Q, dh, kind, kv_dtype)
                    allow = exponent_allowance(inp["q"], inp["kv"], inp["ls"]) if kind == "peaked" else 0.0
                    yield ("query_attention", B, N, Q, dh, kind, kv_dtype), inp, dict(kind=kind, kv_dtype=kv_dtype, allowance=allow)


def attn_lds_runs():
    """The forward at the 64 KiB boundary of its LDS image, B = H = 1."""
    for Q, dh, N in ATTN_LDS_CASES:
        for kv_dtype in (F32, BF16):
            inp = attn_inputs(1, N, 1, Q, dh, "moderate", kv_dtype)
            yield ("query_attention", 1, N, Q, dh, "moderate", kv_dtype), inp, dict(kind="moderate", kv_dtype=kv_dtype, allowance=0.0)


def attn_ref(inp, var, dt=F64, order=False, fwd=None, bwd=True):
    """The figures of one case.  The backward is fed the float64 forward's out and lse rounded to fp32 (fwd: another pair)."""
    q, kv, dout = inp["q"].to(dt), inp["kv"].to(dt), inp["dout"].to(dt)
    out, lse = query_attention(q, kv, inp["ls"], order)
    if not bwd:
        return dict(out=out, lse=lse)
    o_in, l_in = fwd if fwd is not None else (t.float() for t in query_attention(inp["q"].double(), inp["kv"].double(), inp["ls"]))
    res = query_attention_bwd(q, kv, inp["ls"], o_in.to(dt), l_in.to(dt), dout, order)
    return dict(res, out=out, lse=lse)


def attn_errors(key, var, got, ref):
    """{key + (figure,): (error, bar)}: out and dV per row against themselves, dK and dq per row against the un-cancelled magnitude, lse
    absolutely at 1e-5 max(1, |lse|) (error / bound, bar 1)."""
    stored = BF16_BAR if var["kv_dtype"] == BF16 else FP32_BAR
    fig = {}
    if "out" in got:
        fig["out"] = (worst_row(got["out"], ref["out"]), FP32_BAR)
        l = ref["lse"].double()
        fig["lse"] = (float(((got["lse"].double() - l).abs() / (FP32_BAR * l.abs().clamp(min=1.0))).max()), None)
    if "dv" in got:
        fig["dv"] = (worst_row(got["dv"], ref["dv"]), stored)
        fig["dk"] = (worst_row_scaled(got["dk"], ref["dk"], ref["dk_mag"]), stored)
        fig["dq"] = (worst_row_scaled(got["dq"], ref["dq"], ref["dq_mag"]), FP32_BAR)
    return {key + (k,): (e, 1.0 if b is None else bar(key + (k,), b, var["allowance"]), 1.0 if b is None else b) for k, (e, b) in fig.items()}


# ---- head_linear ---------------------------------------------------------------------------------------------------------------------
HL_D = (1, 63, 64, 65, 768)                                  # the lane loop: one lane; all but one; a whole trip; a second; twelve
HL_OUT = [(1, 1), (3, 1), (2, 2), (1, 5), (13, 1)]           # (rows, n_out): 1, 3, 4, 5, 13 waves, four to a block
HL_NQ, HL_PAD = (1, 3), (0, 8)
HL_VARIANTS = [(True, True, False), (False, False, False), (True, False, True), (False, True, True)]   # (mean / var, bias, tanh)
HL_BWD_CASES = [(B, D, n_out) for D in HL_D for B, n_out in ((1, 1), (3, 2), (13, 5))] + [(3, 130, 2)]  # 2 x 130 > WGRAD_BLOCK
HL_KINDS = ("int", "normal")


def hl_inputs(rows, D, n_out, nq, kind="normal"):
    """x [rows, nq, D] around 1 with a scale per row, W of one sign per class and of magnitude 1 / D (the output stays of order 1, where
    tanh still moves), statistics as eval mode hands them in.  "int": small integers, x a multiple of nq (the mean over q is exact)."""
    g = gen(rows, D, n_out, nq, HL_KINDS.index(kind), 43)
    if kind == "int":
        x, dl = values((rows, nq, D), "int", g) * nq, values((rows, n_out), "int", g)
    else:
        x = (1.0 + 0.5 * torch.randn(rows, nq, D, generator=g)) * torch.linspace(0.3, 2.0, rows)[:, None, None]
        dl = torch.randn(rows, n_out, generator=g)
    sign = torch.where(torch.arange(n_out) % 2 == 0, 1.0, -1.0)[:, None]
    return dict(x=x, W=(0.5 + torch.rand(n_out, D, generator=g)) * sign / D, bias=0.1 * torch.randn(n_out, generator=g),
                mean=0.1 * torch.randn(D, generator=g), var=0.5 + torch.rand(D, generator=g), dlogits=dl)


def hl_runs(D):
    for rows, n_out in HL_OUT:
        for nq in HL_NQ:
            base = hl_inputs(rows, D, n_out, nq)
            for xdt in (F32, BF16):
                inp = dict(base, x=base["x"].to(xdt))
                for stats, bias, tanh in HL_VARIANTS:
                    if tanh and xdt == BF16:   # hct_head_linear_x has no activation
                        continue
                    yield ("head_linear", rows, D, n_out, nq, xdt, stats, bias, tanh), inp, dict(xdt=xdt, stats=stats, bias=bias, tanh=tanh, nq=nq)


def hl_ref(inp, var, dt=F64, order=False):
    mean, v = (inp["mean"].to(dt), inp["var"].to(dt)) if var["stats"] else (None, None)
    return head_linear(inp["x"].to(dt), mean, v, EPS, inp["W"].to(dt), inp["bias"].to(dt) if var["bias"] else None, var["tanh"], order)


def hl_error(key, var, got, ref):
    """tanh: the worst absolute error (tanh is bounded by 1); else the worst row."""
    e = float((got.double() - ref.double()).abs().max()) if var["tanh"] else worst_row(got, ref)
    return e, bar(key + ("out",), FP32_BAR), FP32_BAR


def hl_bwd_runs(B, D, n_out):
    for nq in HL_NQ:
        for kind in HL_KINDS:
            base = hl_inputs(B, D, n_out, nq, kind)
            for xdt in (F32, BF16):
                for stats in (False, True):
                    inp = dict(base, x=base["x"].to(xdt))
                    yield ("head_linear_bwd", B, D, n_out, nq, kind, xdt, stats), inp, dict(kind=kind, xdt=xdt, stats=stats, nq=nq)


def hl_bwd_ref(inp, var, dt=F64, order=False):
    mean, v = (inp["mean"].to(dt), inp["var"].to(dt)) if var["stats"] else (None, None)
    return head_linear_wgrad(inp["x"].to(dt), mean, v, EPS, inp["dlogits"].to(dt), order)


def hl_bwd_limits(inp, var):
    """((bound of dW, bound of db), exact): B products of dlogits and v by fmaf, v itself from up to 8 + nq roundings (x - mean, var + eps,
    the root, the reciprocal, the product, the sum over q, the division) of terms |x - mean| rstd; db a plain sum.  Exact on "int" inputs
    without statistics, where v is an integer."""
    x, dl = inp["x"].double(), inp["dlogits"].double()
    B = x.shape[0]
    xa = (x if not var["stats"] else channel_norm(x, inp["mean"].double(), inp["var"].double(), EPS)).abs().mean(1)
    dW = product_sum_bound(B, (8 + var["nq"]) if var["stats"] or var["nq"] > 1 else 0, dl.abs().t() @ xa)
    return (dW, sum_bound(torch.tensor(B), dl.abs().sum(0))), var["kind"] == "int" and not var["stats"]


# ---- channel_norm ----------------------------------------------------------------------------------------------------------------------
CN_CASES = [(1, 4), (7, 260), (5, 1028), (300, 48)]   # a quad's column is (4 i) % C; 1, 455, 1285 and 3600 quads: the last block is ragged
CN_REFUSED_C = 6


def cn_runs(rows, C):
    for key, inp, var in H.norm_runs(rows, C):
        if var["xdt"] == F32:
            yield ("channel_norm",) + key[1:], inp, var


# ---- the copy passes -------------------------------------------------------------------------------------------------------------------
CAST_N = (1, 3, 4, 5, 1023, 1025, CAST_BLOCKS * CAST_TRIP + 5)   # a scalar tail alone; a quad; quad + tail; a block; the second trip + tail
DTYPE_PAIRS = [(F32, BF16), (BF16, F32), (F32, F32), (BF16, BF16)]
TRANSPOSE_CASES = [(1, 1), (63, 65), (64, 64), (65, 130), (300, 130)]
COLSUM_COLS_LIST = (4, 256, 260)
COLSUM_PAD = (0, 8)
GATHER_ROW_BYTES = (16, 48, 1536)
GATHER_BIG = (21846, 1536)    # n_rows x row_bytes / 16 = 2097216 pieces, just past GATHER_BLOCKS x GATHER_THREADS
GATHER_REFUSED_BYTES = 24


def colsum_rows(cols):
    """Row counts by colsum_chunks: one chunk; two chunks with a ragged second; the most chunks there are, each of 33 rows (a second trip of
    the 32-row loop) but a ragged last."""
    cap = -(-COLSUM_BLOCKS // -(-cols // COLSUM_COLS))
    return (13, 29, (COLSUM_TRIP + 1) * cap - 7)


def cast_values(n, dtype, seed):
    """Normal values over six decades, rounded to `dtype`; from the third element on fp32 holds ties of the bf16 rounding (round to even)."""
    g = gen(n, seed)
    x = torch.randn(n, generator=g) * torch.pow(10.0, torch.randint(-3, 4, (n,), generator=g).float())
    ties = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(2.0 + 2.0 ** -7), 2.0 ** -100 * (1.0 + 2.0 ** -8)])
    x[2:2 + len(ties)] = ties[:max(0, min(len(ties), n - 2))]
    return x.to(dtype)


def gather_index(n_rows, n_src, seed):
    """Rows of the source in random order with repeats; every fifth entry -1, and the first and the last."""
    idx = torch.randint(0, n_src, (n_rows,), generator=gen(n_rows, n_src, seed)).to(torch.int32)
    idx[::5] = -1
    idx[-1] = -1
    if n_rows > 3:
        idx[1], idx[2], idx[3] = n_src - 1, n_src - 1, 0
    return idx
