"""GPU: the plain (no-dropout) attention kernels row by row.  Every (batch, token, head) row of o, dq, dk and dv against the fp64
reference of tests/attention_ref.py, at the edges of every instance the dispatch can pick and in all three dispatch modes; the
persistent backward's walk past its second item with a remainder in its XCD permutation; and every operand inside guarded memory.
tests/test_attention_ref_cpu.py shows that the bars used here separate a lost key, a lost query and a neighbour's row from rounding."""
import itertools

import pytest
import torch

from headct_foundation_amd import _lib
from headct_foundation_amd._lib import HCT_BF16, HCT_F32
from tests import attention_ref as A

pytestmark = pytest.mark.gpu

MODES = (0, 1, 2)  # hct_debug_force_simple_attention: the default dispatch, the fp32-math kernels, the general MFMA pair
GUARD_ROWS = 64
PATTERN = {torch.bfloat16: (torch.int16, 0x7FA5), torch.float32: (torch.int32, 0x7FA55AA5)}  # NaNs with a payload no kernel produces


def _st():
    return torch.cuda.current_stream().cuda_stream


def _dt(t):
    return HCT_BF16 if t.dtype == torch.bfloat16 else HCT_F32


def _nan(shape, dtype, dev):
    return torch.full(shape, float("nan"), dtype=dtype, device=dev)


def _forward(lib, qkv, B, N, H, dh, o, lse):
    _lib.check(lib.hct_attention_fwd(qkv.data_ptr(), B, N, H, dh, _dt(qkv), o.data_ptr(), lse.data_ptr(), _st()), "fwd")


def _backward(lib, qkv, o, d_o, lse, B, N, H, dh, dqkv):
    _lib.check(lib.hct_attention_bwd(qkv.data_ptr(), o.data_ptr(), d_o.data_ptr(), lse.data_ptr(), B, N, H, dh, _dt(qkv), dqkv.data_ptr(),
                                     _st()), "bwd")


def _run(lib, cuda, c, mode, backward=True):
    """o, lse, dqkv (None without the backward) of case c on the CPU, every output pre-filled with NaN."""
    B, N, H, dh = c.shape
    qkv, d_o = c.qkv.to(cuda), c.d_o.to(cuda)
    lib.hct_debug_force_simple_attention(mode)
    try:
        o, lse = _nan((B, N, H * dh), c.dtype, cuda), _nan((B, H, N), torch.float32, cuda)
        _forward(lib, qkv, B, N, H, dh, o, lse)
        dqkv = None
        if backward:
            dqkv = torch.full_like(qkv, float("nan"))
            _backward(lib, qkv, o, d_o, lse, B, N, H, dh, dqkv)
        torch.cuda.synchronize()
    finally:
        lib.hct_debug_force_simple_attention(0)
    return o.cpu(), lse.cpu(), None if dqkv is None else dqkv.cpu()


def _hold_rows(c, mode, o, lse, dqkv, tag, batches=None):
    """Print, per output, the worst row's error / bar and its (batch, token, head), then hold every row, lse per element, and finiteness."""
    B, N, H, dh = c.shape
    got = {"o": o}
    if dqkv is not None:
        got.update(zip(("dq", "dk", "dv"), A.parts(dqkv, B, N, H, dh)))
    bf = c.dtype == torch.bfloat16
    worst = {}
    for k, t in got.items():
        margin = A.plain_margin(N, dh, k, mode) if bf else 1.0
        r = c.ratios(k, t, margin)
        if batches is not None:  # only the rows of batch item `batches`
            r = torch.where(torch.arange(B).view(B, 1, 1) == batches, r, torch.zeros_like(r))
        worst[k] = A.worst_row(r) + (margin,)
    e_l = float(torch.nan_to_num((lse - c.lse).abs(), nan=float("inf")).max())
    inst = A.plain_instances(N, dh, mode) if bf else ("simple_fwd", "simple_bwd")
    print(f"{tag} N {N} dh {dh} mode {mode} {inst[0]} {inst[1]}: lse {e_l:.2e} (bar {c.lse_bar:.0e})  "
          + "  ".join(f"{k} {w[0]:.3f} x bar (margin {w[2]:g}) at {w[1]}" for k, w in worst.items()))
    assert torch.isfinite(lse).all() and all(torch.isfinite(t.float()).all() for t in got.values()), (mode, "not finite")
    assert e_l < c.lse_bar, (mode, "lse", e_l)
    for k, w in worst.items():
        assert w[0] <= 1.0, f"mode {mode}: {k} row (batch, token, head) = {w[1]} is at {w[0]:.3f} x its bar"


@pytest.mark.parametrize("N,dh", A.PLAIN_ROW_CASES)
def test_plain_attention_every_row(lib, cuda, N, dh):
    """`flat` inputs at B = 2, H = 3, bf16: every row of o, dq, dk, dv under margin x row_err(rounded, exact) of its own output (at
    N = 1, where dq and dk are zero, under PlainRowCase's absolute bar), lse per element under 2e-2, in all three dispatch modes."""
    c = A.plain_row_case("flat", N, dh)
    for mode in MODES:
        _hold_rows(c, mode, *_run(lib, cuda, c, mode), "plain rows")


@pytest.mark.parametrize("B,N,H,dh", A.PLAIN_FP32_CASES)
def test_plain_attention_every_row_fp32(lib, cuda, B, N, H, dh):
    """fp32 storage (the fp32-math kernels, whatever the mode): the file-wide fp32 bars of tests/test_kernels_gpu.py, per row."""
    c = A.plain_fp32_case(B, N, H, dh)
    _hold_rows(c, 0, *_run(lib, cuda, c, 0), "plain rows fp32")


@pytest.mark.parametrize("N,dh", A.PLAIN_DEEP_CASES)
def test_plain_attention_deep_negative_rows(lib, cuda, N, dh):
    """Forward only, at every table length with padded keys: a padded key that reaches one row's softmax sends that row of o to about
    0 and its lse above -1 (tests/test_attention_ref_cpu.py), so o is held per row and lse per element.  The gradients of this kind
    stay with test_attention_structured_inputs and its global bars."""
    c = A.plain_row_case("deep_negative", N, dh)
    for mode in MODES:
        o, lse, _ = _run(lib, cuda, c, mode, backward=False)
        _hold_rows(c, mode, o, lse, None, "plain deep_negative")


@pytest.mark.parametrize("N,dh", [(129, 64), (193, 48)])
def test_bwd4_walks_three_items(lib, cuda, N, dh):
    """The persistent backward with more than two (batch, head) items per workgroup and B H no multiple of 8: the third item goes back
    into LDS buffer 0, and the XCD-contiguous permutation of the walk has a remainder.  Every row of dq, dk, dv against the fp64
    reference under the per-row bars; a failure names the item b H + h and its turn in its workgroup's walk."""
    assert A.plain_instances(N, dh)[1].startswith("bwd4")
    ncu = torch.cuda.get_device_properties(cuda).multi_processor_count
    H = 5
    B = next(b for b in itertools.count(2 * ncu // H + 1) if b * H > 2 * ncu and (b * H) % 8)
    nbh, grid = B * H, ncu
    turn = A.bwd4_walk(nbh, grid)[1]
    assert int(turn.max()) >= 2 and nbh % 8
    c = A.PlainRowCase("flat", B, N, H, dh, chunk=8)
    _, _, dqkv = _run(lib, cuda, c, 0)
    assert torch.isfinite(dqkv.float()).all()
    bad = []
    for k, t in zip(("dq", "dk", "dv"), A.parts(dqkv, B, N, H, dh)):
        r = torch.nan_to_num(c.ratios(k, t, A.plain_margin(N, dh, k, 0)), nan=float("inf")).amax(dim=1).flatten()  # [B * H]: worst row per item
        per_turn = [float(r[turn == n].max()) for n in range(int(turn.max()) + 1)]
        print(f"bwd4 walk N {N} dh {dh} B {B} H {H} grid {grid}: {k} worst row x bar per turn " + " ".join(f"{x:.3f}" for x in per_turn))
        bad += [f"{k}: item {bh} (turn {int(turn[bh]) + 1} of its workgroup) at {float(r[bh]):.3f} x bar" for bh in torch.nonzero(r > 1.0).flatten().tolist()]
    assert not bad, "; ".join(bad[:8]) + (f" ... {len(bad)} in all" if len(bad) > 8 else "")


def _tailed(t, row, fill):
    """t at the start of a larger allocation whose last GUARD_ROWS rows of `row` elements hold `fill`."""
    flat = torch.full((t.numel() + GUARD_ROWS * row,), fill, dtype=t.dtype, device=t.device)
    flat[:t.numel()] = t.flatten()
    return flat, flat[:t.numel()].view(t.shape)


def _fenced(shape, row, dtype, dev):
    """(allocation as integers, NaN-filled view of `shape`) with GUARD_ROWS rows of `row` sentinel elements before and after the view."""
    itype, pattern = PATTERN[dtype]
    n, g = int(torch.tensor(shape).prod()), GUARD_ROWS * row
    raw = torch.full((g + n + g,), pattern, dtype=itype, device=dev)
    view = raw.view(dtype)[g:g + n].view(shape)
    view.fill_(float("nan"))
    return raw, view


def _fences_intact(raw, n, row, dtype):
    g = GUARD_ROWS * row
    pattern = PATTERN[dtype][1]
    return bool((raw[:g] == pattern).all()) and bool((raw[g + n:] == pattern).all())


# one length with padded rows per forward / backward instance: row-4 + bwd3, row-10 + bwd4<64,160>, row-14 + bwd4<48,224>, row-18 + bwd2 (8 waves),
# row-34 + bwd2 (16 waves), row-34 + bwd5, online forward + bwd5; mode 2 adds the online forward and bwd2 at each
@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("N,dh", [(33, 64), (129, 64), (193, 48), (225, 48), (289, 64), (449, 48), (545, 48)])
def test_attention_buffers_are_guarded(lib, cuda, N, dh, mode):
    """qkv, the o and d_o the backward reads and its lse each end where 64 rows of NaN (+inf behind lse) begin; o, lse and dqkv lie
    between 64 rows of a sentinel pattern on either side.  The sentinels must come back bit for bit, everything must be finite, and every
    row -- the last batch item's above all, whose rows past N are the NaN tails -- must meet the per-row bars."""
    c = A.plain_row_case("flat", N, dh)
    B, _, H, _ = c.shape
    nan, bf = float("nan"), torch.bfloat16
    _, qkv = _tailed(c.qkv.to(cuda), 3 * H * dh, nan)
    _, d_o = _tailed(c.d_o.to(cuda), H * dh, nan)
    raw_o, o = _fenced((B, N, H * dh), H * dh, bf, cuda)
    raw_l, lse = _fenced((B, H, N), N, torch.float32, cuda)
    raw_d, dqkv = _fenced((B, N, 3 * H * dh), 3 * H * dh, bf, cuda)
    lib.hct_debug_force_simple_attention(mode)
    try:
        _forward(lib, qkv, B, N, H, dh, o, lse)
        _, o_in = _tailed(o, H * dh, nan)
        _, lse_in = _tailed(lse, N, float("inf"))
        _backward(lib, qkv, o_in, d_o, lse_in, B, N, H, dh, dqkv)
        torch.cuda.synchronize()
    finally:
        lib.hct_debug_force_simple_attention(0)
    assert _fences_intact(raw_o, o.numel(), H * dh, bf), "o: written outside"
    assert _fences_intact(raw_l, lse.numel(), N, torch.float32), "lse: written outside"
    assert _fences_intact(raw_d, dqkv.numel(), 3 * H * dh, bf), "dqkv: written outside"
    _hold_rows(c, mode, o.cpu(), lse.cpu(), dqkv.cpu(), "guarded, last batch item", batches=B - 1)
    _hold_rows(c, mode, o.cpu(), lse.cpu(), dqkv.cpu(), "guarded, all rows")
