"""tests/attention_ref.py on its own: that the GPU attention tests built on it can see what they claim to see.  No kernel runs here."""
import pytest
import torch
import torch.nn.functional as F

from tests import attention_ref as A
from tests import dropout_ref as R

LSE_BAR = 2e-2  # the bf16 lse bar of tests/test_kernels_gpu.py and tests/test_dropout_gpu.py (fp32: 1e-4)
STRUCTURED = [(2, N, 3, dh, torch.bfloat16) for N, dh in A.STRUCTURED_SHAPES] + [A.STRUCTURED_FP32 + (torch.float32,)]


# ---- flat inputs: one inverted keep decision stands clear of the rounding noise -----------------------------------------------------
@pytest.mark.parametrize("B,H,N,dh,p", A.ROW_CASES)
def test_flat_rows_separate_one_flipped_keep_decision(B, H, N, dh, p):
    """Every entry of the per-row table: 3 x the error the unavoidable bf16 roundings leave in a row of o (of dV) is at most half the
    smallest move of a row when the keep decision of its lightest key (query) is inverted.  An entry that fails leaves the table."""
    c = A.row_case(B, H, N, dh, p)
    print(f"flat B {B} H {H} N {N} dh {dh} p {p}: noise o {c.noise['o']:.2e} dv {c.noise['dv']:.2e}  flip o {c.flip['o']:.2e} dv {c.flip['dv']:.2e}")
    for k in ("o", "dv"):
        assert c.bar[k] == A.ROW_MARGIN * c.noise[k] and A.ROW_MARGIN == 3.0
        assert 3 * c.noise[k] <= c.flip[k] / 2, k


def test_flip_is_the_move_of_an_inverted_decision():
    """The closed form of RowCase.flip against the thing itself: invert the decision in Z, run `exact` again, measure the row."""
    B, H, N, dh, p = 1, 2, 64, 48, 0.5
    c = A.row_case(B, H, N, dh, p)
    Z = A.keep_multiplier(B, H, N, p)
    P = A._attention(c.qkv, c.d_o, B, N, H, dh, Z, lambda t: t)[3]
    ik = P.argmin(dim=-1)  # every query's lightest key, all rows at once: a row of o depends on its own row of Z only
    Z2 = Z.clone()
    cur = torch.gather(Z, -1, ik.unsqueeze(-1))
    Z2.scatter_(-1, ik.unsqueeze(-1), R.scale(p) - cur)
    o2 = A.exact(c.qkv, c.d_o, B, N, H, dh, Z2)[0]
    moves = ((o2 - c.o).view(-1, dh).norm(dim=-1) / c.o.view(-1, dh).norm(dim=-1))
    assert abs(float(moves.min()) - c.flip["o"]) <= 1e-9 * c.flip["o"]
    iq = P.argmin(dim=-2)
    Z3 = Z.clone()
    cur = torch.gather(Z, -2, iq.unsqueeze(-2))
    Z3.scatter_(-2, iq.unsqueeze(-2), R.scale(p) - cur)
    dv3 = A.parts(A.exact(c.qkv, c.d_o, B, N, H, dh, Z3)[2], B, N, H, dh)[2]
    moves = ((dv3 - c.dv).reshape(-1, dh).norm(dim=-1) / c.dv.reshape(-1, dh).norm(dim=-1))
    assert abs(float(moves.min()) - c.flip["dv"]) <= 1e-9 * c.flip["dv"]


# ---- deep_negative: every row past the fp32 exp range, a leaked zero key unmissable -------------------------------------------------
@pytest.mark.parametrize("B,N,H,dh,dtype", STRUCTURED)
def test_deep_negative_rows_are_past_the_fp32_exp_range(B, N, H, dh, dtype):
    c = A.structured_case("deep_negative", B, N, H, dh, dtype)
    print(f"deep_negative N {N} dh {dh}: lse {float(c.lse.min()):.1f} .. {float(c.lse.max()):.1f}")
    assert float(c.lse.max()) < -89.0
    # one all-zero key behind the last token, as a padded row of the K image is: its score is 0
    qkv = c.qkv.view(B, N, 3, H, dh)
    pad = torch.zeros(B, 1, 3, H, dh, dtype=dtype)  # (its query row is not looked at)
    leaked = torch.cat((qkv, pad), dim=1).reshape(B, N + 1, 3 * H * dh)
    d_o = torch.cat((c.d_o, c.d_o[:, :1]), dim=1)
    lse2 = A.exact(leaked, d_o, B, N + 1, H, dh)[1][:, :, :N]
    assert float((lse2 - c.lse).abs().min()) > 100 * LSE_BAR


# ---- rising / falling: the maximum arrives late / early, the far end carries nothing ------------------------------------------------
@pytest.mark.parametrize("kind", ["rising", "falling"])
@pytest.mark.parametrize("B,N,H,dh,dtype", STRUCTURED)
def test_ramps_put_the_peak_at_one_end(kind, B, N, H, dh, dtype):
    """The kernels' 32-key steps start at key 0, so with N no multiple of 32 the last one holds N % 32 keys -- a single key at 129, 289
    or 513 tokens, which the keys' noise (1.6 units of logit against a ramp of 80 / (N - 1) per key) outbids for half of the rows.  The
    last step is therefore taken as the last 32 keys: the peak then lies in the kernels' last step or the one before it, behind every
    rescale but at most one."""
    c = A.structured_case(kind, B, N, H, dh, dtype)
    if kind == "rising":
        assert int(c.peak.min()) >= N - A.STEP
        far = c.first_step
    else:
        assert int(c.peak.max()) < A.STEP
        far = c.last_step
    print(f"{kind} N {N} dh {dh}: weight of the far step {float(far.max()):.1e}")
    assert float(far.max()) < 1e-6


# ---- exact ---------------------------------------------------------------------------------------------------------------------------
def test_exact_is_sdpa_autograd_in_fp64():
    B, N, H, dh = 2, 19, 3, 16
    qkv, d_o = A.make_inputs("gaussian", B, N, H, dh, torch.float32, seed=3)
    o, lse, dqkv = A.exact(qkv, d_o, B, N, H, dh)
    qr = qkv.double().requires_grad_(True)
    q, k, v = qr.view(B, N, 3, H, dh).permute(2, 0, 3, 1, 4)
    o_t = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B, N, H * dh)
    (o_t * d_o.double()).sum().backward()
    assert A.rel_err(o, o_t) <= 1e-10 and A.rel_err(dqkv, qr.grad) <= 1e-10
    s = (q @ k.transpose(-1, -2)).detach() * dh ** -0.5
    assert float((lse - torch.logsumexp(s, -1)).abs().max()) <= 1e-10
    for i, (a, b) in enumerate(zip(A.parts(dqkv, B, N, H, dh), A.parts(qr.grad, B, N, H, dh))):
        assert A.rel_err(a, b) <= 1e-10, "qkv"[i]


def test_exact_with_a_mask_is_the_dropout_restatement():
    """With Z: autograd through dropout_ref.sdpa_dropout, the form the dropout tests have used so far."""
    B, N, H, dh, p = 2, 21, 2, 16, 0.5
    qkv, d_o = A.make_inputs("gaussian", B, N, H, dh, torch.float32, seed=5)
    Z = A.keep_multiplier(B, H, N, p)
    o, _, dqkv = A.exact(qkv, d_o, B, N, H, dh, Z)
    qr = qkv.double().requires_grad_(True)
    q, k, v = qr.view(B, N, 3, H, dh).permute(2, 0, 3, 1, 4)
    o_t = R.sdpa_dropout(q, k, v, Z).transpose(1, 2).reshape(B, N, H * dh)
    (o_t * d_o.double()).sum().backward()
    assert A.rel_err(o, o_t) <= 1e-10 and A.rel_err(dqkv, qr.grad) <= 1e-10


def test_generators_are_seeded_and_rounded_to_storage():
    for kind in A.KINDS:
        a = A.make_inputs(kind, 1, 33, 2, 16, torch.bfloat16, seed=7)
        b = A.make_inputs(kind, 1, 33, 2, 16, torch.bfloat16, seed=7)
        c = A.make_inputs(kind, 1, 33, 2, 16, torch.bfloat16, seed=8)
        assert a[0].dtype == torch.bfloat16 and a[0].shape == (1, 33, 96) and a[1].shape == (1, 33, 32)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and not torch.equal(a[0], c[0])


def test_row_err_sees_one_wrong_row_that_rel_err_does_not():
    g = torch.Generator().manual_seed(0)
    b = torch.randn(2, 300, 3 * 16, generator=g)
    a = b.clone()
    a[1, 7, 16:32] *= 1.05
    assert abs(A.row_err(a, b, 16) - 0.05) < 1e-6 and A.rel_err(a, b) < 2e-3
