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


# ---- the plain per-row table: margin x noise lies between the roundings and a real fault ---------------------------------------------
KEY_CAP = {"o": 0.0, "dq": 0.30}    # lost key: the share of rows it may leave at or under the bar
QUERY_CAP = {"dv": 0.0, "dk": 0.30}  # lost query


def _without(t, j):
    return torch.cat((t[:, :j], t[:, j + 1:]), dim=1)


def _bars(c, N, dh):
    return {k: c.bar(k, A.plain_margin_max(N, dh, k)) for k in A.OUTPUTS}


def test_plain_table_has_three_edges_of_every_instance():
    """Of every kernel the dispatch can pick (by default or as the general pair): its lowest length, its highest, and one with a whole
    16-key tile past N.  The fp32-math kernels have no length limits."""
    lengths = {}
    for dh in (48, 64):
        for N in range(1, 609):
            for mode in (0, 2):
                for inst in A.plain_instances(N, dh, mode):
                    lengths.setdefault((inst, dh), []).append(N)
    assert len(lengths) == 2 * (5 + 1 + 3) + 4  # per head dim five row forwards, the online one, bwd2 at 4 / 8 / 16 waves; bwd3, 2 x bwd4, bwd5
    for (inst, dh), ns in lengths.items():
        have = [N for N in ns if (N, dh) in A.PLAIN_ROW_CASES]
        assert min(ns) in have and max(ns) in have, inst
        assert A.npad(max(ns)) == max(ns), inst
        assert any(A.npad(N) - N >= 16 for N in have), inst
    assert all(N % 32 and A.npad(N) > N for N, _ in A.PLAIN_DEEP_CASES) and len(A.PLAIN_DEEP_CASES) == 2 * 14


@pytest.mark.parametrize("N,dh", A.PLAIN_ROW_CASES)
def test_plain_row_bars_separate_real_faults(N, dh):
    """Faults planted in the fp64 reference, measured row by row against the bar margin x row_err(rounded, exact) that
    tests/test_attention_rows_gpu.py holds the kernels to (the largest margin any dispatch mode applies to the entry):
      lost key    key j never reaches any row's softmax (j = N - 1, N // 2): no row of o may stay under its bar, at most 0.30 of dq's;
      lost query  query j adds nothing to dK and dV: no row of dv, at most 0.30 of dk's;
      neighbour   row i holds row i + 1's values: seen in every row of o, dq, dk and dv.
    The caps are conditions on the inputs, not measurements.  `flat` inputs (q x 0.05) meet them because every key carries about 1 / N
    of every row; on unit Gaussians a few keys own a row, and up to 0.42 of the rows of o and 0.63 of dq's do not notice the loss of one
    of the others at N >= 513.  A seed or a margin that breaks a cap is the thing to change, never the cap."""
    c = A.plain_row_case("flat", N, dh)
    B, _, H, _ = c.shape
    bars = _bars(c, N, dh)
    print(f"plain rows N {N} dh {dh}: noise " + " ".join(f"{k} {c.noise[k]:.2e}" for k in A.OUTPUTS)
          + "  margin " + " ".join(f"{k} {A.plain_margin_max(N, dh, k):g}" for k in A.OUTPUTS))
    assert all(A.plain_margin_max(N, dh, k) >= A.ROW_MARGIN == 3.0 for k in A.OUTPUTS)
    if N < 2:
        return  # one token: no second key, query or row
    for j in sorted({N - 1, N // 2}):
        o2, _, dqkv2 = A.exact(_without(c.qkv, j), _without(c.d_o, j), B, N - 1, H, dh)
        got = {"o": o2, "dq": A.parts(dqkv2, B, N - 1, H, dh)[0]}
        for k, cap in KEY_CAP.items():
            unseen = float((A.row_errs(got[k], _without(c.ref[k], j), dh) <= bars[k]).double().mean())
            print(f"    lost key {j}: unseen share of {k} {unseen:.3f}")
            assert unseen <= cap, (k, j, unseen)
        Z = torch.ones(1, 1, N, 1, dtype=torch.float64)
        Z[0, 0, j, 0] = 0.0  # query j's row of P never reaches a product
        dqkv3 = A.exact(c.qkv, c.d_o, B, N, H, dh, Z)[2]
        got = dict(zip(("dq", "dk", "dv"), A.parts(dqkv3, B, N, H, dh)))
        for k, cap in QUERY_CAP.items():
            unseen = float((A.row_errs(_without(got[k], j), _without(c.ref[k], j), dh) <= bars[k]).double().mean())
            print(f"    lost query {j}: unseen share of {k} {unseen:.3f}")
            assert unseen <= cap, (k, j, unseen)
    for k in A.OUTPUTS:
        move = float(A.row_errs(c.ref[k][:, 1:], c.ref[k][:, :-1], dh).min())
        print(f"    neighbour's row: smallest move of {k} {move:.2e} (bar {bars[k]:.2e})")
        assert move > bars[k], k


@pytest.mark.parametrize("N,dh", A.PLAIN_DEEP_CASES)
def test_plain_deep_negative_rows_see_a_padded_key(N, dh):
    """One zero key with a zero value behind the last token, as a padded row of the K and V images is: every row of o moves past its bar
    (the key's score 0 stands ~100 above the row's, so o goes to about 0) and every lse by more than the lse bar."""
    c = A.plain_row_case("deep_negative", N, dh)
    B, _, H, _ = c.shape
    print(f"plain deep_negative N {N} dh {dh}: lse {float(c.lse.min()):.1f} .. {float(c.lse.max()):.1f}  noise o {c.noise['o']:.2e}")
    assert float(c.lse.max()) < -89.0
    pad = torch.zeros(B, 1, 3 * H * dh, dtype=c.qkv.dtype)
    o2, lse2, _ = A.exact(torch.cat((c.qkv, pad), dim=1), torch.cat((c.d_o, c.d_o[:, :1]), dim=1), B, N + 1, H, dh)
    assert float(A.row_errs(o2[:, :N], c.o, dh).min()) > c.bar("o", A.plain_margin_max(N, dh, "o"))
    assert float((lse2[:, :, :N] - c.lse).abs().min()) > c.lse_bar
    assert float(lse2[:, :, :N].min()) > -1.0


def test_one_token_has_no_gradient_for_q_and_k():
    """What PlainRowCase.abs_bar rests on: at N = 1 dq and dk are zero, o is v and dv is dO."""
    for dh in (48, 64):
        c = A.plain_row_case("flat", 1, dh)
        assert float(c.ref["dq"].abs().max()) <= 1e-12 and float(c.ref["dk"].abs().max()) <= 1e-12
        assert c.noise["o"] == 0.0 and c.noise["dv"] == 0.0
        assert set(c.abs_bar) == {"dq", "dk"} and all(float(v.min()) > 0 for v in c.abs_bar.values())
        assert float(c.ratios("dq", c.d_o.double()).min()) > 1e3  # rows of ordinary size in place of the zeros stand far above it


def test_bwd4_walk_is_a_permutation_with_three_turns():
    """The restated walk of the persistent backward, at the sizes tests/test_attention_rows_gpu.py picks on 256 CUs and on a smaller
    card: every (batch, head) pair exactly once, each XCD's run contiguous, the first nbh % 8 runs one longer, a third turn reached."""
    for nbh, grid in ((515, 256), (245, 120), (320, 256), (7, 256)):
        bh, turn = A.bwd4_walk(nbh, grid)
        assert sorted(bh.tolist()) == list(range(nbh))
        runs = [bh[x::8] for x in range(8)]
        assert all(torch.equal(r, torch.arange(len(r)) + int(r[0])) for r in runs if len(r))
        assert [len(r) for r in runs] == [nbh // 8 + (x < nbh % 8) for x in range(8)]
        assert int(turn.max()) == (nbh - 1) // grid and int((turn == 0).sum()) == min(nbh, grid)
    assert int(A.bwd4_walk(515, 256)[1].max()) == 2 and 515 % 8 == 3


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
