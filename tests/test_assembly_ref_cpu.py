"""Pins tests/assembly_ref.py before tests/test_assembly_kernels_gpu.py uses it as a yardstick: agreement with the oracle, the
hand-written loss gradient against autograd, the restatements' own fp32 error against the GPU bars, and the stated properties of
every input that the GPU tests build (exact integer sums, batch sizes and row counts past the loop limits they are there to cross).
No GPU, no library."""
import pytest
import torch

from oracle import mae_oracle as O
from tests import assembly_ref as A

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
FP32_BAR, DEGENERATE_BAR = 1e-5, 1e-3  # the GPU test's bars; the restatement in fp32 must hold a tenth of them


# ---- against the oracle -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["micro", "yaml_cut"])
def test_references_agree_with_the_oracle(name):
    cfg = O.CONFIGS[name]
    B, P, C, S, K = 3, cfg.patch_size, cfg.in_chans, cfg.input_size, cfg.len_keep
    x, noise = O.make_volume(cfg, B, 2).double(), O.make_noise(cfg, B, 2)
    noise[1, 5] = noise[1, 2]  # a tie: both sides rank the lower index first
    ids_shuffle, ids_restore, ids_keep, mask = O.random_masking_from_noise(cfg, noise)
    r_restore, r_shuffle, r_mask = A.mask_rank(noise, K)
    assert torch.equal(r_restore, ids_restore) and torch.equal(r_shuffle, ids_shuffle) and torch.equal(r_mask, mask)
    rows = O.patchify(cfg, x)
    assert torch.equal(A.patchify(x, P), rows) and torch.equal(A.unpatchify(rows, C, S, P), x)
    assert torch.equal(A.unpatchify(rows, C, S, P), O.unpatchify(cfg, rows))
    # Conv3d order: the patch embedding as a matrix product over the gathered rows is the oracle's convolution
    w = torch.randn(5, C, P, P, P, dtype=torch.float64, generator=A.gen(7))
    conv = torch.nn.functional.conv3d(x, w, stride=P).flatten(2).transpose(1, 2)  # [B, L, 5]
    assert torch.allclose(A.patch_rows(x, P) @ w.reshape(5, -1).t(), conv, rtol=1e-12, atol=1e-12)
    kept = A.patch_gather(x, ids_shuffle, P, K).reshape(B, K, -1)
    assert torch.equal(kept, torch.gather(A.patch_rows(x, P), 1, ids_keep.unsqueeze(-1).expand(-1, -1, kept.shape[-1])))
    # the loss inside forward: the oracle computes it from its own pred
    params = {k: v.double() for k, v in O.make_params(cfg, 2).items()}
    loss, pred, o_mask, _ = O.forward(cfg, params, x, noise)
    full = torch.cat((torch.full_like(pred[:, :1], float("nan")), pred), dim=1)
    r_loss, r_row, _ = A.masked_mse(full, x, mask, P, cfg.norm_pix_loss)
    assert abs(float(r_loss) - float(loss)) <= 1e-13 * abs(float(loss)) and torch.equal(o_mask, mask)
    assert bool((r_row[mask == 0] == 0).all())


def test_assembly_forwards_are_the_oracles_gathers():
    """encoder / decoder assembly against the torch.gather / torch.cat sequence of the oracle's forward (mae.py:212, 233-234, 257-265)."""
    B, L, K, D = 3, 64, 13, 8
    _, ids_restore, ids_shuffle, _ = A.permutations(B, L, K, 1)
    g = A.gen(3)
    tok, cls, pos = torch.randn(B, L, D, generator=g).double(), torch.randn(D, generator=g).double(), torch.randn(L, D, generator=g).double()
    xm = torch.gather(tok + pos, 1, ids_shuffle[:, :K].unsqueeze(-1).repeat(1, 1, D))
    want = torch.cat((cls.expand(B, 1, D), xm), dim=1)
    kept_tok = torch.gather(tok, 1, ids_shuffle[:, :K].unsqueeze(-1).repeat(1, 1, D)).reshape(B * K, D)
    assert torch.equal(A.encoder_assemble(kept_tok, cls, pos, ids_shuffle, B, K), want)
    e, mtok, dcls = torch.randn(B, K + 1, D, generator=g).double(), torch.randn(D, generator=g).double(), torch.randn(D, generator=g).double()
    y_ = torch.cat([e[:, 1:], mtok.reshape(1, 1, D).repeat(B, L - K, 1)], dim=1)
    y_ = torch.gather(y_, 1, ids_restore.unsqueeze(-1).repeat(1, 1, D))
    y = torch.cat([e[:, :1], y_], dim=1) + torch.cat((dcls.expand(B, 1, D), pos.expand(B, L, D)), dim=1)
    assert torch.equal(A.decoder_assemble(e, mtok, dcls, pos, ids_restore, K), y)
    reg = torch.randn(2, D, generator=g).double()
    h = A.vit_assemble(tok.reshape(B * L, D), cls, reg, pos, B)
    assert h.shape == (B, 3 + L, D) and torch.equal(h[:, 0], cls.expand(B, D)) and torch.equal(h[:, 1:3], reg.expand(B, 2, D))
    assert torch.equal(h[:, 3:], tok + pos) and torch.equal(A.vit_assemble(tok.reshape(B * L, D), cls, None, None, B)[:, 1:], tok)


# ---- hand-written backward ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm_pix", [False, True])
def test_loss_gradient_formula_is_autograd(norm_pix):
    x, pred, mask, K = A.mse_inputs(4, 3, 8, 3, F32, F32)
    pred = torch.nan_to_num(pred.double(), nan=0.25).requires_grad_(True)  # the class rows take part in autograd: their gradient is zero
    loss, _, dpred = A.masked_mse(pred, x.double(), mask, 4, norm_pix, scale=3.0)
    (3.0 * loss).backward()
    assert torch.allclose(dpred.detach(), pred.grad, rtol=1e-13, atol=1e-18) and bool((pred.grad[:, 0] == 0).all())


# ---- the restatements' own fp32 error ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm_pix", [False, True])
@pytest.mark.parametrize("P,C,S,B", A.MSE_CASES)
def test_fp32_loss_restatement_holds_a_tenth_of_the_bars(P, C, S, B, norm_pix):
    """The same expressions in fp32 against float64, on the GPU test's inputs: loss, row loss and gradient within 1e-6 (a tenth of the
    fp32 bar), the two degenerate norm_pix rows within 1e-4."""
    L = (S // P) ** 3
    for xdt in (F32, F16):
        for pdt in (F32, BF16):
            x, pred, mask, K = A.mse_inputs(P, C, S, B, xdt, pdt)
            deg = A.degenerate_rows(B, L) if norm_pix else torch.zeros(B, L, dtype=torch.bool)
            lo = A.masked_mse(pred.float(), x.float(), mask, P, norm_pix, 3.0)
            hi = A.masked_mse(pred.double(), x.double(), mask, P, norm_pix, 3.0)
            fig = {"loss": (A.rel(lo[0], hi[0]), FP32_BAR), "row_loss": (A.rel(lo[1][~deg], hi[1][~deg]), FP32_BAR),
                   "dpred": (A.rel(lo[2][:, 1:][~deg], hi[2][:, 1:][~deg]), FP32_BAR)}
            if bool(deg.any()):
                fig["row_loss(degenerate)"] = (A.rel(lo[1][deg], hi[1][deg]), DEGENERATE_BAR)
                fig["dpred(degenerate)"] = (A.rel(lo[2][:, 1:][deg], hi[2][:, 1:][deg]), DEGENERATE_BAR)
            print(P, C, S, B, norm_pix, xdt, pdt, {k: f"{v[0]:.2e}" for k, v in fig.items()})
            for k, (value, bar) in fig.items():
                assert value <= bar / 10, (k, value, bar)


def test_fp32_sums_hold_the_summation_bound():
    """The reductions have no bar but a bound, (n - 1) 2^-24 sum|terms| per element, valid for every order: autograd's own fp32
    summation of the same terms must hold it against the float64 sums, and the float64 sums themselves are 2^-29 of it away from exact."""
    for D, B in ((48, 33), (260, 17)):
        for K in A.KS:
            inp = A.encoder_inputs(D, B, K, "normal")
            hi, cnt, mag = A.encoder_bwd(inp, B, K)
            lo, _, _ = A.encoder_bwd(inp, B, K, dtype=F32)
            for k in ("dcls", "dpos"):
                assert bool(((lo[k].double() - hi[k]).abs() <= A.sum_bound(cnt[k], mag[k])).all()), (k, D, B, K)
            inp = A.decoder_inputs(D, B, K, "normal")
            hi, cnt, mag = A.decoder_bwd(inp, B, K)
            lo, _, _ = A.decoder_bwd(inp, B, K, dtype=F32)
            for k in ("dmask_token", "ddec_cls"):
                assert bool(((lo[k].double() - hi[k]).abs() <= A.sum_bound(cnt[k], mag[k])).all()), (k, D, B, K)
    assert float(A.sum_bound(torch.tensor([1.0, 0.0]), torch.tensor([5.0, 0.0])).max()) == 0.0  # one term: nothing is rounded


# ---- the GPU test's inputs ------------------------------------------------------------------------------------------------------------
def _is_small_integer(t):
    return bool((t == t.round()).all()) and float(t.abs().max()) <= 4 and torch.equal(t.to(BF16).float(), t)


def _exact(mag):
    """Every partial sum, in any order, is an integer below 2^24 in magnitude: exactly representable in fp32."""
    return all(float(m.max()) < 2 ** 24 for m in mag.values() if m is not None)


def test_geometry_and_loop_limits():
    assert A.L_ASM == (A.S_ASM // A.P_ASM) ** 3 == 64
    masked = [A.L_ASM - K for K in A.KS]
    assert masked[0] % 8 == 0 and masked[1] % 8 != 0 and min(masked) > 8            # decoder reduce: whole trips / ragged tail
    lanes = [D // 4 for D in A.DS]
    assert all(D % 4 == 0 for D in A.DS) and lanes[0] <= 64 and 64 < lanes[1] < 256 and 256 < lanes[2] < 512  # 64 / 128 / 256 threads + a second trip
    enc_b, dec_b, vit_b = {b for _, b in A.ENC_CASES}, {b for _, b in A.DEC_CASES}, {b for _, b in A.VIT_CASES}
    assert 1 in enc_b and any(8 < b <= 16 for b in enc_b) and any(16 < b <= 32 for b in enc_b) and any(b > 32 for b in enc_b)
    assert any(16 < b <= 32 for b in vit_b) and any(b > 32 for b in vit_b)           # strided_rowsum: 16 volumes per trip
    assert any(b == A.K_ASM_BLOCKS + 1 for b in dec_b) and any(b > A.K_ASM_BLOCKS + 1 for b in dec_b)  # reduce blocks take a second volume
    assert any(128 < min(b, A.K_ASM_BLOCKS) for b in dec_b) and any(1 < b < 128 for b in dec_b)  # fold_partials: 128 partial rows per trip
    assert all(D == 48 for D, b in A.DEC_CASES if b > 33)
    pds = {P ** 3 * C for P, C, _, _ in A.MSE_CASES}
    assert min(pds) < 256 and any(256 < pd < 1024 for pd in pds) and any(pd > 1024 for pd in pds)
    assert sum(B * (S // P) ** 3 > 2048 for P, C, S, B in A.MSE_CASES) == 1          # loss_fold: 2048 rows per trip
    assert {(P, C) for P, C, S, B in A.MSE_CASES if S == 2 * P} == {(4, 1), (8, 1), (12, 1), (4, 3), (12, 3)}


@pytest.mark.parametrize("D,B", A.ENC_CASES)
def test_encoder_inputs(D, B):
    for K in A.KS:
        inp = A.encoder_inputs(D, B, K, "int")
        assert all(_is_small_integer(inp[k]) for k in ("cls", "pos", "tok", "dh0"))
        ref, cnt, mag = A.encoder_bwd(inp, B, K)
        assert _exact(mag) and bool((ref["dpos"] == ref["dpos"].round()).all())
        idr = inp["ids_restore"]
        assert torch.equal(torch.sort(idr, dim=1).values, torch.arange(A.L_ASM).expand(B, -1))
        assert B == 1 or not torch.equal(idr[0], idr[1])
        assert torch.equal(cnt["dpos"][:, 0].long(), (idr < K).sum(0)) and int(cnt["dcls"][0]) == B
        # dpos, 8 volumes per trip: every later trip holds a volume that keeps some position, so that its terms are in the sum
        for first in range(8, B, 8):
            assert bool((idr[first:first + 8] < K).any())
        assert not bool((inp["dh0"][:, 0] == 0).all(dim=0).any()) or B < 3  # a dropped class row would show in some column


@pytest.mark.parametrize("D,B", A.DEC_CASES)
def test_decoder_inputs(D, B):
    for K in A.KS:
        inp = A.decoder_inputs(D, B, K, "int")
        assert all(_is_small_integer(inp[k]) for k in ("mask_token", "dec_cls", "dec_pos", "e", "dy"))
        ref, cnt, mag = A.decoder_bwd(inp, B, K)
        assert _exact(mag) and float(mag["dmask_token"].max()) > 0
        assert int(cnt["dmask_token"][0]) == B * (A.L_ASM - K) and int(cnt["ddec_cls"][0]) == B
        ids_restore, ids_shuffle = inp["ids_restore"], inp["ids_shuffle"]
        assert torch.equal(torch.gather(ids_restore, 1, ids_shuffle), torch.arange(A.L_ASM).expand(B, -1))
        # the last volume's last masked row carries a non-zero term: dropping the tail of the 8-row trip or the strided volumes changes the sum
        last = inp["dy"][B - 1, 1 + int(ids_shuffle[B - 1, -1])]
        assert bool((last != 0).any())


@pytest.mark.parametrize("D,B", A.VIT_CASES)
def test_vit_inputs(D, B):
    for R in (0, 2):
        inp = A.vit_inputs(D, B, R, "int")
        assert all(_is_small_integer(inp[k]) for k in ("cls", "pos", "tok", "dh") if inp[k] is not None) and (inp["reg"] is None) == (R == 0)
        ref, cnt, mag = A.vit_bwd(inp, B, R)
        assert _exact(mag) and all(int(cnt[k].min()) == int(cnt[k].max()) == B for k in ("dcls", "dpos"))
        assert bool((inp["dh"][B - 1] != 0).any())


@pytest.mark.parametrize("P,C,S,B", A.MSE_CASES)
def test_mse_inputs(P, C, S, B):
    L, pd = (S // P) ** 3, P ** 3 * C
    for xdt in (F32, F16):
        x, pred, mask, K = A.mse_inputs(P, C, S, B, xdt, BF16)
        assert x.dtype == xdt and pred.dtype == BF16 and K == int(L * 0.25) and int(mask.sum()) == B * (L - K)
        rows = A.patchify(x.double(), P)
        assert bool((rows[0, 0] == 0).all()) and int((rows[0, 1] != 0).sum()) == 1 and float(rows[0, 1].max()) == 0.625
        assert mask[0, 0] == 1 and mask[0, 1] == 1 and bool(A.degenerate_rows(B, L)[0, :2].all()) and int(A.degenerate_rows(B, L).sum()) == 2
        assert bool(torch.isnan(pred[:, 0].float()).all()) and bool(torch.isfinite(pred[:, 1:].float()).all())
        # 1 / sqrt(var + 1e-6): 1000 on the all-zero patch, large on the single-voxel patch
        var = rows.var(dim=-1)
        assert float(var[0, 0]) == 0.0 and float(var[0, 1]) < float(var[1:].min())


def test_rank_noise_has_the_ties():
    for L in (64, 1000, 4096):
        n = A.rank_noise(3, L, 1)
        assert n[0, 0] == n[0, 1] == n[0].min() and n[0, L - 1] == n[0, L - 2] == n[0].max()
        assert n[1, 0] == n[1, L - 1] == n[1].min() and bool((n[2] == n[2, 0]).all())
        assert len(set(n[0, 2:L - 2].tolist())) == L - 4
