"""The MAE data-path kernels of csrc/elementwise.hip through the C ABI, one by one, against the plain restatements of
tests/assembly_ref.py evaluated in float64: hct_mask_rank, hct_patch_gather with a shuffle table, the encoder / decoder / ViT
input assemblies with their backwards, hct_masked_mse and hct_unpatchify.

Every output is pre-filled with NaN (integers: a sentinel) inside a buffer with a guard band of at least one row on each side that
must come back untouched, and every call is made twice: the two results must agree bit for bit (the header promises fixed
summation orders).  Copies and single additions are held bit-equal.  Reductions are held (a) bit-equal on integer-valued inputs,
whose sums are exact in fp32 in any order -- the case that catches a dropped or a doubled term -- and (b) on normal inputs to the
recursive-summation bound |got - ref| <= (n - 1) 2^-24 sum|terms| per element, computed from the test's own inputs; nothing is
measured.  The loss is held to the project's fp32 bar (rel. L2 < 1e-5), bf16 gradients to 4e-3, the two degenerate norm_pix
patches to 1e-3.  The batch sizes and widths are the ones at which each kernel's loop is taken a second time or ends raggedly;
the comment beside each case names the loop."""
import math

import pytest
import torch

from headct_foundation_amd import _lib
from headct_foundation_amd._lib import HCT_BF16, HCT_F16, HCT_F32
from tests import assembly_ref as A

pytestmark = pytest.mark.gpu

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
FP32_BAR = 1e-5      # test_layernorm_fwd_bwd's bar for fp32 arithmetic on identical inputs
BF16_BAR = 4e-3      # ... and for values stored as bf16
DEGENERATE_BAR = 1e-3  # tests/test_reconstruct_gpu.py FP32_BAR: rows whose target is scaled by 1 / sqrt(var + 1e-6) up to 1000
L, S, P = A.L_ASM, A.S_ASM, A.P_ASM


def _st():
    return torch.cuda.current_stream().cuda_stream


def _code(dtype):
    return {F32: HCT_F32, BF16: HCT_BF16, F16: HCT_F16}[dtype]


def _p(t):
    return None if t is None else (t.ptr if isinstance(t, _Out) else t.data_ptr())


def _bits(t):
    return t.view({4: torch.int32, 2: torch.int16}[t.element_size()])


class _Out:
    """An output tensor inside a larger buffer: body NaN (integers: -7), a guard band of >= one row (a multiple of 64 elements, so
    the body keeps the buffer's alignment) on each side."""

    def __init__(self, shape, dtype, dev):
        n = math.prod(shape)
        self.guard = -(-max(shape[-1], 1) // 64) * 64
        floating = dtype.is_floating_point
        buf = torch.full((n + 2 * self.guard,), float("nan") if floating else -7, dtype=dtype, device=dev)
        buf[:self.guard] = 7777.0 if floating else -9
        buf[self.guard + n:] = 7777.0 if floating else -9
        self.buf, self.n = buf, n
        self.before = (buf[:self.guard].clone(), buf[self.guard + n:].clone())
        self.t = buf[self.guard:self.guard + n].view(shape)
        self.ptr = self.t.data_ptr()

    def untouched(self):
        body = self.t.flatten()
        return bool(torch.isnan(body).all()) if body.dtype.is_floating_point else bool((body == -7).all())

    def result(self):
        assert torch.equal(_bits(self.buf[:self.guard]), _bits(self.before[0])), "guard band below the output was written"
        assert torch.equal(_bits(self.buf[self.guard + self.n:]), _bits(self.before[1])), "guard band above the output was written"
        return self.t.cpu()


def _twice(run):
    """run() allocates its outputs, enqueues the call(s) and returns {name: _Out}.  Two runs: guards intact, bit-identical."""
    a, b = run(), run()
    torch.cuda.synchronize()
    res = {}
    for k in a:
        x, y = a[k].result(), b[k].result()
        assert torch.equal(_bits(x), _bits(y)), f"{k}: a second identical call differs"
        res[k] = x
    return res


def _check_sum(got, ref, n_terms, abs_sum, kind, what):
    """A reduction: exact on integer inputs; otherwise every element within (n - 1) 2^-24 sum|terms| of the float64 sum."""
    assert got.dtype == F32 and not bool(torch.isnan(got).any()), what
    ref = ref.reshape(got.shape)
    if kind == "int":
        assert torch.equal(got.double(), ref), (what, "integer-valued sum is not exact", float((got.double() - ref).abs().max()))
        return
    err, bound = (got.double() - ref).abs(), A.sum_bound(n_terms, abs_sum).reshape(got.shape)
    over = float((err - bound).max())  # 0 where a single term leaves nothing to round
    print(f"{what}: max err {float(err.max()):.3e}, max bound {float(bound.max()):.3e}, max (err - bound) {over:.3e}, n <= {int(n_terms.max())}")
    assert over <= 0.0, (what, over)


# ---- a. hct_mask_rank ------------------------------------------------------------------------------------------------------------
def _rank_call(lib, noise_d, B, Lr, K, dev):
    outs = dict(ids_restore=_Out((B, Lr), torch.int32, dev), ids_shuffle=_Out((B, Lr), torch.int32, dev), mask=_Out((B, Lr), F32, dev))
    rc = lib.hct_mask_rank(noise_d.data_ptr(), B, Lr, K, _p(outs["ids_restore"]), _p(outs["ids_shuffle"]), _p(outs["mask"]), _st())
    return rc, outs


@pytest.mark.parametrize("Lr,K", [(1000, 250), (4096, 1024),  # the 10^3 grid; 16 passes of the 256 threads over a row
                                  (64, 1), (64, 63), (1000, 1), (1000, 999)])  # a single kept / a single masked patch
def test_mask_rank(lib, cuda, Lr, K):
    """ids_restore, ids_shuffle and mask equal the stable argsort: ties at the start and at the end of a row and an all-tie row."""
    B = 3
    noise = A.rank_noise(B, Lr, K)
    nd = noise.to(cuda)

    def run():
        rc, outs = _rank_call(lib, nd, B, Lr, K, cuda)
        _lib.check(rc, "hct_mask_rank")
        return outs
    got = _twice(run)
    ids_restore, ids_shuffle, mask = A.mask_rank(noise, K)
    assert torch.equal(got["ids_restore"].long(), ids_restore) and torch.equal(got["ids_shuffle"].long(), ids_shuffle)
    assert torch.equal(got["mask"], mask) and int(mask.sum()) == B * (Lr - K)
    assert torch.equal(ids_shuffle[B - 1], torch.arange(Lr)) and ids_shuffle[0, :2].tolist() == [0, 1] and ids_shuffle[1, :2].tolist() == [0, Lr - 1]


@pytest.mark.parametrize("Lr,K", [(12289, 100), (64, 65)])
def test_mask_rank_refuses_before_launching(lib, cuda, Lr, K):
    """A row that does not fit the kernel's LDS image (L > 12288) and K > L return non-zero; nothing is written."""
    nd = torch.rand(1, Lr).to(cuda)
    rc, outs = _rank_call(lib, nd, 1, Lr, K, cuda)
    torch.cuda.synchronize()
    assert rc != 0 and "hct_mask_rank" in lib.hct_last_error_string().decode()
    for o in outs.values():
        o.result()
        assert o.untouched()


# ---- b. hct_patch_gather -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rdt", [BF16, F32])
@pytest.mark.parametrize("xdt", [F16, F32])
@pytest.mark.parametrize("C,Pp,Sp", [(1, 4, 16),    # 16 quads per row: 240 of the 256 threads idle
                                     (3, 12, 48),   # 1296 quads: 5.06 passes, three channels
                                     (1, 16, 64)])  # 1024 quads: exactly four passes
def test_patch_gather_with_shuffle_table(lib, cuda, C, Pp, Sp, xdt, rdt):
    """Kept patches only (K = 13 < L = 64), a different permutation per volume: bit-equal to the gathered Conv3d-order rows."""
    B, K = 3, 13
    Lp = (Sp // Pp) ** 3
    assert Lp == 64
    x = torch.randn(B, C, Sp, Sp, Sp, generator=A.gen(C, Pp, Sp)).to(xdt)
    _, _, ids_shuffle, _ = A.permutations(B, Lp, K, 11)
    assert not torch.equal(ids_shuffle[0], ids_shuffle[1]) and not torch.equal(ids_shuffle[1], ids_shuffle[2])
    xd, idd = x.to(cuda), ids_shuffle.to(torch.int32).to(cuda)

    def run():
        rows = _Out((B * K, C * Pp ** 3), rdt, cuda)
        _lib.check(lib.hct_patch_gather(xd.data_ptr(), _code(xdt), idd.data_ptr(), B, C, Sp, Pp, Lp, K, rows.ptr, _code(rdt), _st()), "hct_patch_gather")
        return dict(rows=rows)
    got = _twice(run)["rows"]
    assert torch.equal(_bits(got), _bits(A.patch_gather(x.float(), ids_shuffle, Pp, K).to(rdt)))


def test_patch_gather_all_patches_beyond_the_pencil(lib, cuda):
    """No table, fp32 rows of (B, C, S, P) = (1, 1, 128, 16): the pencil's LDS image would be 16 * 16 * 128 * 4 B = 128 KiB > 64 KiB, so
    the per-patch kernel runs with a NULL table (the bf16 case of test_patch_gather_all_patches fits exactly and takes the pencil)."""
    B, C, Sp, Pp = 1, 1, 128, 16
    Lp = (Sp // Pp) ** 3
    x = torch.randn(B, C, Sp, Sp, Sp, generator=A.gen(128, 16))
    xd = x.to(cuda)

    def run():
        rows = _Out((B * Lp, C * Pp ** 3), F32, cuda)
        _lib.check(lib.hct_patch_gather(xd.data_ptr(), HCT_F32, None, B, C, Sp, Pp, Lp, Lp, rows.ptr, HCT_F32, _st()), "hct_patch_gather")
        return dict(rows=rows)
    assert torch.equal(_twice(run)["rows"], A.patch_gather(x, None, Pp, Lp))


# ---- c. hct_encoder_assemble_fwd / bwd --------------------------------------------------------------------------------------------
# row copies: D/4 = 12 lanes on 64 threads, 65 on 128 threads, 257 on 256 threads with a second trip of one lane
# dpos (encoder_assemble_bwd_pos_kernel), 8 volumes per trip: B = 9 takes it twice, 17 three times with one volume in the last
# dcls (strided_rowsum_kernel), 16 volumes per trip: B = 17 takes it twice, 33 three times
@pytest.mark.parametrize("D,B", A.ENC_CASES)
def test_encoder_assemble(lib, cuda, D, B):
    ws = torch.empty(lib.hct_assemble_bwd_workspace_bytes(D), dtype=torch.uint8, device=cuda)
    for K in A.KS:
        for kind in ("int", "normal"):
            inp = A.encoder_inputs(D, B, K, kind)
            ids_shuffle, cls, pos, dh0 = inp["ids_shuffle"], inp["cls"], inp["pos"], inp["dh0"]
            idr_d, ids_d = inp["ids_restore"].to(torch.int32).to(cuda), ids_shuffle.to(torch.int32).to(cuda)
            cls_d, pos_d, dh0_d = cls.to(cuda), pos.to(cuda), dh0.to(cuda)
            ref, cnt, mag = A.encoder_bwd(inp, B, K)
            assert int(cnt["dcls"].max()) == B and int(cnt["dpos"].sum()) == B * K * D
            for tdt in (BF16, F32):
                tok = inp["tok"].to(tdt)
                tok_d = tok.to(cuda)
                for use_pos in (True, False):
                    def fwd():
                        h0 = _Out((B, K + 1, D), F32, cuda)
                        _lib.check(lib.hct_encoder_assemble_fwd(tok_d.data_ptr(), _code(tdt), cls_d.data_ptr(), pos_d.data_ptr() if use_pos else None,
                                                                ids_d.data_ptr(), B, L, K, D, h0.ptr, _st()), "hct_encoder_assemble_fwd")
                        return dict(h0=h0)
                    want = A.encoder_assemble(tok.double(), cls.double(), pos.double() if use_pos else None, ids_shuffle, B, K)
                    # one fp32 addition per element: rounding the float64 sum of two fp32 values to fp32 is that addition's result
                    assert torch.equal(_bits(_twice(fwd)["h0"]), _bits(want.float())), (K, kind, tdt, use_pos)

                def bwd(skip=None):
                    outs = dict(dtok=_Out((B * K, D), tdt, cuda), dcls=_Out((D,), F32, cuda), dpos=_Out((L, D), F32, cuda))
                    if skip:
                        del outs[skip]
                    _lib.check(lib.hct_encoder_assemble_bwd(dh0_d.data_ptr(), idr_d.data_ptr(), B, L, K, D, _p(outs.get("dtok")), _code(tdt),
                                                            _p(outs.get("dcls")), _p(outs.get("dpos")), ws.data_ptr(), ws.numel(), _st()),
                               "hct_encoder_assemble_bwd")
                    return outs
                got = _twice(bwd)
                assert torch.equal(_bits(got["dtok"]), _bits(ref["dtok"].float().to(tdt))), (K, kind, tdt)  # copies
                for k in ("dcls", "dpos"):
                    _check_sum(got[k], ref[k], cnt[k], mag[k], kind, f"encoder {k} D={D} B={B} K={K} {kind}")
                for skip in ("dtok", "dcls", "dpos"):  # each output NULL in turn: the others are what they were
                    part = _twice(lambda: bwd(skip))
                    assert set(part) == set(got) - {skip}
                    for k in part:
                        assert torch.equal(_bits(part[k]), _bits(got[k])), (skip, k)


# ---- d. hct_decoder_assemble_fwd / bwd --------------------------------------------------------------------------------------------
# decoder_assemble_bwd_reduce_kernel: one block per volume up to kAsmBlocks = 256, then strided: B = 257 gives block 0 a second
#   volume, 261 blocks 0 .. 4; masked rows 8 per trip: K = 16 -> 48 rows = six whole trips, K = 13 -> 51 rows = six trips + a tail of 3
# fold_partials_kernel: 16 row groups x 8 loads = 128 partial rows per trip: nblk = 256 (B >= 256) takes it twice; nblk = 1, 9, 33 end
#   inside the first trip with idle row groups
# ddec_cls is the same fold over the blocks' class rows
@pytest.mark.parametrize("D,B", A.DEC_CASES)
def test_decoder_assemble(lib, cuda, D, B):
    nws = lib.hct_assemble_bwd_workspace_bytes(D)
    assert nws == A.K_ASM_BLOCKS * 2 * D * 4
    ws = torch.empty(nws, dtype=torch.uint8, device=cuda)
    for K in A.KS:
        for kind in ("int", "normal"):
            inp = A.decoder_inputs(D, B, K, kind)
            ids_restore, mtok, dcls, dpos, dy = inp["ids_restore"], inp["mask_token"], inp["dec_cls"], inp["dec_pos"], inp["dy"]
            idr_d, ids_d = ids_restore.to(torch.int32).to(cuda), inp["ids_shuffle"].to(torch.int32).to(cuda)
            mtok_d, dcls_d, dpos_d, dy_d = mtok.to(cuda), dcls.to(cuda), dpos.to(cuda), dy.to(cuda)
            ref, cnt, mag = A.decoder_bwd(inp, B, K)
            assert int(cnt["dmask_token"].min()) == B * (L - K) and int(cnt["ddec_cls"].min()) == B
            for edt in (BF16, F32):
                e = inp["e"].to(edt)
                e_d = e.to(cuda)

                def fwd():
                    y = _Out((B, L + 1, D), F32, cuda)
                    _lib.check(lib.hct_decoder_assemble_fwd(e_d.data_ptr(), _code(edt), mtok_d.data_ptr(), dcls_d.data_ptr(), dpos_d.data_ptr(),
                                                            idr_d.data_ptr(), B, L, K, D, y.ptr, _st()), "hct_decoder_assemble_fwd")
                    return dict(y=y)
                want = A.decoder_assemble(e.double(), mtok.double(), dcls.double(), dpos.double(), ids_restore, K)
                assert torch.equal(_bits(_twice(fwd)["y"]), _bits(want.float())), (K, kind, edt)  # one fp32 addition per element

                def bwd(short=0):
                    outs = dict(de=_Out((B, K + 1, D), edt, cuda), dmask_token=_Out((D,), F32, cuda), ddec_cls=_Out((D,), F32, cuda))
                    rc = lib.hct_decoder_assemble_bwd(dy_d.data_ptr(), idr_d.data_ptr(), ids_d.data_ptr(), B, L, K, D, outs["de"].ptr, _code(edt),
                                                      outs["dmask_token"].ptr, outs["ddec_cls"].ptr, ws.data_ptr(), nws - short, _st())
                    return rc, outs

                def run():
                    rc, outs = bwd()
                    _lib.check(rc, "hct_decoder_assemble_bwd")
                    return outs
                got = _twice(run)
                assert torch.equal(_bits(got["de"]), _bits(ref["de"].float().to(edt))), (K, kind, edt)  # a gather: copies
                for k in ("dmask_token", "ddec_cls"):
                    _check_sum(got[k], ref[k], cnt[k], mag[k], kind, f"decoder {k} D={D} B={B} K={K} {kind}")
            rc, outs = bwd(short=1)  # a workspace one byte short is refused before anything is launched
            torch.cuda.synchronize()
            assert rc != 0 and all(o.untouched() for o in outs.values())
            for o in outs.values():
                o.result()


# ---- e. hct_vit_assemble_fwd / bwd ------------------------------------------------------------------------------------------------
# strided_rowsum_kernel (dcls, dreg, dpos), 16 volumes per trip: B = 17 takes it twice (one volume in the second), 33 three times
# dreg / dpos run it over R * D and L * D columns: more than one block of 256 columns, the last one ragged (27 * 48 = 5 * 256 + 16)
@pytest.mark.parametrize("D,B", A.VIT_CASES)
def test_vit_assemble(lib, cuda, D, B):
    Lv = A.VIT_L
    for R in (0, 2):
        for kind in ("int", "normal"):
            inp = A.vit_inputs(D, B, R, kind)
            cls, pos, reg, dh = inp["cls"], inp["pos"], inp["reg"], inp["dh"]
            cls_d, pos_d, reg_d, dh_d = cls.to(cuda), pos.to(cuda), reg.to(cuda) if R else None, dh.to(cuda)
            ref, cnt, mag = A.vit_bwd(inp, B, R)
            for tdt in (BF16, F32):
                tok = inp["tok"].to(tdt)
                tok_d = tok.to(cuda)
                for use_pos in (True, False):
                    def fwd():
                        h = _Out((B, 1 + R + Lv, D), F32, cuda)
                        _lib.check(lib.hct_vit_assemble_fwd(tok_d.data_ptr(), _code(tdt), cls_d.data_ptr(), _p(reg_d), pos_d.data_ptr() if use_pos else None,
                                                            B, Lv, R, D, h.ptr, _st()), "hct_vit_assemble_fwd")
                        return dict(h=h)
                    want = A.vit_assemble(tok.double(), cls.double(), reg.double() if R else None, pos.double() if use_pos else None, B)
                    assert torch.equal(_bits(_twice(fwd)["h"]), _bits(want.float())), (R, kind, tdt, use_pos)  # one fp32 addition per element

                def bwd():
                    outs = dict(dtok=_Out((B * Lv, D), tdt, cuda), dcls=_Out((D,), F32, cuda), dpos=_Out((Lv, D), F32, cuda))
                    if R:
                        outs["dreg"] = _Out((R, D), F32, cuda)
                    _lib.check(lib.hct_vit_assemble_bwd(dh_d.data_ptr(), B, Lv, R, D, outs["dtok"].ptr, _code(tdt), outs["dcls"].ptr, _p(outs.get("dreg")),
                                                        outs["dpos"].ptr, _st()), "hct_vit_assemble_bwd")
                    return outs
                got = _twice(bwd)
                assert torch.equal(_bits(got["dtok"]), _bits(ref["dtok"].float().to(tdt))), (R, kind, tdt)  # copies
                for k in ("dcls", "dpos") + (("dreg",) if R else ()):
                    assert int(cnt[k].min()) == B
                    _check_sum(got[k], ref[k], cnt[k], mag[k], kind, f"vit {k} D={D} B={B} R={R} {kind}")


# ---- f. hct_masked_mse -----------------------------------------------------------------------------------------------------------
# masked_mse_kernel, C = 1: quads, 1024 elements per trip: P = 4 (pd = 64) leaves 240 threads idle, P = 8 (512) half of them,
#   P = 12 (1728) takes 1.7 trips; C = 3: one element per thread, pd = 192 < 256 and pd = 5184 = 20.25 trips
# loss_fold_kernel, 256 threads x 8 loads = 2048 rows per trip: (8, 1, 32, 33) folds B * L = 2112 rows (the second trip holds 64)
@pytest.mark.parametrize("norm_pix", [False, True])
@pytest.mark.parametrize("Pm,C,Sm,B", A.MSE_CASES)
def test_masked_mse(lib, cuda, Pm, C, Sm, B, norm_pix):
    """Loss, per-row loss and d loss / d pred against float64 on the same rounded inputs: fp32 and fp16 volumes, fp32 and bf16
    predictions, dpred_scale NULL and 3.0, loss NULL with dpred and dpred NULL with loss.  Volume 0 holds an all-zero patch and a
    patch with a single non-zero voxel, both masked.  Class rows of pred are NaN: they are never read."""
    Lm, pd = (Sm // Pm) ** 3, Pm ** 3 * C
    assert (B * Lm > 2048) == (B == 33)
    for xdt in (F32, F16):
        for pdt in (F32, BF16):
            x, pred, mask, K = A.mse_inputs(Pm, C, Sm, B, xdt, pdt)
            msum = float(mask.sum())
            assert msum == B * (Lm - K)
            x_d, pred_d, mask_d = x.to(cuda), pred.to(cuda), mask.to(cuda)
            three = torch.tensor([3.0], device=cuda)
            deg = A.degenerate_rows(B, Lm) if norm_pix else torch.zeros(B, Lm, dtype=torch.bool)
            kept = mask == 0
            for want_loss, want_dpred, scale in ((True, True, None), (True, True, 3.0), (False, True, None), (True, False, None)):
                def run():
                    outs = dict(row_loss=_Out((B, Lm), F32, cuda))
                    if want_loss:
                        outs["loss"] = _Out((1,), F32, cuda)
                    if want_dpred:
                        outs["dpred"] = _Out((B, Lm + 1, pd), pdt, cuda)
                    _lib.check(lib.hct_masked_mse(pred_d.data_ptr(), _code(pdt), x_d.data_ptr(), _code(xdt), mask_d.data_ptr(), B, C, Sm, Pm, int(norm_pix),
                                                  msum, outs["row_loss"].ptr, _p(outs.get("loss")), _p(outs.get("dpred")),
                                                  three.data_ptr() if scale else None, _st()), "hct_masked_mse")
                    if not want_loss:
                        del outs["row_loss"]  # scratch of the loss: the header promises nothing about it when loss is NULL
                    return outs
                got = _twice(run)
                r_loss, r_row, r_dp = A.masked_mse(pred.double(), x.double(), mask, Pm, norm_pix, scale or 1.0)
                tag = f"masked_mse P={Pm} C={C} S={Sm} B={B} norm_pix={norm_pix} x={xdt} pred={pdt} scale={scale} loss={want_loss} dpred={want_dpred}"
                fig = {}
                if want_loss:
                    fig["loss"] = (A.rel(got["loss"][0], r_loss), FP32_BAR)
                    fig["row_loss"] = (A.rel(got["row_loss"][~deg], r_row[~deg]), FP32_BAR)
                    if bool(deg.any()):
                        fig["row_loss(degenerate)"] = (A.rel(got["row_loss"][deg], r_row[deg]), DEGENERATE_BAR)
                    assert bool((got["row_loss"][kept] == 0).all()), tag
                if want_dpred:
                    d = got["dpred"]
                    assert bool((d[:, 0] == 0).all()) and bool((d[:, 1:][kept] == 0).all()), tag  # class row and kept rows: exactly zero
                    assert bool(torch.isfinite(d.float()).all()), tag
                    if pdt == BF16:
                        fig["dpred"] = (A.rel(d[:, 1:], r_dp[:, 1:]), BF16_BAR)
                    else:
                        fig["dpred"] = (A.rel(d[:, 1:][~deg], r_dp[:, 1:][~deg]), FP32_BAR)
                        if bool(deg.any()):
                            fig["dpred(degenerate)"] = (A.rel(d[:, 1:][deg], r_dp[:, 1:][deg]), DEGENERATE_BAR)
                print(tag, {k: f"{v[0]:.2e}" for k, v in fig.items()})
                for k, (value, bar) in fig.items():
                    assert value < bar, (tag, k, value, bar)


# ---- g. hct_unpatchify -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pdt", [BF16, F32])
@pytest.mark.parametrize("has_cls", [0, 1])
@pytest.mark.parametrize("C,Pu", [(1, 4), (3, 4), (1, 12), (3, 12)])  # pd = 64 < 256 threads ... 5184 = 20.25 passes; channel interleave
def test_unpatchify(lib, cuda, C, Pu, has_cls, pdt):
    """Prediction rows -> voxels, bit-equal to the permuted rows; with has_cls_row the class rows are NaN and never read."""
    B, Su = 3, 2 * Pu
    Lu, pd = 8, Pu ** 3 * C
    rows = torch.randn(B, Lu, pd, generator=A.gen(C, Pu, has_cls)).to(pdt)
    full = torch.cat((torch.full((B, 1, pd), float("nan"), dtype=pdt), rows), dim=1) if has_cls else rows
    full_d = full.contiguous().to(cuda)

    def run():
        vol = _Out((B, C, Su, Su, Su), F32, cuda)
        _lib.check(lib.hct_unpatchify(full_d.data_ptr(), _code(pdt), has_cls, B, C, Su, Pu, vol.ptr, _st()), "hct_unpatchify")
        return dict(vol=vol)
    assert torch.equal(_bits(_twice(run)["vol"]), _bits(A.unpatchify(rows.float(), C, Su, Pu)))
