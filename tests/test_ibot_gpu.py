"""GPU: the iBOT masked patch-token loss on the HIP path against tests/ibot_ref.py -- the two masked assembly kernels through the C ABI
(bit-equal forward, exact integer sums, product_sum_bound on Gaussian sums, guarded NaN-filled outputs, both levels of the dmask_token
reduction), hct_ibot_loss / hct_ibot_loss_sk at the bars tests/head_kernels_ref.py holds hct_dino_loss to, the backbone with masks
against the restatement (the tolerances tests/test_patch_dropout_gpu.py uses for its own), the wrapper's gather / pad / split, the
IBOTPatchLoss module in both centering modes and over two emulated ranks, and main_pretrain_dino.py end to end."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from headct_foundation_amd import _lib
from headct_foundation_amd._lib import HCT_F32
from oracle import mae_oracle as O
from tests import dino_v2_ref as V2
from tests import drop_path_ref as P
from tests import dropout_ref as R
from tests import head_kernels_ref as H
from tests import ibot_ref as IR
from tests import lora_ref
from tests import patch_dropout_ref as PD
from tests.test_assembly_kernels_gpu import _Out, _bits, _code, _st
from tests.util import grads_by_name, rel_err

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
VIT_ARGS = ("in_chans", "img_size", "patch_size", "hidden_size", "mlp_dim", "num_layers", "num_heads", "num_register_tokens", "qkv_bias")
SEED = 0x9E3779B97F4A7C15
TS, TT = 0.1, 0.04


def _p(o):
    return None if o is None else (o.ptr if isinstance(o, _Out) else o.data_ptr())


def _ws(nbytes, dev):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=dev)


# ---- 1. the assembly kernels -----------------------------------------------------------------------------------------------------------------
def _asm_inputs(B, L, Rn, D, tdt, seed):
    g = torch.Generator().manual_seed(seed)
    tok = torch.randn(B * L, D, generator=g).to(tdt)
    cls, reg, pos, mt = torch.randn(D, generator=g), (torch.randn(Rn, D, generator=g) if Rn else None), torch.randn(L, D, generator=g), torch.randn(D, generator=g)
    return tok, cls, reg, pos, mt


def _run_fwd(lib, cuda, B, L, Rn, D, tdt, mask, use_pos, seed):
    tok, cls, reg, pos, mt = _asm_inputs(B, L, Rn, D, tdt, seed)
    dev = [t.to(cuda) if t is not None else None for t in (tok, cls, reg, pos, mt)]
    md = torch.from_numpy(mask).to(cuda)
    outs = []
    for _ in range(2):
        h0 = _Out((B, 1 + Rn + L, D), F32, cuda)
        _lib.check(lib.hct_vit_assemble_masked_fwd(dev[0].data_ptr(), _code(tdt), dev[1].data_ptr(), _p(dev[2]), dev[3].data_ptr() if use_pos else None,
                                                   dev[4].data_ptr(), md.data_ptr(), B, L, Rn, D, h0.ptr, _st()), "hct_vit_assemble_masked_fwd")
        outs.append(h0)
    torch.cuda.synchronize()
    got = outs[0].result()
    assert torch.equal(_bits(got), _bits(outs[1].result()))
    want = IR.assemble_fwd(tok.float().numpy(), cls.numpy(), reg.numpy() if Rn else None, pos.numpy() if use_pos else None, mt.numpy(), mask)
    assert np.array_equal(got.numpy().view(np.int32), want.view(np.int32))


@pytest.mark.parametrize("tdt", [F32, BF16])
@pytest.mark.parametrize("D", IR.ASM_D)
def test_assemble_masked_fwd(lib, cuda, D, tdt):
    B, L = IR.ASM_B, IR.ASM_L
    for Rn in IR.ASM_R:
        for kind in IR.MASK_PATTERNS:
            for use_pos in (True, False):
                _run_fwd(lib, cuda, B, L, Rn, D, tdt, IR.mask_pattern(kind, B, L, Rn + D), use_pos, 100 * Rn + D)


def _run_bwd(lib, cuda, B, L, Rn, D, tdt, mask, values, seed, missings=(None,)):
    g = torch.Generator().manual_seed(seed)
    dh = torch.randint(-8, 9, (B, 1 + Rn + L, D), generator=g).float() if values == "int" else torch.randn(B, 1 + Rn + L, D, generator=g)
    dh_d, md = dh.to(cuda), torch.from_numpy(mask).to(cuda)
    ref = IR.assemble_bwd(dh.numpy(), mask, Rn)
    nws = lib.hct_vit_assemble_masked_bwd_workspace_bytes(B, L, D)
    ws = torch.full((max(nws, 16) // 4 + 64,), float("nan"), device=cuda)  # (NaN: a partial that is read before it is written shows)
    terms = dict(dcls=B, dreg=B, dpos=B, dmask_token=max(ref["n_masked"], 1))
    for missing in missings:
        runs = []
        for _ in range(2):
            o = dict(dtok=_Out((B * L, D), tdt, cuda), dcls=_Out((D,), F32, cuda), dreg=_Out((Rn, D), F32, cuda) if Rn else None,
                     dpos=_Out((L, D), F32, cuda), dmask_token=_Out((D,), F32, cuda))
            if missing:
                o[missing] = None
            _lib.check(lib.hct_vit_assemble_masked_bwd(dh_d.data_ptr(), md.data_ptr(), B, L, Rn, D, _p(o["dtok"]), _code(tdt), _p(o["dcls"]), _p(o["dreg"]),
                                                       _p(o["dpos"]), _p(o["dmask_token"]), ws.data_ptr(), nws, _st()), "hct_vit_assemble_masked_bwd")
            runs.append(o)
        torch.cuda.synchronize()
        got = {k: v.result() for k, v in runs[0].items() if v is not None}
        what = (Rn, values, missing)
        for k, v in got.items():
            assert torch.equal(_bits(v), _bits(runs[1][k].result())), (k, what, "a second identical call differs")
        if "dtok" in got:  # a copy or a zero, and one cast: torch's
            want = torch.where(torch.from_numpy(mask.astype(bool))[:, :, None], torch.zeros(()), dh[:, 1 + Rn:, :]).reshape(B * L, D).to(tdt)
            assert torch.equal(_bits(got["dtok"]), _bits(want)), what
        for k in ("dcls", "dreg", "dpos", "dmask_token"):
            if k not in got:
                continue
            assert not torch.isnan(got[k]).any(), (k, what)
            err = np.abs(got[k].numpy().astype(np.float64) - ref[k])
            if values == "int":
                assert not err.any(), (k, what, "an integer-valued sum is exact in any order")
            else:
                bound = H.product_sum_bound(terms[k], 0, torch.from_numpy(ref["abs"][k])).numpy()
                assert (err <= bound).all(), (k, what, float(err.max()), float(bound.min()))
        if "dmask_token" in got and ref["n_masked"] == 0:
            assert torch.count_nonzero(got["dmask_token"]) == 0 and not torch.signbit(got["dmask_token"]).any(), "no masked entry: an exact zero"


@pytest.mark.parametrize("tdt", [F32, BF16])
@pytest.mark.parametrize("D", IR.ASM_D)
def test_assemble_masked_bwd(lib, cuda, D, tdt):
    B, L = IR.ASM_B, IR.ASM_L
    for Rn in IR.ASM_R:
        for kind in IR.MASK_PATTERNS:
            mask = IR.mask_pattern(kind, B, L, Rn + D)
            _run_bwd(lib, cuda, B, L, Rn, D, tdt, mask, "int", 200 * Rn + D, (None, "dtok", "dcls", "dreg", "dpos", "dmask_token") if kind == "never" else (None,))
            _run_bwd(lib, cuda, B, L, Rn, D, tdt, mask, "gauss", 300 * Rn + D)


@pytest.mark.parametrize("tdt", [F32, BF16])
def test_assemble_masked_crosses_both_reduction_levels(lib, cuda, tdt):
    """1080 patch rows: nine level-1 blocks (the last one ragged, blocks that span two samples), nine partials = a full fold batch and a ragged
    one; D = 1028: a second trip of the column loops."""
    c = IR.ASM_BIG
    B, L, Rn, D = c["B"], c["L"], c["R"], c["D"]
    for kind in ("never", "none", "all"):
        mask = IR.mask_pattern(kind, B, L, 9)
        if kind == "never":
            _run_fwd(lib, cuda, B, L, Rn, D, tdt, mask, True, 77)
        for values in ("int", "gauss"):
            _run_bwd(lib, cuda, B, L, Rn, D, tdt, mask, values, 78)


def test_assemble_masked_refusals(lib, cuda):
    err = lambda: lib.hct_last_error_string().decode()
    t = torch.zeros(256, device=cuda)
    m = torch.zeros(64, dtype=torch.uint8, device=cuda)
    out, dmt = _Out((2, 9, 4), F32, cuda), _Out((4,), F32, cuda)
    for args in ((t.data_ptr(), None, 4, 0), (None, m.data_ptr(), 4, 0), (t.data_ptr(), m.data_ptr(), 6, 0), (t.data_ptr(), m.data_ptr(), 4, 2)):
        mt, mk, D, Rn = args
        rc = lib.hct_vit_assemble_masked_fwd(t.data_ptr(), HCT_F32, t.data_ptr(), None, t.data_ptr(), mt, mk, 2, 8, Rn, D, out.ptr, _st())
        assert rc != 0 and "hct_vit_assemble_masked_fwd" in err(), args
    need = lib.hct_vit_assemble_masked_bwd_workspace_bytes(2, 8, 4)
    assert need == 1 * 4 * 4
    ws = _ws(need, cuda)
    rc = lib.hct_vit_assemble_masked_bwd(t.data_ptr(), m.data_ptr(), 2, 8, 0, 4, None, HCT_F32, None, None, None, dmt.ptr, ws.data_ptr(), need - 1, _st())
    assert rc != 0 and "workspace too small" in err()
    assert lib.hct_vit_assemble_masked_bwd(t.data_ptr(), None, 2, 8, 0, 4, None, HCT_F32, None, None, None, dmt.ptr, ws.data_ptr(), need, _st()) != 0
    torch.cuda.synchronize()
    assert torch.isnan(out.result()).all() and torch.isnan(dmt.result()).all(), "a refused call writes nothing"


# ---- 2. the loss kernels -------------------------------------------------------------------------------------------------------------------
def _loss_call(lib, cuda, inp, dt, form, n_g, sk32=None, dloss=None, want_grad=True, want_csum=True, short=0):
    """One call inside guarded buffers -> (loss, dstudent or None, center_sum or None, rc).  The student rows are the tail of a larger
    buffer (two rows of NaN ahead of them), as the wrapper hands them over."""
    M, K = inp["student"].shape
    big = torch.full((M + 2, K), float("nan"), dtype=dt, device=cuda)
    big[2:] = inp["student"].to(cuda)
    student = big[2:]
    teacher, weight = inp["teacher"].to(cuda), inp["weight"].to(cuda)
    loss, ds = _Out((1,), F32, cuda), (_Out((M, K), dt, cuda) if want_grad else None)
    csum = _Out((K,), F32, cuda) if (want_csum and form == "centering") else None
    dl = torch.tensor([dloss], dtype=F32, device=cuda) if dloss is not None else None
    nws = lib.hct_ibot_loss_workspace_bytes(M, K)
    ws = _ws(nws, cuda)
    if form == "centering":
        center = inp["center"].to(cuda)
        rc = lib.hct_ibot_loss(student.data_ptr(), teacher.data_ptr(), _code(dt), M, K, weight.data_ptr(), center.data_ptr(), TS, TT, 1.0 / n_g, loss.ptr,
                               _p(ds), _lib.ptr(dl), _p(csum), ws.data_ptr(), nws - short, _st())
    else:
        lc, lr, log_n = sk32
        lcd, lrd = lc.to(cuda), lr.to(cuda)
        rc = lib.hct_ibot_loss_sk(student.data_ptr(), teacher.data_ptr(), _code(dt), M, K, weight.data_ptr(), lcd.data_ptr(), lrd.data_ptr(), log_n, TS, TT,
                                  1.0 / n_g, loss.ptr, _p(ds), _lib.ptr(dl), ws.data_ptr(), nws - short, _st())
    torch.cuda.synchronize()
    return loss.result(), (ds.result() if ds is not None else None), (csum.result() if csum is not None else None), rc


@pytest.mark.parametrize("form", ["centering", "sinkhorn_knopp"])
@pytest.mark.parametrize("scale", IR.LOSS_SCALES)
@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("M,K", IR.LOSS_SHAPES)
def test_ibot_loss_vs_restatement(lib, cuda, M, K, dt, scale, form):
    n_g = 4
    inp = IR.loss_inputs(M, K, scale, dt)
    s64, t64, w64 = inp["student"].double(), inp["teacher"].double(), inp["weight"].double()
    sk32 = sk64 = None
    if form == "sinkhorn_knopp":  # the kernel's inputs are fp32 (lc, lr); the reference reads those rounded values
        lc, lr, log_n = IR.sk_logs(inp["teacher"], TT, 3, n_total=M + 5, inv32=True)
        sk32 = (lc.float(), lr.float(), float(np.float32(log_n)))
        sk64 = (sk32[0].double(), sk32[1].double(), sk32[2])
    want, dwant, cwant = IR.ibot_loss(s64, t64, w64, 1.0 / n_g, TS, TT, center=inp["center"].double(), sk=sk64, inv32=True)
    loss, ds, csum, rc = _loss_call(lib, cuda, inp, dt, form, n_g, sk32)
    assert rc == 0, lib.hct_last_error_string()
    e_loss = abs(float(loss) - float(want)) / abs(float(want))
    e_grad = H.worst_row(ds.float(), dwant)
    print(f"ibot loss {form} M{M} K{K} {dt} x{scale}: loss {e_loss:.2e} / {H.DINO_LOSS_BAR:.0e}, worst gradient row {e_grad:.2e} / {H.DINO_GRAD_BAR[dt]:.0e}")
    assert e_loss < H.DINO_LOSS_BAR and e_grad < H.DINO_GRAD_BAR[dt]
    if M > 1:
        z = M // 2
        assert float(inp["weight"][z]) == 0.0 and torch.count_nonzero(ds[z]) == 0, "the row of weight 0 gets an exact-zero gradient"
    if form == "centering":
        bound = H.product_sum_bound(M, 0, t64.abs().sum(0)).numpy()
        err = (csum.double() - cwant).abs().numpy()
        assert (err <= bound).all(), (float(err.max()), float(bound.min()))
    # dloss given: the gradient scales, the loss does not; dstudent / center_sum NULL: the loss is the same bits; a second call is the same bits
    loss2, ds2, _, rc = _loss_call(lib, cuda, inp, dt, form, n_g, sk32, dloss=3.0)
    assert rc == 0 and torch.equal(_bits(loss2), _bits(loss)) and H.worst_row(ds2.float() / 3.0, dwant) < H.DINO_GRAD_BAR[dt]
    loss3, none_ds, none_cs, rc = _loss_call(lib, cuda, inp, dt, form, n_g, sk32, want_grad=False, want_csum=False)
    assert rc == 0 and none_ds is None and none_cs is None and torch.equal(_bits(loss3), _bits(loss))
    loss4, ds4, csum4, rc = _loss_call(lib, cuda, inp, dt, form, n_g, sk32)
    assert rc == 0 and torch.equal(_bits(loss4), _bits(loss)) and torch.equal(_bits(ds4), _bits(ds))
    assert csum is None or torch.equal(_bits(csum4), _bits(csum))


@pytest.mark.parametrize("form", ["centering", "sinkhorn_knopp"])
def test_ibot_loss_refuses_a_short_workspace(lib, cuda, form):
    M, K = 37, 2052
    inp = IR.loss_inputs(M, K, 1.0, F32)
    sk32 = (torch.zeros(K), torch.zeros(M), 0.0)
    loss, ds, csum, rc = _loss_call(lib, cuda, inp, F32, form, 4, sk32, short=1)
    assert rc != 0 and "workspace too small" in lib.hct_last_error_string().decode()
    assert torch.isnan(loss).all() and torch.isnan(ds).all() and (csum is None or torch.isnan(csum).all()), "a refused call leaves the outputs untouched"


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("B,K", [(3, 1028), (5, 2052)])
def test_ibot_loss_is_the_dino_loss_on_two_swapped_crops(lib, cuda, B, K, dt):
    """V = 2 crops: the DINO loss pairs student crop v with teacher crop 1 - v and divides by 2 B.  The iBOT kernel on the same student rows,
    the teacher rows swapped, w = 1 / B and 1 / n_g = 1 / 2 computes the same number, by other blocks and folds."""
    inp = H.dino_inputs(2, B, K, "normal", dt)
    s, t, c = (inp[k].to(cuda) for k in ("student", "teacher", "center"))
    out = _Out((1,), F32, cuda)
    ws = _ws(lib.hct_dino_loss_workspace_bytes(2, B, K), cuda)
    _lib.check(lib.hct_dino_loss(s.data_ptr(), t.data_ptr(), _code(dt), 2, B, K, c.data_ptr(), TS, TT, out.ptr, None, None, None, ws.data_ptr(), ws.numel(),
                                 _st()), "hct_dino_loss")
    swapped = dict(student=inp["student"], teacher=torch.cat((inp["teacher"][B:], inp["teacher"][:B])), weight=torch.full((2 * B,), 1.0 / B), center=inp["center"])
    loss, _, _, rc = _loss_call(lib, cuda, swapped, dt, "centering", 2, want_grad=False, want_csum=False)
    dino = float(out.result())
    print(f"ibot vs dino B{B} K{K} {dt}: {float(loss):.7f} vs {dino:.7f}")
    assert rc == 0 and abs(float(loss) - dino) / abs(dino) < H.DINO_LOSS_BAR


# ---- 3. the backbone ---------------------------------------------------------------------------------------------------------------------------
CASES = {"L8": (IR.TINY_CASE, 8), "L27": (PD.KEEP_CASE_27, 27)}


def _vit(case, dtype, cuda, path=0.0, lora=False, mask_token=True, **kw):
    from headct_foundation_amd.dino_model import ViTBackbone
    m = ViTBackbone(**{k: case[k] for k in VIT_ARGS}, lora=lora, drop_path_rate=path, compute_dtype=dtype, mask_token=mask_token, **kw)
    p = O.make_vit_params({k: tuple(v.shape) for k, v in m.state_dict().items()}, case["seed"])
    for k in p:  # adapters that do something, tokens that matter (a mask token of the embeddings' size)
        if k.endswith("lora_matrix_A"):
            p[k] = p[k] * 50.0
        if k.endswith("lora_matrix_B"):
            p[k] = p[k] * 0.25
        if k in ("cls_token", "register_tokens", "mask_token"):
            p[k] = p[k] * 5.0
    m.load_state_dict(p, strict=True)
    return m.to(cuda), p


def _step(m, x, masks=None, seed=None):
    m.zero_grad()
    if seed is not None:
        m.set_dropout_seed(seed)
    tok = m(x, masks=masks)[0] if masks is not None else m(x)[0]
    lora_ref.case_loss(tok).backward()
    torch.cuda.synchronize()
    return tok.detach().float().cpu(), grads_by_name(m)


_REF = {}


def _ref(key, p, x, mask, case, masks, trainable=None, emulate=False):
    """(tokens, gradients) of the restatement; computed once per key and shared (read only)."""
    if key in _REF:
        return _REF[key]
    old = O._EMU[0]
    O._EMU[0] = emulate
    try:
        pv = {k: v.clone().requires_grad_(trainable is None or trainable(k)) for k, v in p.items()}
        tok = IR.vit_forward_masked(pv, x, mask, case["patch_size"], case["num_heads"], case["num_layers"], masks)
        lora_ref.case_loss(tok).backward()
    finally:
        O._EMU[0] = old
    _REF[key] = tok.detach(), {k: v.grad for k, v in pv.items() if v.grad is not None}
    return _REF[key]


def _compare(got, want, tol, what):
    tok, grads = got
    r_tok, r_grads = want
    assert tok.shape == r_tok.shape
    assert rel_err(tok, r_tok) <= tol, (what, rel_err(tok, r_tok))
    assert set(grads) == set(r_grads), set(grads) ^ set(r_grads)
    worst = max((rel_err(grads[k], r_grads[k]), k) for k in grads)
    print(what, "tokens", rel_err(tok, r_tok), "worst gradient", worst, "mask_token", rel_err(grads["mask_token"], r_grads["mask_token"]) if "mask_token" in grads else None)
    assert worst[0] <= tol, (what, worst)


def _same(a, b):
    return torch.equal(a[0], b[0]) and a[1].keys() == b[1].keys() and all(torch.equal(a[1][k], b[1][k]) for k in a[1])


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_all_false_masks_are_the_plain_forward(lib, cuda, dtype):
    case, L = CASES["L8"]
    B = case["batch"]
    m, p = _vit(case, dtype, cuda)
    plain, _ = _vit(case, dtype, cuda, mask_token=False)
    plain.load_state_dict({k: v for k, v in p.items() if k != "mask_token"}, strict=True)
    x = R.vit_case_input(case).to(cuda)
    base = _step(plain.train(), x)
    nothing = _step(m.train(), x, torch.zeros(B, L, dtype=torch.bool, device=cuda))
    unmasked = _step(m.train(), x)
    for got in (nothing, unmasked):
        assert torch.equal(got[0], base[0]), "bit for bit the plain forward"
        assert torch.count_nonzero(got[1]["mask_token"]) == 0, "a zero mask_token gradient"
        assert all(torch.equal(got[1][k], base[1][k]) for k in base[1]) and set(got[1]) == set(base[1]) | {"mask_token"}
    assert _same(nothing, _step(m.train(), x, torch.zeros(B, L, dtype=torch.uint8, device=cuda))), "uint8 masks are bool masks"
    assert list(m._plans) == [(B, L)], "the masked entry and the unmasked one share the plan of one batch size"
    with torch.no_grad():  # honoured whenever given: evaluation too
        some = IR.case_mask(case, L).to(cuda)
        assert not torch.equal(m.eval()(x, masks=some)[0], m.eval()(x)[0])
        assert torch.equal(m.eval()(x, masks=torch.zeros_like(some))[0], m.eval()(x)[0])


@pytest.mark.parametrize("dtype,tol", [("fp32", 1e-3), ("bf16", 5e-2)])
@pytest.mark.parametrize("name", ["L8", "L27"])
def test_backbone_with_masks_vs_restatement(lib, cuda, name, dtype, tol):
    case, L = CASES[name]
    m, p = _vit(case, dtype, cuda)
    x, mask = R.vit_case_input(case), IR.case_mask(case, L)
    got = _step(m.train(), x.to(cuda), mask.to(cuda))
    emu = dtype == "bf16"
    want = _ref((name, emu), p, x, mask, case, R.Ones(), emulate=emu)
    other, _ = _ref((name, "unmasked"), p, x, None, case, R.Ones())
    assert rel_err(want[0], other) > 1e-2, "the masks change the tokens: the comparison tells whether they were applied"
    assert float(want[1]["mask_token"].abs().max()) > 0
    _compare(got, want, tol, (name, dtype))
    assert _same(got, _step(m, x.to(cuda), mask.to(cuda))), "two runs agree bit for bit"
    assert _same(got, _step(m, [x[:1].to(cuda), x[1:2].to(cuda), x[2:].to(cuda)], mask.to(cuda))), "a list of parts is their concatenation"


@pytest.mark.parametrize("dtype,tol", [("fp32", 1e-3), ("bf16", 5e-2)])
def test_backbone_with_masks_drop_path_and_lora(lib, cuda, dtype, tol):
    """Drop path 0.5 (two blocks: q = [0, 0.5]) and the LoRA adapters on, seed pinned: neither touches the assembly.  Under the LoRA rule
    the mask token is frozen like the class token, and the plan skips its gradient."""
    from headct_foundation_amd.misc import set_requires_grad_false
    name = "L27"
    case, L = CASES[name]
    B = case["batch"]
    m, p = _vit(case, dtype, cuda, path=0.5, lora=True)
    x, mask = R.vit_case_input(case), IR.case_mask(case, L)
    emu = dtype == "bf16"
    # every parameter trains: drop path alone
    got = _step(m.train(), x.to(cuda), mask.to(cuda), SEED)
    want = _ref((name, "path", emu), p, x, mask, case, P.PathMasks(SEED, 0.0, 0.5, case["num_layers"], B), emulate=emu)
    _compare(got, want, tol, (name, dtype, "drop path + lora, all trainable"))
    set_requires_grad_false(m, lora=True)
    got = _step(m.train(), x.to(cuda), mask.to(cuda), SEED)
    want = _ref((name, "path-lora", emu), p, x, mask, case, P.PathMasks(SEED, 0.0, 0.5, case["num_layers"], B), trainable=lora_ref.trainable, emulate=emu)
    assert "mask_token" not in got[1] and sum("lora" in k for k in got[1]) == 4 * case["num_layers"]
    _compare(got, want, tol, (name, dtype, "drop path + lora rule"))


def test_refusals_and_plans_side_by_side(lib, cuda):
    case, L = CASES["L8"]
    B = case["batch"]
    x = R.vit_case_input(case).to(cuda)
    mask = IR.case_mask(case, L).to(cuda)
    err = lambda: lib.hct_last_error_string().decode()
    plain, _ = _vit(case, "fp32", cuda, mask_token=False)
    with pytest.raises(_lib.HctError, match="mask_token=True"):
        plain(x, masks=mask)
    _step(plain.train(), x)
    ptrs = (C.c_void_p * 1)(x.data_ptr())
    handle = plain._plans[(B, L)].handle
    assert lib.hct_vit_forward_parts_masked(handle, ptrs, 1, HCT_F32, mask.data_ptr(), _st()) != 0 and "without mask_token" in err()
    m, _ = _vit(case, "fp32", cuda)
    with pytest.raises(_lib.HctError, match="masks"):
        m(x, masks=mask[:, :-1])
    with pytest.raises(_lib.HctError, match="masks"):
        m(x, masks=mask.float())
    assert lib.hct_vit_forward_parts_masked(m._plan_for(B).handle, ptrs, 1, HCT_F32, None, _st()) != 0 and "hct_vit_forward_parts_masked" in err()
    # patch dropout together with masks
    both, _ = _vit(case, "fp32", cuda, patch_dropout=0.5)
    with pytest.raises(_lib.HctError, match="patch dropout and masks"):
        both.train()(x, masks=mask)
    dropped = _step(both.train(), x)  # the kept-patch plan of a backbone with the token: its backward writes the zero gradient
    assert dropped[0].shape[1] == 1 + case["num_register_tokens"] + 4 and torch.count_nonzero(dropped[1]["mask_token"]) == 0
    keep = both._plans[(B, 4)].handle
    assert lib.hct_vit_forward_parts_masked(keep, ptrs, 1, HCT_F32, mask.data_ptr(), _st()) != 0 and "patch_dropout" in err()
    with torch.no_grad():
        assert both.eval()(x, masks=mask)[0].shape[1] == 1 + case["num_register_tokens"] + L, "evaluation sees every patch, masks allowed"
    # a masked training forward, an unmasked validation forward at the same batch size in between, then the backward: the same plan, so the
    # backward of the overwritten forward is refused as stale -- and a fresh step is the step it always was
    first = _step(m.train(), x, mask)
    m.zero_grad()
    tok = m.train()(x, masks=mask)[0]
    with torch.no_grad():
        m.eval()(x)
    with pytest.raises(_lib.HctError, match="stale"):
        lora_ref.case_loss(tok).backward()
    assert _same(first, _step(m.train(), x, mask))
    torch.cuda.synchronize()


# ---- 4. wrapper and loss module ------------------------------------------------------------------------------------------------------------------
def _pair(cuda, dtype="fp32", K=512, return_cls=False):
    from headct_foundation_amd.dino_model import DINOHead, MultiCropWrapper
    case, L = CASES["L8"]
    vit, _ = _vit(case, dtype, cuda)
    torch.manual_seed(3)
    head = DINOHead(case["hidden_size"], K, hidden_dim=64, bottleneck_dim=32, compute_dtype=dtype)
    return MultiCropWrapper(vit, head, return_cls=return_cls).to(cuda), case, L


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_wrapper_gathers_pads_and_splits(lib, cuda, dtype):
    from headct_foundation_amd.ibot import ibot_rows_and_weights, pad_head_rows
    w, case, L = _pair(cuda, dtype)
    Bc, Rn, D = 2, case["num_register_tokens"], case["hidden_size"]
    T1 = 1 + Rn + L
    x = R.vit_case_input(dict(case, batch=3 * Bc)).to(cuda)
    crops = [x[:Bc], x[Bc:2 * Bc], x[2 * Bc:]]  # two global crops and one local: 6 samples, n_g = 4
    masks = np.zeros((2 * Bc, L), dtype=np.uint8)
    masks[1, [0, 3, 4]] = 1
    masks[2, [7]] = 1
    rows, weights, M = ibot_rows_and_weights(masks, Rn)
    assert M == 4 and pad_head_rows(3 * Bc + M) == 16
    w.train()
    w.zero_grad()
    tokens, seen = {}, {}

    def watch_logits(mod, inp, logits):  # the gradient that reaches the head's output, pad rows included (a tensor hook, set in the forward)
        if logits.requires_grad:
            logits.register_hook(lambda g: seen.update(dlogits=g.detach().clone()))

    hook = w.backbone.register_forward_hook(lambda mod, inp, out: tokens.update(t=out[0]))  # (returns None: the output stays what it is)
    hook_head = w.head.register_forward_hook(watch_logits)
    out = w(crops, masks=torch.from_numpy(masks).to(cuda), patch_rows=rows)
    hook.remove()
    hook_head.remove()
    tok = tokens["t"]
    tok.retain_grad()
    assert out["dino_output"].shape == (3 * Bc, 512) and out["ibot_output"].shape == (M, 512)
    with torch.no_grad():  # the head applied to the gathered rows: class rows, then the masked patch rows, then the padding
        flat = tok.detach().reshape(-1, D)
        idx = torch.cat((torch.arange(3 * Bc, device=cuda) * T1, torch.from_numpy(rows).long().to(cuda)))
        idx = torch.cat((idx, idx[-1:].expand(16 - idx.numel())))
        direct = w.head(flat[idx].contiguous())
    assert torch.equal(out["dino_output"], direct[:3 * Bc]) and torch.equal(out["ibot_output"], direct[3 * Bc:3 * Bc + M])
    # gradients: pad rows get an exact zero; dlatent is zero outside class rows and masked rows
    g = torch.Generator().manual_seed(1)
    ga, gb = torch.randn(3 * Bc, 512, generator=g).to(cuda), torch.randn(M, 512, generator=g).to(cuda)
    ((out["dino_output"].float() * ga).sum() + (out["ibot_output"].float() * gb).sum()).backward()
    torch.cuda.synchronize()
    dl = seen["dlogits"]
    assert dl.shape == (16, 512) and torch.count_nonzero(dl[3 * Bc + M:]) == 0, "pad rows receive an exact-zero logit gradient"
    assert torch.equal(dl[:3 * Bc].float(), ga.to(dl.dtype).float()) and torch.equal(dl[3 * Bc:3 * Bc + M].float(), gb.to(dl.dtype).float())
    dlat = tok.grad.reshape(-1, D)
    used = torch.zeros(3 * Bc * T1, dtype=torch.bool, device=cuda)
    used[idx[:3 * Bc + M]] = True
    assert torch.count_nonzero(dlat[~used]) == 0 and bool((dlat[used].abs().sum(1) > 0).all())
    assert float(w.backbone.mask_token.grad.abs().max()) > 0
    # the masks reached the backbone: its tokens are those of a direct masked forward with the local crops unmasked (after the backward:
    # another forward at this batch size overwrites the plan's activations)
    with torch.no_grad():
        full = torch.cat((torch.from_numpy(masks), torch.zeros(Bc, L, dtype=torch.uint8))).to(cuda)
        assert torch.equal(w.backbone(crops, masks=full)[0], tok.detach())
    # the teacher side: the same rows of an unmasked forward, no gradient.  Its class-token logits are those of the plain call up to the
    # order of the head's products, which run on 16 rows here and on 4 there: fp32 sums of 48 / 64 / 32 terms, bf16 logits rounded at 2^-9
    with torch.no_grad():
        t_out = w.eval()(crops[:2], patch_rows=rows)
        plain = w(crops[:2])
        flat = w.backbone(crops[:2])[0].reshape(-1, D)
        want = w.head(torch.cat((flat[torch.arange(4, device=cuda) * T1], flat[torch.from_numpy(rows).long().to(cuda)], flat[int(rows[-1])].expand(8, D))).contiguous())
    assert t_out["ibot_output"].shape == (M, 512) and torch.equal(t_out["ibot_output"], want[4:8]) and torch.equal(t_out["dino_output"], want[:4])
    assert rel_err(t_out["dino_output"], plain["dino_output"]) <= (1e-5 if dtype == "fp32" else 1e-2)
    with pytest.raises(_lib.HctError, match="patch_rows"):
        w(crops[:2], patch_rows=np.array([0], dtype=np.int32))  # a class-token row


def test_wrapper_refuses_batchnorm_heads(lib, cuda):
    from headct_foundation_amd.dino_model import DINOHead, MultiCropWrapper
    case, L = CASES["L8"]
    vit, _ = _vit(case, "fp32", cuda)
    w = MultiCropWrapper(vit, DINOHead(48, 512, use_bn=True, hidden_dim=64, bottleneck_dim=32, compute_dtype="fp32")).to(cuda)
    x = R.vit_case_input(case).to(cuda)
    with pytest.raises(ValueError, match="USE_BN"):
        w([x], patch_rows=np.array([2], dtype=np.int32))


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("centering", ["centering", "sinkhorn_knopp"])
def test_ibot_patch_loss_module(lib, cuda, centering, dt):
    from headct_foundation_amd.ibot import IBOTPatchLoss
    M, K, n_g = 37, 2052, 4
    inp = IR.loss_inputs(M, K, 1.0, dt, seed=9)
    crit = IBOTPatchLoss(K, 0.04, 0.07, 2, 5, centering=centering).to(cuda)
    crit.center.copy_(inp["center"])
    center0 = crit.center.clone()
    assert [float(v) for v in crit.teacher_temp_schedule] == [0.04, 0.07, 0.07, 0.07, 0.07], "DINOLoss's schedule"
    epoch, temp = 1, 0.07
    s = inp["student"].to(cuda).requires_grad_(True)
    loss = crit(s, inp["teacher"].to(cuda), inp["weight"].to(cuda), n_g, epoch)
    (loss * 3.0).backward()
    torch.cuda.synchronize()
    s64, t64, w64 = inp["student"].double(), inp["teacher"].double(), inp["weight"].double()
    sk = IR.sk_logs(inp["teacher"], temp, 3) if centering == "sinkhorn_knopp" else None
    want, dwant, csum = IR.ibot_loss(s64, t64, w64, 1.0 / n_g, TS, temp, center=inp["center"].double(), sk=sk)
    e_loss, e_grad = abs(float(loss) - float(want)) / abs(float(want)), H.worst_row(s.grad.float() / 3.0, dwant)
    print(f"IBOTPatchLoss {centering} {dt}: loss {e_loss:.2e} / {H.DINO_LOSS_BAR:.0e}, gradient {e_grad:.2e} / {H.DINO_GRAD_BAR[dt]:.0e}")
    assert s.grad.dtype == dt and e_loss < H.DINO_LOSS_BAR and e_grad < H.DINO_GRAD_BAR[dt]
    if centering == "centering":  # the centre moves by the restated update, its count the masked rows
        moved = H.center_update(center0.cpu()[0], csum.float(), 0.9, float(M))
        assert rel_err(crit.center.cpu()[0], moved) < 1e-6 and not torch.equal(crit.center, center0)
    else:
        assert torch.equal(_bits(crit.center), _bits(center0)), "the centre is not to be touched in this mode"
    with torch.no_grad():
        crit.center.copy_(center0)
        again = crit(s.detach(), inp["teacher"].to(cuda), inp["weight"].to(cuda), n_g, epoch)
    assert float(again) == float(loss)


@pytest.mark.parametrize("centering", ["centering", "sinkhorn_knopp"])
def test_two_emulated_ranks_with_unequal_rows(lib, cuda, centering):
    """Rank 0 holds 21 masked rows, rank 1 holds 16; each has n_g = 2 images.  With the row total given, the two ranks' losses average to the
    loss of one rank on all 37 rows with n_g = 4 (what the data-parallel mean of the per-rank losses is), and the centre sums add up.
    Sinkhorn-Knopp: the ranks' column passes are combined as combine_lse does over a process group (tests/test_dino_v2_gpu.py's two-rank
    case); lc and lr then carry at most 4 n b (its derivation), the bound that case derives, which moves log q by as much and the loss by
    that relative amount at most -- held beside the loss bar of each computation."""
    from headct_foundation_amd.dino import combine_lse, sk_col_lse, sk_row_lse, sinkhorn_knopp_logs
    from headct_foundation_amd.ibot import IBOTPatchLoss, _IbotLossFn
    M, K, n = 37, 1028, 3
    cut = 21
    inp = IR.loss_inputs(M, K, 1.0, F32, seed=4)
    s, t, w = (inp[k].to(cuda) for k in ("student", "teacher", "weight"))
    one = IBOTPatchLoss(K, TT, TT, 0, 5, centering=centering).to(cuda)
    whole = one(s, t, w, 4, 0, n_total=M)
    parts = [(s[:cut], t[:cut], w[:cut]), (s[cut:], t[cut:], w[cut:])]
    if centering == "centering":
        ranks = [IBOTPatchLoss(K, TT, TT, 0, 5).to(cuda) for _ in parts]
        losses = [r(a, b, c, 2, 0, n_total=len(a)) for r, (a, b, c) in zip(ranks, parts)]  # (each rank's own centre update is not the subject here)
        csums = []
        for a, b, c in parts:
            cs = torch.empty(K, device=cuda)
            _IbotLossFn.apply(a, b, c, 0.5, TS, TT, one.center.new_zeros(K), cs, None)
            csums.append(cs)
        total = torch.empty(K, device=cuda)
        _IbotLossFn.apply(s, t, w, 0.25, TS, TT, one.center.new_zeros(K), total, None)
        torch.cuda.synchronize()
        bound = H.product_sum_bound(M, 0, t.double().abs().sum(0).cpu()).numpy()
        assert ((csums[0] + csums[1]).double().cpu() - total.double().cpu()).abs().numpy().max() <= 2 * bound.max()
        tol = 2 * H.DINO_LOSS_BAR
    else:
        inv = V2.inv_temp32(TT)
        lrs = [None, None]
        for _ in range(n):
            lc = -math.log(K) - combine_lse([sk_col_lse(b, inv, l) for (_, b, _), l in zip(parts, lrs)])
            lrs = [-math.log(M) - sk_row_lse(b, inv, lc) for _, b, _ in parts]
        losses = [_IbotLossFn.apply(a, b, c, 0.5, TS, TT, None, None, (lc, l, math.log(M))) for (a, b, c), l in zip(parts, lrs)]
        lc1, lr1, log_n = sinkhorn_knopp_logs(t, TT, n, n_total=M)
        torch.cuda.synchronize()
        assert log_n == math.log(M)
        arg = float((t.double() * inv).abs().max()) + float(lr1.abs().max()) + float(lc1.abs().max())
        b = float(V2.lse_bound(arg, 16, arg))
        e_lc, e_lr = float((lc.cpu() - lc1.cpu()).abs().max()), float((torch.cat(lrs).cpu() - lr1.cpu()).abs().max())
        print(f"two ranks vs one: lc {e_lc:.2e}, lr {e_lr:.2e}, bound {4 * n * b:.2e}")
        assert e_lc <= 4 * n * b and e_lr <= 4 * n * b
        tol = 2 * H.DINO_LOSS_BAR + 2 * 4 * n * b
    mean = 0.5 * (float(losses[0]) + float(losses[1]))
    print(f"two ranks vs one ({centering}): {mean:.7f} vs {float(whole):.7f}, tolerance {tol:.2e}")
    assert abs(mean - float(whole)) / abs(float(whole)) <= tol


# ---- 5. main_pretrain_dino.py ----------------------------------------------------------------------------------------------------------------
def _run_main(tmp_path, tag, port, *extra):
    out = tmp_path / tag
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1", "--master-addr", "127.0.0.1", "--master-port", port,
           os.path.join(ROOT, "main_pretrain_dino.py"), "--local_rank", "0", "--model_name", "dino", "--batch_size", "2", "--max_epochs", "1",
           "--base_lr", "5e-4", "--cfg", os.path.join(ROOT, "configs", "dino", "dino_tiny_plumbing.yaml"), "--optimizer", "AdamW", "--scheduler", "cosine",
           *extra, "--opts", "DATA.SYNTHETIC_SAMPLES", "4", "MODEL.DIR", str(out), "LOG.OUTPUT_DIR", str(out / "log"), "OUTPUT", str(out / "json"),
           "MAE.COMPUTE_DTYPE", "fp32"]
    r = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=300)
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-4000:]
    return log, torch.load(out / "last_dino_tiny.pt", weights_only=True)


@pytest.mark.parametrize("centering,port", [("centering", "29681"), ("sinkhorn_knopp", "29682")])
def test_main_pretrain_dino_with_ibot(lib, cuda, tmp_path, centering, port):
    log, ckpt = _run_main(tmp_path, "ibot", port, "--ibot_weight", "1.0", "--centering", centering)
    lines = re.findall(r"Loss: ([-\d.naif]+)  dino_loss: ([-\d.naif]+)  ibot_loss: ([-\d.naif]+)", log)
    assert len(lines) == 2, log[-3000:]
    for total, dino, ibot in lines:
        assert all(math.isfinite(float(v)) for v in (total, dino, ibot)) and abs(float(total) - float(dino) - float(ibot)) < 2e-3
        assert float(ibot) > 0
    assert "Final test loss" in log and "Loss is" not in log
    assert re.search(r"Averaged stats:.*dino_loss.*ibot_loss", log)
    val = [l for l in log.splitlines() if "Final validation" in l or "Final test" in l]
    assert val and not any("ibot" in l for l in val), "validation and test report the DINO term alone"
    sd = ckpt["state_dict"]
    assert any(k.endswith("backbone.mask_token") for k in sd)
    assert any(k.endswith("backbone.mask_token") for k in ckpt["momentum_model_state_dict"])
    # the checkpoint loads back into a pair built like the run's
    strip = lambda d: {k[len("module."):]: v for k, v in d.items() if k.startswith("module.")}  # (the wrapper's own view of the pair)
    from headct_foundation_amd.dino_model import DINOHead, MultiCropWrapper, ViTBackbone
    vit = ViTBackbone(in_chans=3, img_size=24, patch_size=12, hidden_size=48, mlp_dim=96, num_layers=2, num_heads=3, pos_embed="sincos",
                      num_register_tokens=4, qkv_bias=True, compute_dtype="fp32", mask_token=True)
    pair = MultiCropWrapper(vit, DINOHead(48, 512, hidden_dim=64, bottleneck_dim=32, compute_dtype="fp32"))
    report = pair.load_state_dict(strip(sd), strict=True)
    assert not report.missing_keys and not report.unexpected_keys
    assert bool(torch.isfinite(pair.backbone.mask_token).all())


def test_main_pretrain_dino_weight_zero_is_the_plain_run(lib, cuda, tmp_path):
    log0, ck0 = _run_main(tmp_path, "zero", "29683", "--ibot_weight", "0")
    log1, ck1 = _run_main(tmp_path, "none", "29684")
    assert list(ck0["state_dict"]) == list(ck1["state_dict"]) and not any("mask_token" in k for k in ck0["state_dict"])
    first = lambda log: re.search(r"\[1/\d+\]  Loss: (\S+)", log).group(1)
    assert first(log0) == first(log1) and "ibot" not in "".join(l for l in log0.splitlines() if "Loss:" in l)
    assert all(torch.equal(ck0["state_dict"][k], ck1["state_dict"][k]) for k in ck0["state_dict"]), "the whole epoch is the same bits"
