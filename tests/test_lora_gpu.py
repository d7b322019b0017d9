"""GPU: LoRA fine-tuning of the ViT backbone (TRAIN.LORA) on the HIP path, against the torch restatement of tests/lora_ref.py (which
tests/test_lora_cpu.py pins to the reference's own modules): the two kernels' entry points through the C ABI, the full step with
both heads, the adapters' contribution on its own, freezing, the unchanged plain path, fresh adapters, and the entry point."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from oracle import mae_oracle as O
from tests import lora_ref as R
from tests.test_finetune_gpu import _abs_close, _attn_ref, _bn, _linear_ref, _rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANK = 128


def _vit(dtype, regs, hidden=48, heads=3, lora=True):
    from headct_foundation_amd.dino_model import ViTBackbone
    return ViTBackbone(in_chans=3, img_size=24, patch_size=12, hidden_size=hidden, mlp_dim=2 * hidden, num_layers=2, num_heads=heads,
                       num_register_tokens=regs, lora=lora, compute_dtype=dtype)


def _with_adapters(vit, b_std=0.005, tokens=True):
    """Adapters that do something (B = b_std randn; A keeps its standard-normal init) and class / register tokens that matter."""
    sd = vit.state_dict()
    for n in sd:
        if n.endswith("lora_matrix_B"):
            sd[n] = torch.randn(sd[n].shape) * b_std
        if tokens and n in ("cls_token", "register_tokens"):
            sd[n] = torch.randn(sd[n].shape) * 0.5
    vit.load_state_dict(sd, strict=True)
    return vit


# ---- 4. the kernels' entry points ------------------------------------------------------------------------------------
def _kernel_case(D, H, N, B, r, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    t = dict(x1=rn(B, N, D), qkv=rn(B, N, 3, H, D // H), dqkv=rn(B, N, 3, H, D // H), dx0=rn(B, N, D),
             Aq=rn(r, D), Av=rn(r, D), Bq=rn(D, r) * 0.05, Bv=rn(D, r) * 0.05)
    if dtype == "bf16":
        t = {k: v.bfloat16().float() for k, v in t.items()}
    return t


def _kernel_ref(t, H, dtype):
    """(updated qkv, T, dAq, dAv, dBq, dBv, dx1 increment) of the restatement; fp64 for the fp32 kernels, bf16 storage emulation for bf16."""
    emu = dtype == "bf16"
    cast = (lambda v: v.clone()) if emu else (lambda v: v.double())
    p = {k: cast(v) for k, v in t.items()}
    for k in ("x1", "Aq", "Av", "Bq", "Bv"):
        p[k].requires_grad_(True)
    old = O._EMU[0]
    O._EMU[0] = emu
    try:
        qkv = p["qkv"].permute(2, 0, 3, 1, 4)  # [3, B, H, N, dh]
        q = O._r(qkv[0] + R.lora_update(p["x1"], p["Aq"], p["Bq"], H))
        v = O._r(qkv[2] + R.lora_update(p["x1"], p["Av"], p["Bv"], H))
        T = torch.cat([O._r(p["x1"] @ p["Aq"].T), O._r(p["x1"] @ p["Av"].T)], dim=-1)
        out = torch.stack([q, qkv[1], v]).permute(1, 3, 0, 2, 4)  # back to [B, N, 3, H, dh]
        dq = p["dqkv"].permute(2, 0, 3, 1, 4)
        ((q * dq[0]).sum() + (v * dq[2]).sum()).backward()
    finally:
        O._EMU[0] = old
    return out.detach(), T.detach(), p["Aq"].grad, p["Av"].grad, p["Bq"].grad, p["Bv"].grad, p["x1"].grad


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("D,H,N,B,r", [(768, 12, 513, 2, 128), (48, 3, 11, 2, 128), (48, 3, 9, 3, 32), (128, 2, 9, 2, 128), (128, 2, 37, 3, 64)])
def test_lora_kernels_vs_restatement(lib, cuda, dtype, D, H, N, B, r):
    from headct_foundation_amd import _lib
    tol = 1e-3 if dtype == "fp32" else 2e-2
    code, tdt = (_lib.HCT_F32, torch.float32) if dtype == "fp32" else (_lib.HCT_BF16, torch.bfloat16)
    t = _kernel_case(D, H, N, B, r, dtype, seed=D + N + r)
    want = _kernel_ref(t, H, dtype)
    d = {k: v.to(cuda, tdt).contiguous() for k, v in t.items()}
    st = torch.cuda.current_stream().cuda_stream
    M = B * N
    T = torch.zeros(M, 2 * r, dtype=tdt, device=cuda)
    qkv = d["qkv"].clone()
    _lib.check(lib.hct_lora_qv_fwd(d["x1"].data_ptr(), d["Aq"].data_ptr(), d["Av"].data_ptr(), d["Bq"].data_ptr(), d["Bv"].data_ptr(), B, N, H,
                                   D // H, r, code, T.data_ptr(), qkv.data_ptr(), st), "hct_lora_qv_fwd")
    errs = {"qkv": _rel(qkv, want[0]), "T": _rel(T.view(B, N, 2 * r), want[1])}
    # the update itself, not hidden behind the stored values: (qkv after) - (qkv before) against the restatement's
    errs["update"] = _rel(qkv.float() - d["qkv"].float(), want[0].float() - t["qkv"])
    assert torch.equal(qkv[:, :, 1], d["qkv"][:, :, 1]), "the k slot must stay untouched"
    nbytes = lib.hct_lora_qv_bwd_workspace_bytes(M, D, r, code)
    ws = torch.empty(max(16, nbytes), dtype=torch.uint8, device=cuda)
    tr = {k: (d[k].t().contiguous() if dtype == "bf16" else None) for k in ("Aq", "Av", "Bq", "Bv")}
    ptr = lambda v: None if v is None else v.data_ptr()
    for base, key in ((torch.zeros_like(d["dx0"]), "dx1 increment"), (d["dx0"].clone(), "dx1 sum")):
        g = {k: torch.full(d[k].shape, float("nan"), dtype=torch.float32, device=cuda) for k in ("Aq", "Av", "Bq", "Bv")}
        dx = base.clone()
        _lib.check(lib.hct_lora_qv_bwd(d["dqkv"].data_ptr(), d["x1"].data_ptr(), T.data_ptr(), d["Aq"].data_ptr(), d["Av"].data_ptr(),
                                       d["Bq"].data_ptr(), d["Bv"].data_ptr(), ptr(tr["Aq"]), ptr(tr["Av"]), ptr(tr["Bq"]), ptr(tr["Bv"]), B, N, H,
                                       D // H, r, code, g["Aq"].data_ptr(), g["Av"].data_ptr(), g["Bq"].data_ptr(), g["Bv"].data_ptr(),
                                       dx.data_ptr(), ws.data_ptr(), ws.numel(), st), "hct_lora_qv_bwd")
        errs[key] = _rel(dx, base.float().cpu() + want[6].float())
        for i, k in enumerate(("Aq", "Av", "Bq", "Bv")):
            errs["d" + k] = _rel(g[k], want[2 + i])
    print("lora kernels", dtype, (D, H, N, B, r), {k: f"{e:.2e}" for k, e in errs.items()})
    for k, e in errs.items():
        assert e < tol, (k, e)


@pytest.mark.gpu
def test_lora_kernels_refuse_other_ranks(lib, cuda):
    from headct_foundation_amd import _lib
    z = torch.zeros(4096, device=cuda)
    for r in (8, 48, 0):
        rc = lib.hct_lora_qv_fwd(z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), 1, 4, 2, 8, r, _lib.HCT_F32, z.data_ptr(),
                                 z.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc != 0 and b"multiple of 32" in lib.hct_last_error_string()


# ---- 5. the full step ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype,regs,hidden,heads,head", [("fp32", 0, 48, 3, "linear"), ("fp32", 2, 48, 3, "attentive"),
                                                          ("fp32", 0, 128, 2, "attentive"), ("bf16", 0, 48, 3, "linear"),
                                                          ("bf16", 2, 48, 3, "attentive")])
def test_full_lora_step_vs_restatement(lib, cuda, dtype, regs, hidden, heads, head):
    """test_full_finetune_step_vs_oracle with lora=True, B = 0.005 randn, under the LoRA freezing rule: loss and every trainable
    gradient at that test's bars (fp32 1e-3, bf16 5e-2), the batch-cancelling vectors treated as there."""
    from headct_foundation_amd import AttentionClassifier, LinearClassifier, cross_entropy
    from headct_foundation_amd.misc import set_requires_grad_false
    torch.manual_seed(4)
    tol = 1e-3 if dtype == "fp32" else 5e-2
    vit = _with_adapters(_vit(dtype, regs, hidden, heads)).to(cuda)
    set_requires_grad_false(vit, lora=True)
    cls = (LinearClassifier(hidden, 2, feature_grad=True) if head == "linear" else
           AttentionClassifier(hidden, 2, num_heads=heads * 2 if hidden % (heads * 2) == 0 else heads, compute_dtype=dtype)).to(cuda).train()
    B = 8
    x = torch.rand(B, 3, 24, 24, 24) * torch.tensor([0.5, 1.0, 2.0, 3.0, 4.0, 6.0, 8.0, 12.0]).view(-1, 1, 1, 1, 1)
    tg = torch.tensor([0, 1, 1, 0, 1, 0, 0, 1])
    vit.train()
    loss = cross_entropy(cls(vit(x.to(cuda))[0]), tg.to(cuda))
    loss.backward()
    pv = {k: v.detach().cpu().float().clone().requires_grad_(True) for k, v in vit.state_dict().items()}
    ph = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in cls.named_parameters()}
    tok, _ = R.vit_forward(pv, x, 12, heads, 2)
    if head == "linear":
        logits = _linear_ref(tok[:, 0], ph["linear.weight"], ph["linear.bias"], _bn(hidden))
    else:
        logits = _attn_ref(tok, ph, cls.num_heads, 1, cls.scale, _bn(hidden), _bn(hidden))
    F.cross_entropy(logits, tg).backward()
    assert abs(float(loss.detach()) - float(F.cross_entropy(logits, tg).detach())) < tol * abs(float(loss.detach()))
    named = dict(vit.named_parameters())
    scale = float(pv["patch_embedding.position_embeddings"].grad.norm())
    errs, trainable = {}, []
    for k, v in named.items():
        if not R.trainable(k):
            assert not v.requires_grad and v.grad is None, k
            continue
        trainable.append(k)
        ref = pv[k].grad
        summed = ref.dim() == 1 or k in ("cls_token", "register_tokens")
        if k in ("norm.weight", "norm.bias") or (summed and head == "linear" and dtype == "bf16"):
            assert float((v.grad.float().cpu() - ref).norm()) < tol * max(scale, float(ref.norm())), k
        else:
            errs[k] = _rel(v.grad, ref)
    print("per-parameter relative errors (lora)", dtype, head, {k: round(e, 4) for k, e in errs.items()})
    assert sum("lora" in k for k in errs) == 8
    for k, e in errs.items():
        assert e < tol, (k, e)
    got = torch.cat([named[k].grad.float().cpu().flatten() for k in trainable])
    assert _rel(got, torch.cat([pv[k].grad.flatten() for k in trainable])) < tol
    for k, v in cls.named_parameters():
        if k == "wkv.bias":
            assert _abs_close(v.grad, ph[k].grad, ph["wkv.weight"].grad, tol), k
        else:
            assert _rel(v.grad, ph[k].grad) < tol, k
    g0 = vit._flat_grad.clone(), cls._flat_grad.clone()
    vit.zero_grad()
    cls.zero_grad()
    cross_entropy(cls(vit(x.to(cuda))[0]), tg.to(cuda)).backward()
    assert torch.equal(g0[0], vit._flat_grad) and torch.equal(g0[1], cls._flat_grad)


# ---- 6. the adapters' contribution itself ---------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("regs,hidden,heads", [(2, 48, 3), (0, 128, 2)])
def test_adapter_contribution_fp32(lib, cuda, regs, hidden, heads):
    torch.manual_seed(6)
    vit = _with_adapters(_vit("fp32", regs, hidden, heads))
    sd = {k: v.clone() for k, v in vit.state_dict().items()}
    sd0 = {k: (torch.zeros_like(v) if k.endswith("lora_matrix_B") else v) for k, v in sd.items()}
    x = torch.rand(4, 3, 24, 24, 24) * 2.0
    vit = vit.to(cuda)
    with torch.no_grad():
        with_a = vit(x.to(cuda))[0].float().cpu()
        vit.load_state_dict(sd0, strict=True)
        without = vit(x.to(cuda))[0].float().cpu()
    p = lambda d: {k: v.double() for k, v in d.items()}
    ref = R.vit_forward(p(sd), x.double(), 12, heads, 2)[0] - R.vit_forward(p(sd0), x.double(), 12, heads, 2)[0]
    share = float(ref.norm() / R.vit_forward(p(sd), x.double(), 12, heads, 2)[0].norm())
    err = _rel(with_a - without, ref)
    print("adapter contribution: share of the output norm", round(share, 4), "relative error of the difference", err)
    assert share > 0.02 and err < 1e-3


# ---- 7. freezing -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_frozen_parameters_stay_and_trainable_move(lib, cuda, dtype):
    from headct_foundation_amd.misc import set_requires_grad_false
    from headct_foundation_amd.optim import HipAdamW, clip_grad_norm_
    torch.manual_seed(7)
    vit = _with_adapters(_vit(dtype, 2)).to(cuda)
    set_requires_grad_false(vit, lora=True)
    opt = HipAdamW(vit, lr=1e-3, weight_decay=0.04)
    x = (torch.rand(4, 3, 24, 24, 24) * 2.0).to(cuda)
    start = {k: v.detach().clone() for k, v in vit.named_parameters()}

    def backward():
        R.case_loss(vit(x)[0].float()).backward()

    for step in range(5):
        opt.zero_grad()
        backward()
        if step == 0:
            g0 = vit._flat_grad.clone()
            opt.zero_grad()
            backward()
            assert torch.equal(g0, vit._flat_grad), "a repeated backward after zero_grad must be bit-identical"
            grads = [p.grad.detach().float().cpu().clone() for p in vit.parameters() if p.requires_grad]
            assert all(p.grad is None for p in vit.parameters() if not p.requires_grad)
            holders = [torch.nn.Parameter(torch.zeros_like(g)) for g in grads]
            for h, g in zip(holders, grads):
                h.grad = g.clone()
            want = torch.nn.utils.clip_grad_norm_(holders, 1.0)
            got = clip_grad_norm_(vit, 1.0)
            assert abs(float(got) - float(want)) < 1e-5 * float(want), (float(got), float(want))
            for p, h in zip([p for p in vit.parameters() if p.requires_grad], holders):
                assert _rel(p.grad, h.grad) < 1e-5
        else:
            clip_grad_norm_(vit, 1.0)
        opt.step()
    torch.cuda.synchronize()
    for k, v in vit.named_parameters():
        if R.trainable(k):
            assert v.requires_grad and not torch.equal(v.detach(), start[k]), k
        else:
            assert not v.requires_grad and v.grad is None and torch.equal(v.detach(), start[k]), k


# ---- 8. the plain path is the parent's ------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_plain_gradients_unchanged_by_flag_mechanism(lib, cuda, dtype):
    """lora=False, every parameter trainable: the gradients with the flags untouched, and after the flags were set to frozen and
    back to trainable explicitly, are bit-identical (the launch sequence is the same one)."""
    from headct_foundation_amd.misc import set_requires_grad_false
    torch.manual_seed(8)
    vit = _vit(dtype, 2, lora=False).to(cuda)
    x = (torch.rand(4, 3, 24, 24, 24) * 2.0).to(cuda)

    def grads():
        vit.zero_grad()
        R.case_loss(vit(x)[0].float()).backward()
        return vit._flat_grad.clone()

    g_untouched = grads()
    set_requires_grad_false(vit, lora=True)
    g_frozen = grads()
    for p in vit.parameters():
        p.requires_grad_(True)
    g_explicit = grads()
    assert torch.equal(g_untouched, g_explicit)
    # frozen matrices: their slices are zero, every trainable slice is what it was
    for name, off, numel, *_ in vit._layout:
        if R.trainable(name):
            assert torch.equal(g_frozen[off:off + numel], g_untouched[off:off + numel]), name
        else:
            assert not g_frozen[off:off + numel].any() and g_untouched[off:off + numel].any(), name


# ---- 9. fresh adapters (B = 0) ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype,hidden,heads", [("fp32", 48, 3), ("bf16", 48, 3), ("bf16", 128, 2)])
def test_fresh_adapters_change_nothing(lib, cuda, dtype, hidden, heads):
    torch.manual_seed(9)
    lora = _vit(dtype, 2, hidden, heads)
    plain = _vit(dtype, 2, hidden, heads, lora=False)
    plain.load_state_dict({k: v for k, v in lora.state_dict().items() if "lora" not in k}, strict=True)
    lora, plain = lora.to(cuda), plain.to(cuda)
    x = (torch.rand(4, 3, 24, 24, 24) * 2.0).to(cuda)
    with torch.no_grad():
        want = plain(x)[0]
    tok = lora(x)[0]
    assert torch.equal(tok.detach(), want)
    R.case_loss(tok.float()).backward()
    for k, v in lora.named_parameters():
        if k.endswith("lora_matrix_A"):
            assert not v.grad.any(), k     # dT = dU . B is an exact zero
        if k.endswith("lora_matrix_B"):
            assert v.grad.any() and torch.isfinite(v.grad).all(), k


# ---- forward-only ViT ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_forward_only_vit_with_adapters(lib, cuda, dtype):
    from headct_foundation_amd.vit import ViT
    torch.manual_seed(10)
    bb = _with_adapters(_vit(dtype, 2))
    m = ViT(in_chans=3, img_size=24, patch_size=12, hidden_size=48, mlp_dim=96, num_layers=2, num_heads=3, num_register_tokens=2, lora=True,
            compute_dtype=dtype)
    m.load_state_dict(bb.state_dict(), strict=True)
    x = torch.rand(2, 3, 24, 24, 24) * 2.0
    out, hidden = m.to(cuda)(x.to(cuda))
    ref, _ = R.vit_forward({k: v.double() for k, v in bb.state_dict().items()}, x.double(), 12, 3, 2)
    assert len(hidden) == 2 and _rel(out, ref) < (1e-3 if dtype == "fp32" else 3e-2)


# ---- 10. the entry point and a short loop ------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("head", ["linear", "attentive"])
def test_main_downstream_lora_run(lib, cuda, tmp_path, head):
    """test_main_downstream_plumbing_run with TRAIN.LORA True: the pre-training checkpoint has no adapter keys, the saved one has."""
    from headct_foundation_amd.dino_model import ViTBackbone
    vit = _vit("fp32", 0, lora=False)
    sd = {"module." + k: v for k, v in vit.state_dict().items()}
    sd["module.decoder_embed.weight"] = torch.zeros(8, 48)
    torch.save({"state_dict": sd, "epoch": 3}, tmp_path / "pre.pt")
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("MODEL:\n  NAME: vit\n")
    opts = ["DATA.SYNTHETIC", "True", "DATA.SYNTHETIC_SAMPLES", "8", "VIT.INPUT_SIZE", "24", "VIT.PATCH_SIZE", "12",
            "VIT.HIDDEN_SIZE", "48", "VIT.MLP_DIM", "96", "VIT.NUM_LAYERS", "2", "VIT.NUM_HEADS", "3", "TRAIN.VAL_EVERY", "1",
            "MODEL.DIR", str(tmp_path / "out"), "MODEL.SAVE_NAME", "ft.pt", "LOG.OUTPUT_DIR", str(tmp_path / "log"),
            "PREDS_SAVE_NAME", "run", "TRAIN.LORA", "True"]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nproc-per-node", "1", "--master-port", "29617",
           os.path.join(ROOT, "main_downstream.py"), "--cfg", str(cfg), "--model_name", "vit", "--model_load_path", str(tmp_path / "pre.pt"),
           "--classifier", head, "--batch_size", "4", "--max_epochs", "2", "--grad_clip", "1.0", "--base_lr", "1e-4", "--opts"] + opts
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-4000:]
    assert "MulticlassAccuracy" in log and "MulticlassAUROC" in log and "Final test loss" in log, log[-4000:]
    lora = ViTBackbone(in_chans=3, img_size=24, patch_size=12, hidden_size=48, mlp_dim=96, num_layers=2, num_heads=3, lora=True)
    n_train = sum(p.numel() for n, p in lora.named_parameters() if R.trainable(n))
    assert f"Total trainable parameters: {n_train}" in log, log[-4000:]
    b = torch.load(tmp_path / "out" / "ft.pt", weights_only=True)
    lora.load_state_dict(b["state_dict"], strict=True)
    for k, v in vit.state_dict().items():  # the frozen tensors are the checkpoint's, bit for bit
        if not R.trainable(k):
            assert torch.equal(b["state_dict"][k].cpu(), v), k
    assert any(bool(v.any()) for k, v in b["state_dict"].items() if k.endswith("lora_matrix_B")), "the adapters were trained"


@pytest.mark.gpu
@pytest.mark.parametrize("head", ["linear", "attentive"])
def test_lora_loop_halves_loss(lib, cuda, head):
    """test_finetune_loop_halves_loss (same data, same optimizers, same bar) with LoRA fine-tuning instead of full fine-tuning."""
    from headct_foundation_amd import AttentionClassifier, LinearClassifier, cross_entropy
    from headct_foundation_amd.data import SyntheticLabelled
    from headct_foundation_amd.misc import set_requires_grad_false
    from headct_foundation_amd.optim import HipAdamW, clip_grad_norm_
    torch.manual_seed(5)
    vit = _vit("bf16", 0).to(cuda)
    set_requires_grad_false(vit, lora=True)
    cls = (LinearClassifier(48, 2, feature_grad=True) if head == "linear" else AttentionClassifier(48, 2, num_heads=12, compute_dtype="bf16")).to(cuda).train()
    opts = [HipAdamW(cls, lr=1e-3, weight_decay=0.04), HipAdamW(vit, lr=1e-5, weight_decay=0.04)]
    v, t, _ = SyntheticLabelled(1, 16, 3, 24, 2, cuda, seed=0).batches[0]
    before = {k: p.detach().clone() for k, p in vit.named_parameters()}
    losses = []
    for _ in range(30):
        for o in opts:
            o.zero_grad()
        loss = cross_entropy(cls(vit(v)[0]), t)
        loss.backward()
        clip_grad_norm_(cls, 1.0)
        clip_grad_norm_(vit, 1.0)
        for o in opts:
            o.step()
        losses.append(float(loss.detach()))
    assert losses[-1] < 0.5 * losses[0], losses
    for k, p in vit.named_parameters():
        assert torch.equal(p.detach(), before[k]) == (not R.trainable(k)), k
