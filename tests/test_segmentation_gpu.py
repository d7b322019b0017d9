"""GPU: the segmentation kernels of csrc/segmentation.hip through the C ABI against tests/seg_ref.py (float64, fed the stored logits),
inside NaN-filled guarded allocations with the logits given as strided views; then the head, the autograd wrappers, training on one
synthetic batch and the entry point.  Every bound is derived in tests/seg_ref.py; none comes from a kernel's output."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from headct_foundation_amd import _lib
from tests import seg_ref as R
from tests.test_assembly_kernels_gpu import _Out, _bits, _code, _st

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
W_CE, W_DICE = 1.0, 0.5


class _Bytes:
    """An integer output (uint8 / int64) inside a guarded buffer: body and guards hold a sentinel."""

    def __init__(self, shape, dtype, dev, fill=99):
        n = int(np.prod(shape))
        self.g = 64
        self.buf = torch.full((n + 2 * self.g,), fill, dtype=dtype, device=dev)
        self.fill, self.n = fill, n
        self.t = self.buf[self.g:self.g + n].view(shape)
        self.ptr = self.t.data_ptr()

    def result(self):
        assert bool((self.buf[:self.g] == self.fill).all()) and bool((self.buf[self.g + self.n:] == self.fill).all()), "guard band written"
        return self.t.cpu()


def _ws(nbytes, dev):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=dev)


def _case(name, dtype):
    c = R.LOSS_CASES[name]
    tok, y = R.make_case(c["B"], c["G"], c["P"], c["K"], c["first"], seed=len(name), pad=c["pad"], dtype=dtype)
    return c, tok, y


def _class_weight(K):
    return torch.linspace(0.5, 2.0, K, dtype=F32)


def _loss_call(lib, c, logits_d, y_d, cw_d, dev, dloss=None, inplace=False, want_loss=True):
    """One hct_seg_loss call; logits_d is the [B, T, N + pad] device buffer, read through its [:, :, :N] view."""
    B, G, P, K, first = c["B"], c["G"], c["P"], c["K"], c["first"]
    T, N = first + G ** 3, K * P ** 3
    ld = logits_d.stride(1)
    outs = {}
    if want_loss:
        outs = dict(loss=_Out((1,), F32, dev), ce=_Out((1,), F32, dev), dice=_Out((1,), F32, dev), dice_bc=_Out((B, K), F32, dev))
    if inplace:
        dl = _Out(tuple(logits_d.shape), logits_d.dtype, dev)
        dl.t.copy_(logits_d)
        src = dl.t
    else:
        dl = _Out(tuple(logits_d.shape), logits_d.dtype, dev)
        src = logits_d
    outs["dlogits"] = dl
    ws = _ws(lib.hct_seg_loss_workspace_bytes(B, G, P, K), dev)
    g = lambda k: outs[k].ptr if k in outs else None
    rc = lib.hct_seg_loss(src.data_ptr(), _code(logits_d.dtype), ld, y_d.data_ptr(), cw_d.data_ptr(), B, T, first, G, P, K, W_CE, W_DICE,
                          None if dloss is None else dloss.data_ptr(), g("loss"), g("ce"), g("dice"), g("dice_bc"), dl.ptr, ld, 0,
                          ws.data_ptr(), ws.numel(), _st())
    _lib.check(rc, "hct_seg_loss")
    return outs


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", list(R.LOSS_CASES))
def test_seg_loss_kernel(lib, cuda, name, dtype):
    c, tok, y = _case(name, dtype)
    B, G, P, K, first = c["B"], c["G"], c["P"], c["K"], c["first"]
    N, T = K * P ** 3, first + G ** 3
    cw = _class_weight(K)
    logits_d, y_d, cw_d = tok.to(cuda), y.to(cuda), cw.to(cuda)
    a = _loss_call(lib, c, logits_d, y_d, cw_d, cuda)
    b = _loss_call(lib, c, logits_d, y_d, cw_d, cuda)
    two = _loss_call(lib, c, logits_d, y_d, cw_d, cuda, dloss=torch.tensor([2.0], device=cuda), want_loss=False)
    inp = _loss_call(lib, c, logits_d, y_d, cw_d, cuda, inplace=True, want_loss=False)
    torch.cuda.synchronize()
    got = {k: v.result() for k, v in a.items()}
    for k, v in b.items():
        assert torch.equal(_bits(v.result()), _bits(got[k])), f"{k}: a second identical call differs"
    # the reference, fed the stored logits
    vec = 4 if (P % 4 == 0 and (N + c["pad"]) % 4 == 0) else 1
    _, trips, nb = R.work_split(G * P, vec)
    r = R.loss_parts(R.unpatchify(tok.to(F64), first, G, P, K), y, W_CE, W_DICE, cw)
    bd = R.loss_bounds(r, K, W_CE, W_DICE, run=trips * vec, out_bf16=dtype == BF16)
    for k in ("loss", "ce", "dice"):
        err = abs(float(got[k][0]) - float(r[k]))
        print(f"{name} {k}: {float(got[k][0]):.8f} ref {float(r[k]):.8f} err {err:.2e} bound {float(bd[k]):.2e}")
        assert err <= float(bd[k]), (k, err, float(bd[k]))
    e = (got["dice_bc"].to(F64) - r["dice_bc"]).abs()
    print(f"{name} dice_bc: worst err / bound {float((e / bd['dice_bc']).max()):.3f}")
    assert bool((e <= bd["dice_bc"]).all())
    assert float(got["dice_bc"][B - 1].min()) == 1.0  # the all-ignored sample
    dl = got["dlogits"]
    assert bool(torch.isnan(dl[:, :, N:]).all()), "pad columns of dlogits were written"
    body = dl[:, :, :N]
    assert not bool(torch.isnan(body).any())
    if first:
        assert bool((body[:, :first] == 0).all()), "leading rows are not zero"
    gv = R.unpatchify(body.to(F64), first, G, P, K)
    ign = (y.to(torch.int64) >= K).unsqueeze(1).expand_as(gv)
    assert bool((gv[ign] == 0).all()), "gradient at ignored voxels is not zero"
    e = (gv - r["grad"]).abs()
    print(f"{name} dlogits: worst err / bound {float((e / bd['grad']).max()):.3f}, max |grad| {float(r['grad'].abs().max()):.3e}")
    assert bool((e <= bd["grad"]).all())
    # dloss = 2: twice the gradient, bit for bit; in place: the same bits as out of place
    g2 = two["dlogits"].result()[:, :, :N]
    assert torch.equal(g2.to(F64), 2 * body.to(F64))
    gi = inp["dlogits"].result()[:, :, :N]
    assert torch.equal(_bits(gi.contiguous()), _bits(body.contiguous()))


def test_seg_loss_no_valid_voxel_and_reuse(lib, cuda):
    """A batch with no valid voxel: loss 0, zero gradient.  reuse_stats: the gradient phase alone gives the full call's bits."""
    c, tok, y = _case("odd_K_first2", F32)
    B, G, P, K, first = c["B"], c["G"], c["P"], c["K"], c["first"]
    T, N = first + G ** 3, K * P ** 3
    cw_d, logits_d = _class_weight(K).to(cuda), tok.to(cuda)
    none = torch.full_like(y, 255).to(cuda)
    o = _loss_call(lib, c, logits_d, none, cw_d, cuda)
    torch.cuda.synchronize()
    assert float(o["loss"].result()[0]) == 0.0 and float(o["ce"].result()[0]) == 0.0 and float(o["dice"].result()[0]) == 0.0
    assert bool((o["dlogits"].result()[:, :, :N] == 0).all())
    y_d = y.to(cuda)
    full = _loss_call(lib, c, logits_d, y_d, cw_d, cuda)
    ws = _ws(lib.hct_seg_loss_workspace_bytes(B, G, P, K), cuda)
    ld = logits_d.stride(1)
    loss = torch.empty(1, device=cuda)
    args = (logits_d.data_ptr(), _code(F32), ld, y_d.data_ptr(), cw_d.data_ptr(), B, T, first, G, P, K, W_CE, W_DICE, None)
    _lib.check(lib.hct_seg_loss(*args, loss.data_ptr(), None, None, None, None, 0, 0, ws.data_ptr(), ws.numel(), _st()), "stats")
    dl = _Out(tuple(logits_d.shape), F32, cuda)
    _lib.check(lib.hct_seg_loss(*args, None, None, None, None, dl.ptr, ld, 1, ws.data_ptr(), ws.numel(), _st()), "gradient")
    torch.cuda.synchronize()
    assert torch.equal(_bits(dl.result()[:, :, :N].contiguous()), _bits(full["dlogits"].result()[:, :, :N].contiguous()))
    assert torch.equal(_bits(loss.cpu()), _bits(full["loss"].result()))
    # refusals: a workspace that is too small, more classes than the kernels hold
    rc = lib.hct_seg_loss(*args, loss.data_ptr(), None, None, None, None, 0, 0, ws.data_ptr(), 8, _st())
    assert rc != 0 and "workspace" in lib.hct_last_error_string().decode()
    assert lib.hct_seg_loss_workspace_bytes(B, G, P, 17) == 0


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", ["odd_K_first2", "two_partials", "one_voxel_access", "K_below_bound"])
def test_seg_predict_kernel(lib, cuda, name, dtype):
    """Integer logits with planted ties: labels and counts exact, the probability within fp16 rounding of the softmax."""
    c = R.LOSS_CASES[name]
    B, G, P, K, first = c["B"], c["G"], c["P"], c["K"], c["first"]
    T, N, S = first + G ** 3, K * P ** 3, G * P
    gen = torch.Generator().manual_seed(3)
    vol = torch.randint(-2, 3, (B, K, S, S, S), generator=gen).to(F64)  # 5 values over K classes: ties everywhere
    vol[:, :, 0, 0, :] = 1.0  # a row where every class ties: class 0 wins
    y = torch.randint(0, K, (B, S, S, S), generator=gen).to(torch.uint8)
    y[torch.rand(B, S, S, S, generator=gen) < 0.15] = 255
    tok = torch.full((B, T, N + c["pad"]), float("nan"), dtype=F64)
    tok[:, :, :N] = R.patchify(vol, first, T, G, P)
    tok[:, :first] = float("nan")
    logits_d, y_d = tok.to(dtype).to(cuda), y.to(cuda)
    pc = K - 1
    pred, prob, cnt = _Bytes((B, S, S, S), torch.uint8, cuda), _Out((B, S, S, S), torch.float16, cuda), _Bytes((B, K, 3), torch.int64, cuda, -5)
    ws = _ws(lib.hct_seg_predict_workspace_bytes(B, G, P, K), cuda)
    _lib.check(lib.hct_seg_predict(logits_d.data_ptr(), _code(dtype), logits_d.stride(1), y_d.data_ptr(), B, T, first, G, P, K, pc, pred.ptr,
                                   prob.ptr, cnt.ptr, ws.data_ptr(), ws.numel(), _st()), "hct_seg_predict")
    torch.cuda.synchronize()
    want = R.predict(vol)
    assert torch.equal(pred.result(), want)
    assert bool((want[:, 0, 0, :] == 0).all())
    assert np.array_equal(cnt.result().numpy(), R.counts(want, y, K))
    p = torch.softmax(vol, dim=1)[:, pc]
    e = (prob.result().to(F64) - p).abs()
    bound = 2.0 ** -11 * p + 2.0 ** -25 + R.U * (R.A_P + R.c_p(K) * p)  # half an fp16 ulp (or half the subnormal spacing) + the softmax's own
    assert bool((e <= bound).all()), float((e / bound).max())
    # pred alone, no labels, no workspace
    pred2 = _Bytes((B, S, S, S), torch.uint8, cuda)
    _lib.check(lib.hct_seg_predict(logits_d.data_ptr(), _code(dtype), logits_d.stride(1), None, B, T, first, G, P, K, 0, pred2.ptr, None, None,
                                   None, 0, _st()), "hct_seg_predict")
    torch.cuda.synchronize()
    assert torch.equal(pred2.result(), want)


@pytest.mark.parametrize("S", [8, 12])
def test_gather_flip_labels_kernel(lib, cuda, S):
    gen = torch.Generator().manual_seed(S)
    pool = torch.randint(0, 256, (3, S, S, S), generator=gen).to(torch.uint8)
    slots = torch.tensor([0, 1, 2, 0, 1, 2, 0, 1, -1, 1, 1], dtype=torch.int32)  # all 8 codes, slot -1, a repeated slot
    flip = torch.tensor([0, 1, 2, 3, 4, 5, 6, 7, 5, 7, 7], dtype=torch.uint8)
    B = slots.numel()
    out = _Bytes((B, S, S, S), torch.uint8, cuda, 77)
    pool_d, slots_d, flip_d = pool.to(cuda), slots.to(cuda), flip.to(cuda)
    _lib.check(lib.hct_gather_flip_labels(pool_d.data_ptr(), slots_d.data_ptr(), out.ptr, B, S, 3, flip_d.data_ptr(), _st()), "flip")
    torch.cuda.synchronize()
    assert torch.equal(out.result(), R.flip_labels(pool, slots, flip))
    out2 = _Bytes((B, S, S, S), torch.uint8, cuda, 77)
    _lib.check(lib.hct_gather_flip_labels(pool_d.data_ptr(), slots_d.data_ptr(), out2.ptr, B, S, 3, None, _st()), "flip")
    torch.cuda.synchronize()
    assert torch.equal(out2.result(), R.flip_labels(pool, slots, torch.zeros(B, dtype=torch.uint8)))


# ---- head + autograd ------------------------------------------------------------------------------------------------------------
def _rel(a, b):
    a, b = a.detach().to(F64).cpu(), b.detach().to(F64).cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _composed(tokens, W, b, y, first, G, P, K, cw):
    """The torch composition on the same tokens: Linear, un-patchify, log_softmax, one-hot, MONAI's formula."""
    logits = torch.nn.functional.linear(tokens, W, b)
    return R.loss_composed(R.unpatchify(logits, first, G, P, K), y, W_CE, W_DICE, cw)


def _vit(dtype, regs=1, **kw):
    """The tiny backbone the fine-tuning GPU tests build (tests/test_finetune_gpu.py)."""
    from headct_foundation_amd.dino_model import ViTBackbone
    return ViTBackbone(in_chans=3, img_size=24, patch_size=12, hidden_size=48, mlp_dim=96, num_layers=2, num_heads=3, num_register_tokens=regs,
                       compute_dtype=dtype, **kw)


@pytest.mark.parametrize("dtype,tol", [("fp32", 1e-3), ("bf16", 3e-2)])
def test_head_and_loss_vs_torch(lib, cuda, dtype, tol):
    """SegmentationHead + seg_loss on the tiny backbone's tokens, one step against the torch composition in float64 on the same
    tokens: head and token gradients at the bars tests/test_finetune_gpu.py holds the attentive head to (1e-3 fp32, 3e-2 bf16);
    then gradient accumulation over two backwards."""
    from headct_foundation_amd.segmentation import SegmentationHead, seg_loss
    torch.manual_seed(4)
    B, D, P, G, K, first = 3, 48, 12, 2, 3, 2
    T, S = first + G ** 3, G * P
    tdt = F32 if dtype == "fp32" else BF16
    vit = _vit(dtype).to(cuda).eval()
    with torch.no_grad():
        x = vit((torch.rand(B, 3, S, S, S) * torch.tensor([1.0, 3.0, 6.0]).view(-1, 1, 1, 1, 1)).to(cuda))[0].detach().cpu()
    assert tuple(x.shape) == (B, T, D) and x.dtype == tdt
    head = SegmentationHead(D, P, K).to(cuda).train()
    with torch.no_grad():
        head.linear.weight.mul_(4.0)  # logits of order one, so that the softmax is not flat
    y = torch.randint(0, K, (B, S, S, S)).to(torch.uint8)
    y[torch.rand(B, S, S, S) < 0.1] = 255
    cw = _class_weight(K)
    xg = x.to(cuda).requires_grad_(True)
    parts = {}
    logits = head(xg)
    assert logits.dtype == tdt and tuple(logits.shape) == (B, T, K * P ** 3)
    loss = seg_loss(logits, y.to(cuda), P, K, first, W_CE, W_DICE, cw, parts=parts)
    loss.backward()
    xr = x.to(F64).requires_grad_(True)
    Wr = head.linear.weight.detach().cpu().to(F64).requires_grad_(True)
    br = head.linear.bias.detach().cpu().to(F64).requires_grad_(True)
    lref = _composed(xr, Wr, br, y, first, G, P, K, cw.to(F64))
    lref.backward()
    lv, rv = float(loss.detach()), float(lref.detach())
    print(f"loss {lv:.6f} ref {rv:.6f}; dW {_rel(head.linear.weight.grad, Wr.grad):.2e} db {_rel(head.linear.bias.grad, br.grad):.2e} "
          f"dx {_rel(xg.grad, xr.grad):.2e}")
    assert abs(lv - rv) < tol * abs(rv)
    assert abs(float(parts["ce"]) * W_CE + float(parts["dice"]) * W_DICE - lv) < 1e-6 * max(1.0, abs(lv))
    assert _rel(head.linear.weight.grad, Wr.grad) < tol and _rel(head.linear.bias.grad, br.grad) < tol
    assert xg.grad.dtype == tdt and _rel(xg.grad, xr.grad) < tol
    assert bool((xg.grad[:, :first] == 0).all())  # the class token and the register get no gradient from the decoder
    # accumulation: a second backward at half the weight adds up; after zero_grad the next one writes the first one's bits
    one = {k: p.grad.clone() for k, p in head.named_parameters()}
    (seg_loss(head(xg), y.to(cuda), P, K, first, W_CE, W_DICE, cw) * 0.5).backward()
    for k, p in head.named_parameters():
        assert torch.allclose(p.grad, one[k] * 1.5, rtol=1e-5, atol=1e-7), k
    head.zero_grad()
    seg_loss(head(xg), y.to(cuda), P, K, first, W_CE, W_DICE, cw, inplace_grad=True).backward()
    assert all(torch.equal(p.grad, one[k]) for k, p in head.named_parameters())
    head.eval()  # eval mode: the same logits without a graph
    with torch.no_grad():
        assert torch.equal(head(xg.detach()), logits.detach())


@pytest.mark.parametrize("dtype,recipe", [("fp32", "plain"), ("bf16", "plain"), ("bf16", "drop_path_lora")])
def test_training_beats_the_constant_prediction(lib, cuda, dtype, recipe):
    """30 steps on one fixed synthetic batch: the loss ends below its first value and below the loss of the best constant prediction
    (softmax at the class prior, tests/seg_ref.py); the foreground Dice of the arg-max exceeds that prediction's.  How far it gets
    is printed, not asserted."""
    from headct_foundation_amd.data import SyntheticSegmented
    from headct_foundation_amd.metrics import SegmentationMetrics
    from headct_foundation_amd.misc import set_requires_grad_false
    from headct_foundation_amd.optim import HipAdamW, clip_grad_norm_
    from headct_foundation_amd.segmentation import SegmentationHead, seg_loss, seg_predict
    torch.manual_seed(7)
    K, P, S = 3, 12, 24
    extra = dict(lora=True, drop_path_rate=0.1) if recipe == "drop_path_lora" else {}
    vit = _vit(dtype, **extra).to(cuda)
    if recipe == "drop_path_lora":
        set_requires_grad_false(vit, lora=True)
    head = SegmentationHead(48, P, K).to(cuda)
    first = 1 + vit.num_register_tokens
    v, y, _ = SyntheticSegmented(1, 8, 3, S, K, cuda, seed=0).batches[0]
    const = R.constant_prediction(y.cpu(), K)
    opts = [HipAdamW(head, lr=1e-2, weight_decay=0.0), HipAdamW(vit, lr=1e-4, weight_decay=0.0)]
    losses = []
    vit.train()
    head.train()
    for _ in range(30):
        for o in opts:
            o.zero_grad()
        loss = seg_loss(head(vit(v)[0]), y, P, K, first, inplace_grad=True)
        loss.backward()
        clip_grad_norm_(head, 1.0)
        clip_grad_norm_(vit, 1.0)
        for o in opts:
            o.step()
        losses.append(float(loss.detach()))
    vit.eval()
    head.eval()
    with torch.no_grad():
        out = seg_predict(head(vit(v)[0]), P, K, first, labels=y)
    m = SegmentationMetrics(K)
    m(out["counts"])
    fg = float(np.nan_to_num(m.compute()["DiceGlobal"][1:]).mean())
    print(f"{dtype} {recipe}: loss {losses[0]:.4f} -> {losses[-1]:.4f}, constant prediction {const['loss']:.4f}; foreground Dice {fg:.4f} "
          f"(constant {const['fg_dice']:.4f})")
    assert losses[-1] < losses[0] and losses[-1] < const["loss"], (losses, const)
    assert fg > const["fg_dice"], (fg, const)


def test_main_segmentation_end_to_end(lib, cuda, tmp_path):
    """main_segmentation.py through torch.distributed.run in a child process: tiny ViT, synthetic data, 2 epochs, validation every
    epoch, --save_preds.  Metrics are printed, the checkpoint reloads into fresh modules, and the prediction files read back equal
    to seg_predict of the reloaded model on the test set."""
    from headct_foundation_amd.data import SyntheticSegmented
    from headct_foundation_amd.nifti import read_nifti
    from headct_foundation_amd.segmentation import SegmentationHead, seg_predict
    vit = _vit("fp32", 0)
    torch.save({"state_dict": {"module." + k: t for k, t in vit.state_dict().items()}, "epoch": 3}, tmp_path / "pre.pt")
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("MODEL:\n  NAME: vit\n")
    opts = ["DATA.SYNTHETIC", "True", "DATA.SYNTHETIC_SAMPLES", "8", "VIT.INPUT_SIZE", "24", "VIT.PATCH_SIZE", "12", "VIT.HIDDEN_SIZE", "48",
            "VIT.MLP_DIM", "96", "VIT.NUM_LAYERS", "2", "VIT.NUM_HEADS", "3", "TRAIN.VAL_EVERY", "1", "MODEL.DIR", str(tmp_path / "out"),
            "MODEL.SAVE_NAME", "seg.pt", "LOG.OUTPUT_DIR", str(tmp_path / "log"), "PREDS_SAVE_NAME", "run", "MAE.COMPUTE_DTYPE", "fp32"]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nproc-per-node", "1", "--master-port", "29617",
           os.path.join(ROOT, "main_segmentation.py"), "--cfg", str(cfg), "--model_name", "vit", "--model_load_path", str(tmp_path / "pre.pt"),
           "--seg_classes", "3", "--batch_size", "4", "--max_epochs", "2", "--grad_clip", "1.0", "--base_lr", "1e-4", "--save_preds",
           "--opts"] + opts
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-4000:]
    assert "SegDiceGlobal" in log and "SegIoUGlobal" in log and "SegDiceScan" in log and "Final test loss" in log, log[-4000:]
    ck = torch.load(tmp_path / "out" / "seg.pt", weights_only=True)
    assert ck["seg"] == {"num_classes": 3, "patch_size": 12, "dim": 48}
    vit2 = _vit("fp32", 0)
    vit2.load_state_dict(ck["state_dict"], strict=True)
    head = SegmentationHead(48, 12, 3)
    head.load_state_dict(ck["seg_head_state_dict"], strict=True)
    vit2, head = vit2.to(cuda).eval(), head.to(cuda).eval()
    test = SyntheticSegmented(1, 4, 3, 24, 3, cuda, seed=42 + 2000)  # the entry point's test loader: SEED + 2000, SAMPLES // batch // 4 batches
    files = sorted(os.listdir(tmp_path / "out" / "run_preds"))
    assert len(files) == 4, files
    with torch.no_grad():
        for v, y, names in test:
            pred = seg_predict(head(vit2(v)[0]), 12, 3, 1)["pred"].cpu().numpy()
            for b, name in enumerate(names):
                raw = read_nifti(str(tmp_path / "out" / "run_preds" / f"{name}_pred.nii.gz"))[0]
                assert np.array_equal(np.asarray(raw).astype(np.int64), pred[b].astype(np.int64)), name


# ---- real masks ---------------------------------------------------------------------------------------------------------------------
def test_label_to_item_kernel(lib, cuda):
    """Bit for bit against the numpy map: anisotropic spacing, a box that starts at a non-zero offset (and one that overhangs the
    volume, which the kernel confines); a value 300 sets the status word and reads as ignore."""
    from headct_foundation_amd import nifti
    from headct_foundation_amd.data import nearest_tables
    gen = np.random.default_rng(2)
    d, zooms = (9, 14, 11), (2.5, 0.7, 1.3)
    geom = [nifti.spacing_geometry(d[a], zooms[a]) for a in range(3)]
    m, steps = [g[0] for g in geom], [g[1] for g in geom]
    mask = gen.integers(0, 5, d).astype(np.float32)
    near_d = torch.from_numpy(nearest_tables(d, m, steps)).to(cuda)
    for roi, start, size in (((8, 6, 10), (3, 1, 2), (m[0] - 5, m[1] - 2, m[2] - 4)), ((16, 16, 16), (0, 0, 0), tuple(m)),
                             ((4, 4, 4), (2, 2, 2), (m[0], m[1], m[2]))):
        box_d = torch.tensor(list(start) + list(size) + [0, 0], dtype=torch.int32, device=cuda)
        ras_d = torch.from_numpy(mask).to(cuda)
        out, status = _Bytes(roi, torch.uint8, cuda, 77), _Bytes((1,), torch.int32, cuda, -5)
        _lib.check(lib.hct_label_to_item(ras_d.data_ptr(), *d, near_d.data_ptr(), *m, box_d.data_ptr(), out.ptr, *roi, status.ptr, _st()), "label")
        torch.cuda.synchronize()
        conf = [min(size[a], m[a] - start[a]) for a in range(3)]
        want = R.label_item(mask, m, steps, start, conf, roi)
        assert np.array_equal(out.result().numpy(), want) and int(status.result()[0]) == 0
    bad = mask.copy()
    rows = R.nearest_axis(d[0], m[0], steps[0])[R.cell_centres(3, m[0] - 5, 8)]  # the mask row each output row of axis 0 shows
    bad[rows[0], :, :] = 300.0
    box_d = torch.tensor([3, 1, 2, m[0] - 5, m[1] - 2, m[2] - 4, 0, 0], dtype=torch.int32, device=cuda)
    out, status = _Bytes((8, 6, 10), torch.uint8, cuda, 77), _Bytes((1,), torch.int32, cuda, -5)
    bad_d = torch.from_numpy(bad).to(cuda)
    _lib.check(lib.hct_label_to_item(bad_d.data_ptr(), *d, near_d.data_ptr(), *m, box_d.data_ptr(), out.ptr, *(8, 6, 10), status.ptr, _st()), "label")
    torch.cuda.synchronize()
    got = out.result()
    hit = torch.from_numpy(rows == rows[0])
    want = torch.from_numpy(R.label_item(mask, m, steps, (3, 1, 2), (m[0] - 5, m[1] - 2, m[2] - 4), (8, 6, 10)))
    assert int(status.result()[0]) == 2 and bool((got[hit] == 255).all()) and torch.equal(got[~hit], want[~hit])


def _write_pair(tmp_path, tag, shape_ijk, affine, seed, bad_value=False):
    """An image (HU-like values, positive inside a box, air outside) and a mask of blocks 0 .. 2 on the same grid."""
    from headct_foundation_amd.nifti import write_nifti
    gen = np.random.default_rng(seed)
    ni, nj, nk = shape_ijk
    img = np.full((nk, nj, ni), -1000.0, np.float32)  # air around the head: the cubic resampling's ringing stays below 0 away from it
    img[2:nk - 2, 3:nj - 2, 2:ni - 3] = gen.uniform(20.0, 80.0, (nk - 4, nj - 5, ni - 5)).astype(np.float32)
    mask = np.zeros((nk, nj, ni), np.int16)
    mask[3:nk // 2, 4:nj - 4, 3:ni // 2] = 1
    mask[nk // 2:nk - 3, 5:nj // 2, ni // 2:ni - 4] = 2
    if bad_value:
        mask[nk // 2, nj // 2, ni // 2] = 300
    ip, sp = tmp_path / f"{tag}.nii.gz", tmp_path / f"{tag}_seg.nii.gz"
    write_nifti(ip, img, affine, dtype="f4")
    write_nifti(sp, mask, affine, dtype="i2")
    return str(ip), str(sp), mask


def _expected_labels(img_path, mask, roi, cuda):
    """The numpy map of the mask through the image's geometry; the box is the one the image's own loading chain finds."""
    from headct_foundation_amd.data import DecodedVolume, run_loading_chain
    dec = DecodedVolume(img_path)
    with torch.cuda.device(cuda):
        _, box = run_loading_chain(dec, dec.host.to(cuda), roi, 3)
    box = box.cpu().numpy()
    assert int(box[6]) == 0
    ras = np.transpose(np.transpose(mask, (2, 1, 0)), dec.perm)  # file order [k, j, i] -> axes (i, j, k) -> RAS axis o = file axis perm[o]
    for o in range(3):
        if dec.flip[o]:
            ras = np.flip(ras, axis=o)
    return R.label_item(np.ascontiguousarray(ras), dec.m, dec.steps, box[:3], box[3:6], roi), box


def test_real_mask_loaders(lib, cuda, tmp_path):
    """Two small NIfTI image / mask pairs written into tmp_path, one of them anisotropic and not RAS, plus a row whose files do not
    exist: the loaders' labels equal the numpy map, the training loader flips volumes and labels alike, a mask of another grid or
    with a value 300 is refused."""
    from headct_foundation_amd.data import (DeviceAugment, LabelCache, SegmentedVolumes, VolumeCache, load_segmentation_pair, read_segmentation_paths)
    roi = (16, 16, 16)
    aff_a = np.eye(4)
    aff_b = np.array([[0.0, 1.5, 0.0, -10.0], [-0.8, 0.0, 0.0, 12.0], [0.0, 0.0, 2.0, 5.0], [0.0, 0.0, 0.0, 1.0]])  # i -> -y, j -> +x: not RAS, anisotropic
    ia, sa, ma = _write_pair(tmp_path, "a", (20, 18, 14), aff_a, 0)
    ib, sb, mb = _write_pair(tmp_path, "b", (24, 14, 10), aff_b, 1)
    csv = tmp_path / "pairs.csv"
    csv.write_text("img_path,seg_path\n" + f"{ia},{sa}\n{ib},{sb}\n{tmp_path}/missing.nii.gz,{tmp_path}/missing_seg.nii.gz\n")
    pairs = read_segmentation_paths(csv)
    want = [_expected_labels(ia, ma, roi, cuda), _expected_labels(ib, mb, roi, cuda)]
    assert any(int(b[k]) > 0 for _, b in want for k in range(3))  # a foreground box that starts at a non-zero offset
    for w, _ in want:
        assert set(np.unique(w)) == {0, 1, 2}
    vc, lc = VolumeCache(tmp_path / "cache", roi, 3), LabelCache(tmp_path / "cache", roi, 3)
    val = SegmentedVolumes(pairs, [0, 1, 2], vc, lc, 3, cuda, None, 2)
    (vol, lab, names), = list(val)
    assert vol.dtype == F32 and tuple(vol.shape) == (3, 3, 16, 16, 16) and lab.dtype == torch.uint8 and names[2] == "None" and names[:2] == [ia, ib]
    for b in range(2):
        assert np.array_equal(lab[b].cpu().numpy(), want[b][0]), b
        assert torch.equal(vol[b], vc.get(pairs[b][0], cuda).float())
    assert bool((lab[2] == 255).all()) and bool((vol[2] == 0).all())
    assert os.path.exists(lc.file_of(ia, sa)) and torch.equal(lc.get(ia, sa, cuda).cpu(), lab[0].cpu())  # the second read comes from the cache file
    train = SegmentedVolumes(pairs, [1, 0, 1, 0], vc, lc, 4, cuda, DeviceAugment(flip_prob=0.5, shift_offsets=0.0, shift_prob=0.0, seed=3), 2)
    (tv, tl, _), = list(train)
    flip = train.last_flip
    assert int(flip.max()) > 0
    base = torch.stack([torch.from_numpy(want[i][0]) for i in (1, 0, 1, 0)])
    assert torch.equal(tl.cpu(), R.flip_labels(base, range(4), flip))
    vbase = torch.stack([vc.get(pairs[i][0], cuda).float().cpu() for i in (1, 0, 1, 0)])
    for b in range(4):
        dims = [1 + a for a in range(3) if int(flip[b]) >> a & 1]
        assert torch.equal(tv[b].cpu(), torch.flip(vbase[b], dims) if dims else vbase[b])
    # refusals
    ic, sc, _ = _write_pair(tmp_path, "c", (20, 18, 14), aff_a, 2, bad_value=True)
    with pytest.raises(ValueError, match="no integer"):
        load_segmentation_pair(ic, sc, roi, 3, cuda)
    with pytest.raises(ValueError, match="shape"):
        load_segmentation_pair(ia, sb, roi, 3, cuda)
    shifted = aff_a.copy()
    shifted[0, 3] = 0.5
    _, sd, _ = _write_pair(tmp_path, "d", (20, 18, 14), shifted, 0)
    with pytest.raises(ValueError, match="affine"):
        load_segmentation_pair(ia, sd, roi, 3, cuda)
