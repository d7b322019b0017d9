"""GPU: multi-label fine-tuning (TRAIN.LABEL_NAMES).  hct_sigmoid_bce through the C ABI against torch's float64
binary_cross_entropy_with_logits (tests/multilabel_ref.py), the autograd function over it, training through
engine_downstream.train_one_epoch with both heads and with TRAIN.LOCK, and main_downstream.py end to end.

Bars (tests/multilabel_ref.FP32_BAR = 1e-5, the project's fp32 bar for composite kernels): |loss - ref| <= 1e-5 |ref|, the same per
label for label_loss, and for the gradient |got - ref| n / (g max(1, w_t)) <= 1e-5 per element -- the error in units of the
unscaled per-element derivative, which lies in [-w, 1]; a relative bar is meaningless where the true gradient underflows.
Missing entries are bit-equal to 0.  One allowance from the output format: a lone +100 logit with target 1 (the issue's inputs at
B = 1, and at B = T = 1 the loss itself) has the loss term w log1p(exp(-100)) = w 3.7e-44, below fp32's smallest normal number
2^-126 = 1.2e-38, where a float carries 5 bits, not 24 (the kernel returns 3.78e-44 for 3.72e-44: 1.7e-2 relative, the nearest
subnormal), or none where subnormals are flushed.  The two loss bars therefore read |got - ref| <= 1e-5 |ref| + 2^-126: the bar as
stated for every reference an fp32 output can hold.  Measured on an MI355X: loss within 1.1e-7, label_loss within 1.5e-7 of the float64
reference wherever it is a normal number, the gradient within 2.2e-7 of the per-element derivative; at 1 x 1 the loss is 3.783506e-44 for 3.720076e-44.  Outputs are NaN-filled inside guard bands that must come back untouched, and every call is
made twice and must agree bit for bit."""
import os
import pickle
import subprocess
import sys

import pytest
import torch

from tests import multilabel_ref as R
from tests.test_assembly_kernels_gpu import _Out, _p, _st, _twice

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = torch.float32
TINY = 2.0 ** -126  # fp32's smallest normal number: the absolute floor of the two loss bars (module docstring)


def _call(lib, xd, yd, wd, gd, want=("loss", "label_loss", "dlogits")):
    """One hct_sigmoid_bce call into fresh guarded outputs; the workspace is NaN-filled: nothing in it may be read before written."""
    B, T = xd.shape
    outs = {}
    if "loss" in want:
        outs["loss"] = _Out((1,), F32, xd.device)
    if "label_loss" in want:
        outs["label_loss"] = _Out((T,), F32, xd.device)
    if "dlogits" in want:
        outs["dlogits"] = _Out((B, T), F32, xd.device)
    need = lib.hct_sigmoid_bce_workspace_bytes(B, T)
    assert need == R.workspace_bytes(B, T)
    ws = torch.full(((need + 3) // 4,), float("nan"), dtype=F32, device=xd.device)
    rc = lib.hct_sigmoid_bce(xd.data_ptr(), yd.data_ptr(), _p(wd), B, T, _p(gd), _p(outs.get("loss")), _p(outs.get("label_loss")),
                             _p(outs.get("dlogits")), ws.data_ptr(), need, _st())
    assert rc == 0, lib.hct_last_error_string()
    return outs


def _check(res, x, y, w, g, what):
    loss, label_loss, grad, n = R.reference(x, y, w, 1.0 if g is None else g)
    gv = 1.0 if g is None else g
    if "loss" in res:
        got = float(res["loss"][0])
        err = abs(got - float(loss))
        print(f"{what}: loss {got:.7g} ref {float(loss):.7g} rel err {err / max(abs(float(loss)), 1e-300):.2e}")
        assert err <= R.FP32_BAR * abs(float(loss)) + TINY, (what, got, float(loss))
    if "label_loss" in res:
        err = (res["label_loss"].double() - label_loss).abs()
        normal = label_loss.abs() >= TINY
        rel = float((err[normal] / label_loss[normal].abs()).max()) if bool(normal.any()) else 0.0
        print(f"{what}: label_loss max rel err {rel:.2e} over {int(normal.sum())} labels, {int((~normal & (label_loss != 0)).sum())} below 2^-126")
        assert bool((err <= R.FP32_BAR * label_loss.abs() + TINY).all()), (what, rel)
    if "dlogits" in res:
        got = res["dlogits"]
        assert not bool(torch.isnan(got).any()), what
        missing = ~(y >= 0)
        assert bool((got[missing].view(torch.int32) == 0).all()), (what, "a missing entry's gradient is not +0.0")
        wt = torch.ones(y.shape[1], dtype=torch.float64) if w is None else w.double().clamp(min=1)
        units = (got.double() - grad).abs() * max(n, 1) / (gv * wt)
        print(f"{what}: gradient max err {float(units.max()):.2e} in units of the per-element derivative, n = {n}")
        assert float(units.max()) <= R.FP32_BAR, (what, float(units.max()))


@pytest.mark.parametrize("B,T", R.CASES)
def test_sigmoid_bce_vs_float64(lib, cuda, B, T):
    x, y, w = R.inputs(B, T)
    xd, yd, wd = x.to(cuda), y.to(cuda), w.to(cuda)
    gd = torch.tensor([R.DLOSS], dtype=F32, device=cuda)
    for use_w in (True, False):
        for use_g in (True, False):
            res = _twice(lambda: _call(lib, xd, yd, wd if use_w else None, gd if use_g else None))
            _check(res, x, y, w if use_w else None, R.DLOSS if use_g else None, f"{B}x{T} pos_weight={use_w} dloss={use_g}")


def test_sigmoid_bce_missing_column_and_nothing_valid(lib, cuda):
    B, T = R.EXTRA_SHAPE
    x, y, w = R.inputs(B, T)
    xd, wd = x.to(cuda), w.to(cuda)
    full = _twice(lambda: _call(lib, xd, y.to(cuda), wd, None))
    y1 = y.clone()
    y1[:, 5] = -1.0  # one column entirely missing: its label_loss is 0, the others are unaffected
    res = _twice(lambda: _call(lib, xd, y1.to(cuda), wd, None))
    _check(res, x, y1, w, None, "column 5 missing")
    assert float(res["label_loss"][5]) == 0.0 and not bool(res["dlogits"][:, 5].any())
    keep = [t for t in range(T) if t != 5]
    assert torch.equal(res["label_loss"][keep], full["label_loss"][keep])
    y0 = -torch.ones_like(y)  # everything missing: loss 0, all gradients 0, nothing NaN
    res = _twice(lambda: _call(lib, xd, y0.to(cuda), wd, None))
    for k in ("loss", "label_loss", "dlogits"):
        assert bool((res[k].view(torch.int32) == 0).all()), k
    y0[3, 2] = float("nan")  # a NaN target is a missing entry too
    res = _twice(lambda: _call(lib, xd, y0.to(cuda), wd, None))
    assert all(bool((res[k].view(torch.int32) == 0).all()) for k in ("loss", "label_loss", "dlogits"))


def test_sigmoid_bce_soft_labels(lib, cuda):
    B, T = R.EXTRA_SHAPE
    x, y, w = R.inputs(B, T)
    ys = torch.where(y < 0, y, 0.1 + 0.8 * y)  # 0.1 / 0.9
    for wv in (w, None):
        res = _twice(lambda: _call(lib, x.to(cuda), ys.to(cuda), None if wv is None else wv.to(cuda), None))
        _check(res, x, ys, wv, None, f"soft labels pos_weight={wv is not None}")


@pytest.mark.parametrize("absent", ["loss", "label_loss", "dlogits"])
def test_sigmoid_bce_null_outputs(lib, cuda, absent):
    """Each output NULL in turn: the others are what the full call gives, bit for bit."""
    B, T = R.EXTRA_SHAPE
    x, y, w = R.inputs(B, T)
    xd, yd, wd = x.to(cuda), y.to(cuda), w.to(cuda)
    gd = torch.tensor([R.DLOSS], dtype=F32, device=cuda)
    full = _twice(lambda: _call(lib, xd, yd, wd, gd))
    want = tuple(k for k in ("loss", "label_loss", "dlogits") if k != absent)
    res = _twice(lambda: _call(lib, xd, yd, wd, gd, want))
    assert set(res) == set(want)
    for k in want:
        assert torch.equal(res[k].view(torch.int32), full[k].view(torch.int32)), k
    only = _twice(lambda: _call(lib, xd, yd, wd, gd, (absent,)))
    assert torch.equal(only[absent].view(torch.int32), full[absent].view(torch.int32))


def test_sigmoid_bce_refusals_touch_nothing(lib, cuda):
    B, T = R.EXTRA_SHAPE
    x, y, _ = R.inputs(B, T)
    xd, yd = x.to(cuda), y.to(cuda)
    need = lib.hct_sigmoid_bce_workspace_bytes(B, T)
    ws = torch.empty(need, dtype=torch.uint8, device=cuda)
    outs = dict(loss=_Out((1,), F32, cuda), label_loss=_Out((T,), F32, cuda), dlogits=_Out((B, T), F32, cuda))
    ptrs = [_p(outs[k]) for k in ("loss", "label_loss", "dlogits")]
    assert lib.hct_sigmoid_bce(xd.data_ptr(), yd.data_ptr(), None, B, T, None, *ptrs, ws.data_ptr(), need - 1, _st()) == -3
    assert b"hct_sigmoid_bce" in lib.hct_last_error_string()
    assert lib.hct_sigmoid_bce(xd.data_ptr(), yd.data_ptr(), None, 0, T, None, *ptrs, ws.data_ptr(), need, _st()) == -1
    assert b"hct_sigmoid_bce" in lib.hct_last_error_string()
    torch.cuda.synchronize()
    for o in outs.values():
        o.result()
        assert o.untouched()


# ---- 2. the autograd function ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_w", [True, False])
def test_bce_with_logits_autograd(lib, cuda, use_w):
    from headct_foundation_amd import HctError, bce_with_logits
    B, T = R.EXTRA_SHAPE
    x, y, w = R.inputs(B, T)
    wv = w if use_w else None
    xd, yd, wd = x.to(cuda), y.to(cuda), (w.to(cuda) if use_w else None)
    kernel = _twice(lambda: _call(lib, xd, yd, wd, None))
    leaf = xd.clone().requires_grad_(True)
    loss = bce_with_logits(leaf, yd, wd)
    loss.backward()
    assert loss.shape == () and torch.equal(loss.detach().cpu().view(1), kernel["loss"])
    assert torch.equal(leaf.grad.cpu().view(torch.int32), kernel["dlogits"].view(torch.int32))
    _check({"loss": loss.detach().cpu().view(1), "dlogits": leaf.grad.cpu()}, x, y, wv, None, f"autograd pos_weight={use_w}")
    one = leaf.grad.clone()
    leaf.grad = None
    (3 * bce_with_logits(leaf, yd, wd)).backward()  # a scaled loss scales the gradient: within one ulp of 3 x
    ulp = torch.abs(torch.nextafter(3 * one, torch.full_like(one, float("inf"))) - 3 * one)
    assert bool(((leaf.grad - 3 * one).abs() <= ulp).all()) and bool((leaf.grad[yd < 0] == 0).all())
    with pytest.raises(HctError, match="differs from the logits"):
        bce_with_logits(leaf, yd[:, :-1], None)
    with pytest.raises(HctError, match="no CPU fallback"):
        bce_with_logits(x, y, None)


# ---- 3. training ------------------------------------------------------------------------------------------------------------------------
EPOCHS = 30  # the steps of tests/test_finetune_gpu.py's _loop


def _train(cuda, lock, head):
    import config as cfgmod
    from engine_downstream import train_one_epoch, val_one_epoch
    from headct_foundation_amd import AttentionClassifier, LinearClassifier, bce_with_logits
    from headct_foundation_amd.data import SyntheticMultiLabelled
    from headct_foundation_amd.dino_model import ViTBackbone
    from headct_foundation_amd.metrics import MultilabelMetrics
    from headct_foundation_amd.optim import HipAdamW
    names = ["a", "b", "c"]
    cfg = cfgmod._C.clone()
    cfg.MODEL.NAME, cfg.TRAIN.LOCK, cfg.TRAIN.GRAD_CLIP, cfg.TRAIN.LABEL_NAMES = "vit", lock, 1.0, names
    torch.manual_seed(5)
    vit = ViTBackbone(in_chans=3, img_size=24, patch_size=12, hidden_size=48, mlp_dim=96, num_layers=2, num_heads=3, num_register_tokens=0,
                      compute_dtype="bf16").to(cuda)
    cls = (LinearClassifier(48, 3, feature_grad=not lock) if head == "linear" else
           AttentionClassifier(48, 3, num_heads=12, compute_dtype="bf16")).to(cuda).train()
    if lock:
        for p in vit.parameters():
            p.requires_grad_(False)
    opts = [HipAdamW(cls, lr=1e-3, weight_decay=0.04)] + ([] if lock else [HipAdamW(vit, lr=1e-5, weight_decay=0.04)])
    train = SyntheticMultiLabelled(2, 4, 3, 24, 3, cuda, seed=0)
    val = SyntheticMultiLabelled(4, 4, 3, 24, 3, cuda, seed=1000)
    before = vit._flat.clone()
    metrics = MultilabelMetrics(names)
    losses = [train_one_epoch(cfg, vit, cls, train, opts, [], bce_with_logits, e, EPOCHS, metrics, device=cuda)["loss"] for e in range(EPOCHS)]
    vm = MultilabelMetrics(names)
    val_loss = val_one_epoch(cfg, vit, cls, val, 0, 1, vm, bce_with_logits, device=cuda)["loss"]
    out = vm.compute()
    print(f"multi-label training head={head} lock={lock}: loss {losses[0]:.4f} -> {losses[-1]:.4f} (x{losses[-1] / losses[0]:.3f}) in {EPOCHS} epochs, "
          f"validation loss {val_loss:.4f}, AUROC {out['MultilabelAUROC'].tolist()}, AP {out['MultilabelAveragePrecision'].tolist()}")
    return losses, before, vit


@pytest.mark.parametrize("head", ["linear", "attentive"])
def test_multilabel_training_loss_falls(lib, cuda, head):
    losses, before, vit = _train(cuda, False, head)
    assert losses[-1] < losses[0], losses
    assert not torch.equal(before, vit._flat)


def test_multilabel_lock_keeps_backbone_bit_unchanged(lib, cuda):
    losses, before, vit = _train(cuda, True, "linear")
    assert torch.equal(before, vit._flat)
    assert losses[-1] < losses[0], losses


# ---- 4. main_downstream.py end to end ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("head,port", [("linear", "29621"), ("attentive", "29622")])
def test_main_downstream_multilabel_run(lib, cuda, tmp_path, head, port):
    from headct_foundation_amd.classifier import AttentionClassifier, LinearClassifier
    from headct_foundation_amd.dino_model import ViTBackbone
    vit = ViTBackbone(in_chans=3, img_size=24, patch_size=12, hidden_size=48, mlp_dim=96, num_layers=2, num_heads=3, compute_dtype="fp32")
    torch.save({"state_dict": {"module." + k: v for k, v in vit.state_dict().items()}, "epoch": 3}, tmp_path / "pre.pt")
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("MODEL:\n  NAME: vit\n")
    opts = ["DATA.SYNTHETIC", "True", "DATA.SYNTHETIC_SAMPLES", "8", "VIT.INPUT_SIZE", "24", "VIT.PATCH_SIZE", "12",
            "VIT.HIDDEN_SIZE", "48", "VIT.MLP_DIM", "96", "VIT.NUM_LAYERS", "2", "VIT.NUM_HEADS", "3", "TRAIN.VAL_EVERY", "1",
            "MODEL.DIR", str(tmp_path / "out"), "MODEL.SAVE_NAME", "ft.pt", "LOG.OUTPUT_DIR", str(tmp_path / "log"),
            "PREDS_SAVE_NAME", "run"]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nproc-per-node", "1", "--master-port", port,
           os.path.join(ROOT, "main_downstream.py"), "--cfg", str(cfg), "--model_name", "vit", "--model_load_path", str(tmp_path / "pre.pt"),
           "--classifier", head, "--batch_size", "4", "--max_epochs", "2", "--grad_clip", "1.0", "--base_lr", "1e-4",
           "--label_names", "a", "b", "c", "--opts"] + opts
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-4000:]
    assert "MultilabelAUROC" in log and "Final test loss" in log, log[-4000:]
    c = torch.load(tmp_path / "out" / "ft_classifier.pt", weights_only=True)
    fresh = LinearClassifier(48, 3) if head == "linear" else AttentionClassifier(48, 3, num_heads=12)
    fresh.load_state_dict(c["state_dict"], strict=True)
    with open(tmp_path / "out" / "run_preds.pkl", "rb") as f:
        preds = pickle.load(f)
    assert set(preds) == {"fnames", "preds", "targets", "label_names"} and preds["label_names"] == ["a", "b", "c"]
    N = len(preds["fnames"])
    assert N > 0 and preds["preds"].shape == preds["targets"].shape == (N, 3)
    assert float(preds["preds"].min()) >= 0.0 and float(preds["preds"].max()) <= 1.0
    assert set(preds["targets"].flatten().tolist()) <= {-1.0, 0.0, 1.0}  # -1: the synthetic table's missing entries
