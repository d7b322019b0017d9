"""GPU: the DINO step held per row and per column to its restatement in float64 (tests/dino_step_ref.py).

Student and teacher are MultiCropWrapper(ViTBackbone, DINOHead) pairs with the case's parameters; the step is the engine's own
(engine_pretrain_dino._forward_loss, backward(), cancel_gradients_last_layer) with DINOLoss, IBOTPatchLoss and an IBotObjective wired as
main_pretrain_dino.py wires them, the objective's generator returning the case's explicit masks.  Held to E(device, reference) <= M * Y
per tensor (E the worst slice over rows and columns, Y the reference side's own distance, M = dino_step_ref.M32_DINO / MBF_DINO): the
loss and each of its parts, every gradient, the centres after the step, the BatchNorm running statistics, and in fp32 the logits rows
and the class-token rows.  The mathematically-zero gradients under BatchNorm are held absolutely (dino_step_ref.zero_bias_bounds); under
Sinkhorn-Knopp the centres must not move by a bit.  The set of gradient names must be the reference's, frozen tensors have none.

Cases: `small` (the fixture's backbone, 8 head rows), `tile16` (hidden 768, head 2048 / 256 / 4100, 16 head rows: the split-K dgrad of
the prototype layer in bf16) and `tile15` (15 rows: the NT fallback).  Settings: plain with the last layer frozen and trained, BatchNorm
heads, Sinkhorn-Knopp, iBOT in both centering forms on both mask variants (class rows + masked rows a multiple of 16 or not), KoLeo,
and Sinkhorn-Knopp + iBOT + KoLeo with the last layer trained.

Measured on an MI355X, worst E / Y per case, mode and setting (DINO_ROWS lines; the tensor in brackets):
    fp32        gradients | loss and parts | centres, running statistics | logits, class-token rows (| share of the zero tensors' bounds)
      small  plain / trained   2.47 (blocks.0.att_norm.bias) | 2.34 | 1.00 | 0.92
      small  bn                2.46 (blocks.0.attn.qkv.bias) | 1.12 | 1.58 | 1.35 | 0.08
      small  sk                1.61 (blocks.1.ffn_norm.weight) | 3.75 | - | 0.92
      small  ibot-ragged       1.89 (blocks.1.attn.qkv.bias) | 1.13 | 0.92 | 1.55
      small  ibot-exact        1.96 (head.mlp.4.bias) | 2.26 | 0.88 | 1.19
      small  ibot-sk-ragged    2.20 (mask_token) | 1.05 | - | 1.55
      small  ibot-sk-exact     1.34 (norm.weight) | 1.45 | - | 1.19
      small  koleo             2.43 (blocks.0.att_norm.bias) | 2.51 | 1.00 | 0.92
      small  v2 trained        1.70 (mask_token) | 1.05 | - | 1.55
      tile16 plain / trained   1.52 (blocks.0.mlp.linear2.bias) | 0.72 | 1.07 | 1.30
      tile16 bn                2.22 (register_tokens) | 1.48 | 1.63 | 1.18 | 0.10
      tile16 sk                2.88 (blocks.0.mlp.linear1.bias) | 1.45 | - | 1.30
      tile16 ibot-ragged       1.75 (blocks.0.attn.qkv.weight) | 0.74 | 1.05 | 1.42
      tile16 ibot-exact        1.34 (mask_token) | 0.72 | 1.00 | 1.39
      tile16 ibot-sk-ragged    2.76 (norm.weight) | 2.75 | - | 1.42
      tile16 ibot-sk-exact     2.34 (norm.weight) | 2.92 | - | 1.39
      tile16 koleo             1.68 (blocks.0.ffn_norm.weight) | 0.78 | 1.07 | 1.30
      tile16 v2 trained        1.74 (head.mlp.4.bias) | 2.75 | - | 1.42
      tile15 plain / trained   2.26 (blocks.0.ffn_norm.weight) | 1.60 | 0.95 | 1.36
      tile15 bn                2.51 (blocks.0.mlp.linear2.bias) | 0.30 | 2.14 | 1.30 | 0.09
      tile15 sk                2.27 (head.mlp.4.bias) | 4.03 | - | 1.36
      tile15 ibot-ragged       2.27 (norm.weight) | 0.76 | 1.00 | 1.47
      tile15 ibot-exact        1.98 (mask_token) | 0.78 | 1.01 | 1.47
      tile15 ibot-sk-ragged    2.61 (register_tokens) | 10.18 (loss:dino) | - | 1.47
      tile15 ibot-sk-exact     2.35 (patch_embeddings.bias) | 5.29 | - | 1.47
      tile15 koleo             2.19 (register_tokens) | 1.74 | 0.95 | 1.36
      tile15 v2 trained        1.93 (blocks.0.ffn_norm.bias) | 10.18 (loss:dino) | - | 1.47
    bf16        gradients | loss and parts | centres, running statistics (| share of the zero tensors' bounds)
      small  plain / trained   3.34 (blocks.0.attn.qkv.bias) | 1.01 | 0.57
      small  bn                1.36 (blocks.1.attn.proj.bias) | 0.01 | 1.18 | 0.11
      small  sk                1.38 (head.mlp.0.bias) | 0.87 | -
      small  ibot-ragged       1.15 (register_tokens) | 2.77 | 0.62
      small  ibot-exact        1.43 (norm.bias) | 0.90 | 0.65
      small  ibot-sk-ragged    1.84 (patch_embeddings.bias) | 1.09 | -
      small  ibot-sk-exact     2.34 (norm.weight) | 0.59 | -
      small  koleo             2.69 (blocks.0.attn.qkv.bias) | 3.25 (loss:koleo) | 0.57
      small  v2 trained        1.75 (blocks.1.attn.qkv.bias) | 1.09 | -
      tile16 plain / trained   0.81 (norm.weight; trained: head.last_layer.weight_v) | 0.07 | 0.41
      tile16 bn                1.20 (blocks.0.attn.proj.bias) | 0.26 | 0.67 | 0.12
      tile16 sk                1.01 (blocks.0.mlp.linear2.bias) | 0.32 | -
      tile16 ibot-ragged       0.83 (position_embeddings) | 0.92 | 0.54
      tile16 ibot-exact        0.82 (position_embeddings) | 0.79 | 0.54
      tile16 ibot-sk-ragged    0.90 (blocks.0.attn.qkv.weight) | 0.69 | -
      tile16 ibot-sk-exact     0.83 (head.mlp.0.bias) | 0.78 | -
      tile16 koleo             0.69 (blocks.0.ffn_norm.weight) | 0.49 | 0.41
      tile16 v2 trained        0.94 (blocks.0.ffn_norm.weight) | 0.69 | -
      tile15 plain / trained   1.02 (blocks.0.attn.qkv.weight) | 0.02 | 0.52
      tile15 bn                1.43 (blocks.0.mlp.linear2.bias) | 0.17 | 0.78 | 0.14
      tile15 sk                0.92 (blocks.0.mlp.linear2.weight) | 0.50 | -
      tile15 ibot-ragged       1.08 (position_embeddings) | 1.57 | 0.39
      tile15 ibot-exact        1.11 (position_embeddings) | 0.53 | 0.37
      tile15 ibot-sk-ragged    0.90 (patch_embeddings.bias) | 2.99 (loss:ibot) | -
      tile15 ibot-sk-exact     0.82 (register_tokens) | 0.50 | -
      tile15 koleo             0.79 (blocks.0.attn.qkv.weight) | 0.18 | 0.52
      tile15 v2 trained        0.89 (blocks.0.attn.qkv.bias) | 2.99 (loss:ibot) | -
M32_DINO = 32: the next power of two at or above twice the worst fp32 ratio, 10.18 -- a scalar, the DINO term of `tile15` under
Sinkhorn-Knopp + iBOT, 3.4e-7 from the reference where its yardstick is 3.3e-8; the tensors peak at 2.88.  MBF_DINO = 4, its cap: the
worst bf16 ratio is 3.34 (`small`, whose backward the device rounds at more sites than the emulation does); the two tile cases stay
within 1.43.  The scalars' yardsticks carry the sites that dino_step_ref.py's docstring lists under "Scalars": with the single draws
alone the same device figures stood at up to 95 (fp32) and 58 (bf16) x the yardstick while every gradient of those runs lay within 2.9
and 1.1.  No slice stood out from its siblings: nothing to fix was found in the device code.
"""
import pytest
import torch

from tests import dino_step_ref as R

pytestmark = pytest.mark.gpu

# (setting of dino_step_ref.SETTINGS, last layer frozen)
RUNS = [("plain", True), ("plain", False), ("bn", True), ("sk", True), ("ibot-ragged", True), ("ibot-exact", True), ("ibot-sk-ragged", True),
        ("ibot-sk-exact", True), ("koleo", True), ("v2", False)]


def _pair(ref, pb, ph, mode, device, return_cls):
    from headct_foundation_amd.dino_model import DINOHead, MultiCropWrapper, ViTBackbone
    ibot = ref.ibot_weight > 0
    b = ViTBackbone(**ref.vit, compute_dtype=mode, mask_token=ibot)
    assert {k: tuple(v.shape) for k, v in b.state_dict().items()} == R.backbone_shapes(ref.vit, ibot)
    b.load_state_dict(pb, strict=True)
    h = DINOHead(ref.vit["hidden_size"], ref.head["out_dim"], use_bn=ref.use_bn, norm_last_layer=True, hidden_dim=ref.head["hidden_dim"],
                 bottleneck_dim=ref.head["bottleneck_dim"], compute_dtype=mode)
    assert list(h.state_dict().keys()) == list(ph.keys())
    h.load_state_dict(ph, strict=True)
    return MultiCropWrapper(b, h, return_cls=return_cls).to(device).train()


def _device_step(ref, mode, device):
    """One step of the engine on the device: ({name: tensor} as DinoRef.flat names them, the zero tensors' gradients, the modules)."""
    import engine_pretrain_dino as eng
    from headct_foundation_amd.dino import DINOLoss
    from headct_foundation_amd.ibot import IBotObjective, IBOTPatchLoss
    K, B, V = ref.head["out_dim"], ref.B, ref.V
    student = _pair(ref, ref.sb, ref.sh, mode, device, ref.koleo_weight > 0)
    teacher = _pair(ref, ref.tb, ref.th, mode, device, False)
    for p in teacher.parameters():
        p.requires_grad = False
    crit = DINOLoss(K, V, 0.04, 0.07, 3, 10, centering=ref.centering, sk_iters=R.SK_ITERS).to(device)
    crit.center.copy_(ref.center0)
    ibot = None
    if ref.ibot_weight > 0:
        patch_loss = IBOTPatchLoss(K, 0.04, 0.07, 3, 10, centering=ref.centering, sk_iters=R.SK_ITERS).to(device)
        patch_loss.center.copy_(ref.ibot_center0)

        def generator(n_g):
            assert n_g == 2 * B
            return ref.masks

        crit.ibot = ibot = IBotObjective(ref.ibot_weight, generator, patch_loss, ref.vit["num_register_tokens"])
    seen = {}
    hooks = [student.register_forward_hook(lambda m, i, o: seen.update(o)),
             student.backbone.register_forward_hook(lambda m, i, o: seen.update(tokens=o[0]))]
    parts = {}
    epoch = 0
    assert float(crit.teacher_temp_schedule[epoch]) == R.TEACHER_TEMP and crit.student_temp == R.STUDENT_TEMP and crit.center_momentum == R.CENTER_MOMENTUM
    loss = eng._forward_loss(student, teacher, ref.crops, crit, epoch, device, ref.koleo_weight, parts, ibot)
    for h in hooks:
        h.remove()
    loss.backward()
    eng.cancel_gradients_last_layer(epoch, student, 1 if ref.freeze_last_layer else 0)
    torch.cuda.synchronize()
    f = lambda t: t.detach().float().cpu()
    got = {"loss": f(loss), "loss:dino": f(parts.get("dino_loss", loss))}
    if ibot is not None:
        got["loss:ibot"] = f(parts["ibot_loss"])
    if ref.koleo_weight > 0:
        got["loss:koleo"] = f(parts["koleo_loss"])
    assert set(parts) == ({"dino_loss"} if len(got) > 2 else set()) | {k.replace("loss:", "") + "_loss" for k in got if k not in ("loss", "loss:dino")}
    grads = {"backbone." + n: f(p.grad) for n, p in student.backbone.named_parameters() if p.grad is not None}
    grads.update({"head." + n: f(p.grad) for n, p in student.head.named_parameters() if p.grad is not None})
    assert set(grads) == set(ref.grad_names()), set(grads) ^ set(ref.grad_names())
    assert student.head.last_layer.weight_g.grad is None and (student.head.last_layer.weight_v.grad is None) == ref.freeze_last_layer
    assert all(p.grad is None for p in teacher.parameters())
    zero = {k: grads.pop(k) for k in ref.zero_names()}
    got.update(grads)
    centres = {"center": f(crit.center)}
    if ibot is not None:
        centres["ibot_center"] = f(ibot.loss.center)
    if ref.centering == "centering":
        got.update({"centre:" + k: v for k, v in centres.items()})
    else:
        assert torch.equal(centres["center"], ref.center0) and (ibot is None or torch.equal(centres["ibot_center"], ref.ibot_center0)), \
            "Sinkhorn-Knopp leaves the centres alone"
    sd = student.head.state_dict()
    got.update({"stat:head." + k: f(v) for k, v in sd.items() if "running" in k})
    assert all(int(v) == 1 for k, v in sd.items() if k.endswith("num_batches_tracked"))
    if mode == "fp32":
        got["act:logits"], got["act:cls_tokens"] = f(seen["dino_output"]), f(seen["tokens"][:, 0, :])
        if ibot is not None:
            got["act:ibot_logits"] = f(seen["ibot_output"])
    return got, zero


@pytest.mark.parametrize("setting,freeze", RUNS, ids=[f"{s}-{'frozen' if fz else 'trained'}" for s, fz in RUNS])
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("case", list(R.CASES))
def test_dino_step_rows_and_columns_vs_fp64_restatement(lib, cuda, case, mode, setting, freeze):
    ref = R.dino_ref(case, setting, freeze)
    want, yard = ref.flat(ref.reference(mode), mode), ref.yardstick(mode)
    margin = R.M32_DINO if mode == "fp32" else R.MBF_DINO
    got, zero = _device_step(ref, mode, cuda)
    assert set(got) == set(want), set(got) ^ set(want)
    rs = R.ratios(got, want, yard)
    kinds = {"gradients": lambda k: k.startswith(("backbone.", "head.")), "loss": lambda k: k.startswith("loss"),
             "centres and statistics": lambda k: k.startswith(("centre:", "stat:")), "activations": lambda k: k.startswith("act:")}
    line = f"DINO_ROWS {case} {setting} {'frozen' if freeze else 'trained'} {mode}:"
    for what, pick in kinds.items():
        sub = {k: r for k, r in rs.items() if pick(k)}
        if sub:
            w = R.worst(sub)
            line += f" {what} worst E/Y {w[1]:.3f} ({w[0]}, {w[4]} {w[5]}, E {w[2]:.2e}, Y {w[3]:.2e});"
    bad = [(k, f"E/Y {r[0]:.2f} > {margin:g} (E {r[1]:.3e}, Y {r[2]:.3e}, {r[3]} {r[4]})") for k, r in rs.items() if not r[0] <= margin]
    for k, bound in ref.zero_bias_bounds(mode).items():
        g = zero[k].double().abs()
        share = g / torch.as_tensor(bound, dtype=torch.float64)
        line += f" zero {k} {float(share.max()):.3f} of its bound;"
        if not bool((share <= 1.0).all()):
            bad.append((k, f"|g| {float(g.max()):.3e} at column {int(share.argmax())}: {float(share.max()):.2f} x its bound"))
    print(line)
    assert not bad, "\n".join(map(str, bad))
