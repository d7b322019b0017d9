"""CPU: models built with norm_layer=RMSNorm (MAE.NORM_LAYER: rmsnorm).  The torch restatement (tests/rmsnorm_ref.py) against the
fixture made from the reference's own modules (tests/golden/rmsnorm.json), the host modules' state dicts against the reference's
manifests, the native plan's parameter layout for both kinds, and the entry points' build_model."""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import mae_oracle as O
from tests import rmsnorm_ref as R
from tests.util import load_golden, sample_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAE_CASES = [("micro", 2, 0), ("yaml_cut", 2, 1)]


def _vit_kwargs(lora=False):
    c = R.VIT_CASE
    return dict(in_chans=c["in_chans"], img_size=c["img_size"], patch_size=c["patch_size"], hidden_size=c["hidden_size"], mlp_dim=c["mlp_dim"],
                num_layers=c["num_layers"], num_heads=c["num_heads"], num_register_tokens=c["num_register_tokens"], qkv_bias=c["qkv_bias"],
                lora=lora)


@pytest.mark.parametrize("name,batch,seed", MAE_CASES)
def test_mae_restatement_reproduces_reference_fixture(name, batch, seed):
    """Pins tests/rmsnorm_ref.py to the reference where the reference itself is absent: loss, activations, prediction, every
    gradient (fp32 1e-3 is the project's bar; the restatement is the same arithmetic and sits at ~1e-6) and the 4-step curve."""
    fx = load_golden("rmsnorm")["mae"][name]
    cfg = O.CONFIGS[name]
    params = R.make_params(cfg, seed)
    assert [[k, list(v.shape)] for k, v in params.items()] == [[k, s] for k, s, _ in fx["state_dict_manifest"]]
    x, noise = O.make_volume(cfg, batch, seed), O.make_noise(cfg, batch, seed)
    loss, pred, mask, grads, inter = R.forward_backward(cfg, params, x, noise, want_inter=True)
    assert abs(float(loss) - fx["loss"]) <= 1e-5 * abs(fx["loss"]) and float(mask.sum()) == fx["mask_sum"]
    for k, entry in list(fx["act"].items()) + [("pred", fx["pred"])]:
        got, want, l2, l2w = sample_of(pred if k == "pred" else inter[k], entry)
        assert abs(l2 - l2w) <= 1e-5 * l2w and torch.allclose(got, want, rtol=1e-4, atol=1e-5 * float(want.abs().max())), k
    frozen = {n for n, _, rg in R.param_shapes(cfg) if not rg}
    assert set(grads) == set(fx["grads"]) == set(params) - frozen
    for k, entry in fx["grads"].items():
        got, want, l2, l2w = sample_of(grads[k], entry)
        assert torch.allclose(got, want, rtol=1e-3, atol=2e-5 * float(want.abs().max()) + 1e-9), k
    hp, tr = fx["train"]["hp"], fx["train"]
    st = O.TrainState({k: v.clone() for k, v in params.items()})
    losses, lrs = [], []
    for i in range(tr["steps"]):
        l, lr, _, _ = R.train_step(cfg, st, O.make_volume(cfg, batch, seed + 10 + i), O.make_noise(cfg, batch, seed + 10 + i), **hp)
        losses.append(l)
        lrs.append(lr)
    assert np.allclose(lrs, tr["lrs"], rtol=1e-12) and np.allclose(losses, tr["logged_losses"], atol=6e-5)
    for k, entry in tr["params_after"].items():
        got, want, _, _ = sample_of(st.params[k], entry)
        assert torch.allclose(got, want, rtol=1e-4, atol=4 * hp["base_lr"] if k.endswith("qkv.bias") else 1e-5), k


@pytest.mark.parametrize("lora", [False, True], ids=["plain", "lora"])
def test_vit_restatement_reproduces_reference_fixture(lora):
    fx = load_golden("rmsnorm")["vit_lora" if lora else "vit"]
    c = fx["case"]
    assert c == R.VIT_CASE
    params = R.vit_case_params({e["name"]: e["shape"] for e in fx["state_dict"]})
    p = {k: v.double().requires_grad_(k in fx["trainable"]) for k, v in params.items()}
    out, hidden = R.vit_forward(p, R.vit_case_input().double(), c["patch_size"], c["num_heads"], c["num_layers"])
    R.case_loss(out).backward()
    for t, entry in [(out, fx["out"])] + list(zip(hidden, fx["hidden"])):
        got, want, l2, l2w = sample_of(t, entry)
        assert abs(l2 - l2w) <= 1e-5 * l2w and torch.allclose(got, want, rtol=1e-4, atol=1e-5)
    assert {k for k, v in p.items() if v.grad is not None} == set(fx["grads"])
    for k, entry in fx["grads"].items():
        got, want, _, _ = sample_of(p[k].grad, entry)
        assert torch.allclose(got, want, rtol=1e-3, atol=2e-5 * float(want.abs().max()) + 1e-9), k


@pytest.mark.parametrize("name,batch,seed", MAE_CASES)
def test_mae_module_mirrors_reference_state_dict(lib, name, batch, seed):
    from headct_foundation_amd import MaskedAutoencoderViT, RMSNorm
    fx = load_golden("rmsnorm")["mae"][name]
    cfg = O.CONFIGS[name]
    m = MaskedAutoencoderViT(**cfg.ctor_kwargs(), norm_layer=RMSNorm)
    assert [[k, list(v.shape), str(v.dtype)] for k, v in m.state_dict().items()] == fx["state_dict_manifest"]
    assert len(fx["state_dict_manifest"]) == {"micro": 43, "yaml_cut": 33}[name]
    assert [n for n, _ in m.named_parameters()] == [n for n, _, _ in R.param_shapes(cfg)]
    assert not any(R.is_norm_bias(k) for k in m.state_dict())
    assert all(torch.equal(v, torch.ones_like(v)) for k, v in m.state_dict().items() if k.endswith("norm.weight"))
    assert [n for n, p in m.named_parameters() if not p.requires_grad] == ["decoder_pos_embed"]
    params = R.make_params(cfg, seed)
    m.load_state_dict(params, strict=True)
    for k, v in m.state_dict().items():
        assert torch.equal(v, params[k]), k
    base = m._flat.data_ptr()
    for n, p in m.named_parameters():
        assert base <= p.data_ptr() < base + m._flat.numel() * 4
    # a LayerNorm checkpoint: strict refuses it, non-strict reports the norm biases as unexpected (as torch does)
    ln = O.make_params(cfg, seed)
    with pytest.raises(RuntimeError, match="Unexpected"):
        m.load_state_dict(ln, strict=True)
    res = m.load_state_dict(ln, strict=False)
    assert sorted(res.unexpected_keys) == sorted(k for k in ln if R.is_norm_bias(k)) and not res.missing_keys
    # the default stays LayerNorm, with its biases
    d = MaskedAutoencoderViT(**cfg.ctor_kwargs())
    assert [n for n, _ in d.named_parameters()] == [n for n, _, _ in O.param_shapes(cfg)]
    with pytest.raises(NotImplementedError):
        MaskedAutoencoderViT(**cfg.ctor_kwargs(), norm_layer=nn.BatchNorm1d)


@pytest.mark.parametrize("lora", [False, True], ids=["plain", "lora"])
def test_vit_modules_mirror_reference_state_dict(lib, lora):
    from headct_foundation_amd import RMSNorm, ViT
    from headct_foundation_amd.dino_model import ViTBackbone
    from headct_foundation_amd.misc import set_requires_grad_false
    fx = load_golden("rmsnorm")["vit_lora" if lora else "vit"]
    want = [[e["name"], e["shape"]] for e in fx["state_dict"]]
    params = R.vit_case_params({e["name"]: e["shape"] for e in fx["state_dict"]})
    for cls in (ViT, ViTBackbone):
        m = cls(**_vit_kwargs(lora), norm_layer=RMSNorm)
        assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == want, cls.__name__
        assert all(v.dtype == torch.float32 for v in m.state_dict().values())
        assert all(torch.equal(v, torch.ones_like(v)) for k, v in m.state_dict().items() if k.endswith("norm.weight"))
        m.load_state_dict(params, strict=True)
        assert all(torch.equal(v, params[k]) for k, v in m.state_dict().items())
        if lora:  # the LoRA rule keeps names containing `norm` trainable: nothing to change for RMSNorm
            set_requires_grad_false(m, lora=True)
            assert [n for n, p in m.named_parameters() if p.requires_grad] == fx["trainable"], cls.__name__
        with pytest.raises(NotImplementedError):
            cls(**_vit_kwargs(lora), norm_layer=nn.GroupNorm)
    b = ViTBackbone(**_vit_kwargs(lora), norm_layer=RMSNorm)
    base = b._flat.data_ptr()
    assert all(base <= p.data_ptr() < base + b._flat.numel() * 4 for p in b.parameters())
    names, offs = b.flat_segments()
    assert set(names) == set(dict(b.named_parameters())) and offs[-1] == b._flat.numel()


def _plan_params(lib, cfg):
    from headct_foundation_amd import _lib
    h = lib.hct_mae_plan_create(C.byref(cfg), 2, _lib.HCT_F32)
    assert h, lib.hct_last_error_string()
    try:
        info, out = _lib.ParamInfo(), []
        for i in range(lib.hct_mae_plan_num_params(h)):
            _lib.check(lib.hct_mae_plan_param_info(h, i, C.byref(info)))
            out.append((info.name.decode(), int(info.offset), int(info.numel), tuple(int(info.shape[k]) for k in range(info.ndim))))
        total = int(lib.hct_mae_plan_param_elems(h))
        ranges = []
        for s in range(lib.hct_mae_num_backward_stages(h)):
            b, e = C.c_int64(), C.c_int64()
            _lib.check(lib.hct_mae_backward_stage_range(h, s, C.byref(b), C.byref(e)))
            ranges.append((b.value, e.value))
        return out, total, ranges
    finally:
        lib.hct_mae_plan_destroy(h)


def _mae_use_order(cfg):
    """Names of the MAE plan in forward-use order (csrc/mae_plan.hip: the flat layout), from the oracle's shapes."""
    shapes = {n: s for n, s, _ in O.param_shapes(cfg)}
    blk = ["att_norm.weight", "att_norm.bias", "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight", "attn.proj.bias", "ffn_norm.weight",
           "ffn_norm.bias", "mlp.linear1.weight", "mlp.linear1.bias", "mlp.linear2.weight", "mlp.linear2.bias"]
    order = ["patch_embedding.patch_embeddings.weight", "patch_embedding.patch_embeddings.bias", "patch_embedding.position_embeddings", "cls_token"]
    order += [f"blocks.{i}.{s}" for i in range(cfg.encoder_depth) for s in blk]
    order += ["norm.weight", "norm.bias", "decoder_embed.weight", "decoder_embed.bias", "mask_token", "decoder_cls_token", "decoder_pos_embed"]
    order += [f"decoder_blocks.{i}.{s}" for i in range(cfg.decoder_depth) for s in blk]
    order += ["decoder_norm.weight", "decoder_norm.bias", "decoder_pred.weight", "decoder_pred.bias"]
    order = [n for n in order if n in shapes]
    assert set(order) == set(shapes)
    return order, shapes


def _expected_layout(order, shapes):
    out, off = [], 0
    for n in order:
        numel = int(np.prod(shapes[n]))
        out.append((n, off, numel, tuple(shapes[n])))
        off += (numel + 1023) // 1024 * 1024  # every tensor starts on a 1024-element unit
    return out, off


@pytest.mark.parametrize("name", ["micro", "yaml_cut", "tiny"])
def test_plan_parameter_layout_for_both_kinds(lib, name):
    """norm_kind 0 lists exactly the LayerNorm model's parameters at the offsets of the 1024-unit rule (the layout of the parent
    commit); 1 lists the same without the norm biases; 2 is refused with an error string.  For both kinds the backward stages'
    ranges tile [0, param_elems) from the end to the start."""
    from headct_foundation_amd import MaskedAutoencoderViT, RMSNorm, _lib
    cfg = O.CONFIGS[name]
    order, shapes = _mae_use_order(cfg)
    for kind, norm_layer in ((0, nn.LayerNorm), (1, RMSNorm)):
        ccfg = MaskedAutoencoderViT(**cfg.ctor_kwargs(), norm_layer=norm_layer)._ccfg
        assert ccfg.norm_kind == kind
        got, total, ranges = _plan_params(lib, ccfg)
        want, wtotal = _expected_layout([n for n in order if kind == 0 or not R.is_norm_bias(n)], shapes)
        assert got == want and total == wtotal
        assert ranges[0][1] == total and ranges[-1][0] == 0
        assert all(b < e for b, e in ranges) and all(ranges[i + 1][1] == ranges[i][0] for i in range(len(ranges) - 1))
    bad = MaskedAutoencoderViT(**cfg.ctor_kwargs())._ccfg
    bad.norm_kind = 2
    assert not lib.hct_mae_plan_create(C.byref(bad), 2, _lib.HCT_F32)
    assert b"norm_kind" in lib.hct_last_error_string()


def test_vitb_mae_has_42_tensors_fewer(lib):
    from headct_foundation_amd import _lib
    base = dict(input_size=96, patch_size=16, in_chans=1, mask_ratio=0.75, pos_embed=2, encoder_depth=12, encoder_embed_dim=768,
                encoder_mlp_dim=3072, encoder_num_heads=12, decoder_depth=8, decoder_embed_dim=768, decoder_mlp_dim=3072, decoder_num_heads=16)
    (ln, ln_total, _), (rms, rms_total, _) = (_plan_params(lib, _lib.MaeConfig(**base, norm_kind=k)) for k in (0, 1))
    assert len(ln) - len(rms) == 42 and ln_total - rms_total == 43008
    assert [n for n, *_ in ln if not R.is_norm_bias(n)] == [n for n, *_ in rms]


@pytest.mark.parametrize("lora", [False, True], ids=["plain", "lora"])
def test_encoder_only_plan_layout_for_both_kinds(lib, lora):
    from headct_foundation_amd import RMSNorm
    from headct_foundation_amd.dino_model import ViTBackbone
    layouts = {}
    for kind, norm_layer in ((0, nn.LayerNorm), (1, RMSNorm)):
        m = ViTBackbone(**_vit_kwargs(lora), norm_layer=norm_layer)
        got, total, ranges = _plan_params(lib, m._ccfg)
        shapes = {n: tuple(p.shape) for n, p in m.named_parameters()}
        want, wtotal = _expected_layout([n for n, *_ in got], shapes)  # the plan's order, offsets by the unit rule
        assert got == want and total == wtotal and set(shapes) == {n for n, *_ in got}
        assert ranges[0][1] == total and ranges[-1][0] == 0 and all(ranges[i + 1][1] == ranges[i][0] for i in range(len(ranges) - 1))
        layouts[kind] = [n for n, *_ in got]
    assert [n for n in layouts[0] if not R.is_norm_bias(n)] == layouts[1]
    assert len(layouts[0]) - len(layouts[1]) == 2 * R.VIT_CASE["num_layers"] + 1


def test_build_model_reads_the_norm_layer(lib, monkeypatch, tmp_path):
    import config as cfgmod
    import main_downstream
    import main_pretrain_mae
    from headct_foundation_amd import RMSNorm
    from headct_foundation_amd.layers import _Affine

    def mae_config(norm):
        a = argparse.Namespace(cfg=os.path.join(ROOT, "configs/mae/mae_tiny_plumbing.yaml"), opts=["MAE.NORM_LAYER", norm], local_rank=0)
        return cfgmod.get_config(a)
    m = main_pretrain_mae.build_model(mae_config("rmsnorm"), torch.device("cpu"))
    assert m.norm_kind == 1 and isinstance(m.norm, RMSNorm) and isinstance(m.decoder_blocks[0].ffn_norm, RMSNorm)
    assert not any(R.is_norm_bias(k) for k in m.state_dict())
    m = main_pretrain_mae.build_model(mae_config("layernorm"), torch.device("cpu"))
    assert m.norm_kind == 0 and isinstance(m.norm, _Affine) and "norm.bias" in m.state_dict()
    with pytest.raises(ValueError):
        main_pretrain_mae.build_model(mae_config("batchnorm"), torch.device("cpu"))

    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("MODEL:\n  NAME: vit\n")

    def vit_config(norm, lora):
        argv = ["main_downstream.py", "--cfg", str(cfg), "--model_name", "vit", "--classifier", "linear", "--opts", "MAE.NORM_LAYER", norm,
                "TRAIN.LORA", str(lora), "VIT.INPUT_SIZE", "24", "VIT.PATCH_SIZE", "12", "VIT.HIDDEN_SIZE", "48", "VIT.MLP_DIM", "96",
                "VIT.NUM_LAYERS", "2", "VIT.NUM_HEADS", "3"]
        monkeypatch.setattr(sys, "argv", argv)
        return main_downstream.parse_option()[1]
    for lora in (False, True):
        model, _ = main_downstream.build_model(vit_config("rmsnorm", lora), torch.device("cpu"))
        assert model.norm_kind == 1 and isinstance(model.norm, RMSNorm) and not any(R.is_norm_bias(k) for k in model.state_dict())
        assert model.lora == lora
    model, _ = main_downstream.build_model(vit_config("layernorm", False), torch.device("cpu"))
    assert model.norm_kind == 0 and "norm.bias" in model.state_dict()
    with pytest.raises(ValueError, match="not supported"):
        main_downstream.build_model(vit_config("groupnorm", False), torch.device("cpu"))


def test_rmsnorm_forward_fails_loudly_without_gpu(lib):
    from headct_foundation_amd import HctError, MaskedAutoencoderViT, RMSNorm, ViT
    from headct_foundation_amd.dino_model import ViTBackbone
    cfg = O.CONFIGS["micro"]
    with pytest.raises(HctError):
        MaskedAutoencoderViT(**cfg.ctor_kwargs(), norm_layer=RMSNorm)(O.make_volume(cfg, 2, 0))
    x = R.vit_case_input()
    with pytest.raises(HctError):
        ViT(**_vit_kwargs(), norm_layer=RMSNorm)(x)
    with pytest.raises(HctError):
        ViTBackbone(**_vit_kwargs(), norm_layer=RMSNorm)(x)
    with pytest.raises(HctError):
        RMSNorm(48)(torch.zeros(2, 48))  # a parameter holder: never called
