"""CPU: LoRA fine-tuning of the ViT backbone (TRAIN.LORA).  The torch restatement (tests/lora_ref.py) against the fixture made from
the reference's own ViT(lora=True) (tests/golden/lora_vit.json); the host module's state dict and trainable set against the
fixture's manifest; the entry point's configuration."""
import os
import sys

import pytest
import torch

from tests import lora_ref as R
from tests.util import load_golden, sample_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _backbone(lora=True, dtype="fp32"):
    from headct_foundation_amd.dino_model import ViTBackbone
    c = R.CASE
    return ViTBackbone(in_chans=c["in_chans"], img_size=c["img_size"], patch_size=c["patch_size"], hidden_size=c["hidden_size"],
                       mlp_dim=c["mlp_dim"], num_layers=c["num_layers"], num_heads=c["num_heads"],
                       num_register_tokens=c["num_register_tokens"], qkv_bias=c["qkv_bias"], lora=lora, compute_dtype=dtype)


def test_restatement_reproduces_reference_fixture():
    fx = load_golden("lora_vit")
    assert fx["case"] == R.CASE
    c = R.CASE
    params = R.case_params({e["name"]: e["shape"] for e in fx["state_dict"]})
    p = {k: v.double().requires_grad_(True) for k, v in params.items()}
    out, _ = R.vit_forward(p, R.case_input().double(), c["patch_size"], c["num_heads"], c["num_layers"])
    R.case_loss(out).backward()
    got, want, l2, want_l2 = sample_of(out, fx["out"])
    err = float((got - want).norm() / want.norm())
    print("tokens: relative error", err)
    assert err <= 1e-4 and abs(l2 - want_l2) <= 1e-4 * want_l2
    assert set(fx["grads"]) == set(fx["trainable"])
    for name, entry in fx["grads"].items():
        got, want, l2, want_l2 = sample_of(p[name].grad, entry)
        err = float((got - want).norm() / want.norm())
        print(name, "relative error", err)
        assert err <= 1e-4 and abs(l2 - want_l2) <= 1e-4 * want_l2, name
    # the adapters matter in this case: without them the tokens differ by far more than the bound
    q = {k: v.double() for k, v in params.items() if "lora" not in k}
    plain, _ = R.vit_forward(q, R.case_input().double(), c["patch_size"], c["num_heads"], c["num_layers"])
    assert float((plain - out.detach()).norm() / out.detach().norm()) > 1e-2


def test_backbone_state_dict_and_trainable_set_match_reference(lib):
    from headct_foundation_amd.misc import set_requires_grad_false
    fx = load_golden("lora_vit")
    torch.manual_seed(0)
    m = _backbone()
    sd = m.state_dict()
    assert [(k, list(v.shape)) for k, v in sd.items()] == [(e["name"], e["shape"]) for e in fx["state_dict"]]
    assert fx["rank"] == 128
    for k, init in fx["fresh_init"].items():  # B zeros, A standard normal, as the reference's
        assert bool((sd[k] == 0).all()) == init["zero"], k
        if not init["zero"]:
            assert abs(float(sd[k].std()) - 1.0) < 0.05 and abs(init["std"] - 1.0) < 0.05, k
    set_requires_grad_false(m, lora=True)
    assert [n for n, p in m.named_parameters() if p.requires_grad] == fx["trainable"]
    assert all(R.trainable(n) == p.requires_grad for n, p in m.named_parameters())
    assert all(p.grad is None for p in m.parameters())
    # state dict round trip, and a pre-training checkpoint without adapter keys through load_model (non-strict)
    vals = R.case_params({k: list(v.shape) for k, v in sd.items()})
    m.load_state_dict(vals, strict=True)
    assert all(torch.equal(v, vals[k]) for k, v in m.state_dict().items())
    set_requires_grad_false(m)
    assert not any(p.requires_grad for p in m.parameters())


def test_pretrained_checkpoint_without_adapters_loads(lib, tmp_path):
    from headct_foundation_amd.cfgnode import CfgNode
    from headct_foundation_amd.misc import load_model
    torch.manual_seed(1)
    plain, m = _backbone(lora=False), _backbone()
    before = {k: v.clone() for k, v in m.state_dict().items() if "lora" in k}
    torch.save({"state_dict": {"module." + k: v + 0.25 for k, v in plain.state_dict().items()}}, tmp_path / "pre.pt")
    cfg = CfgNode({"MODEL": CfgNode({"PRETRAINED": str(tmp_path / "pre.pt"), "NAME": "vit"})})
    load_model(cfg, m, None, None)
    sd = m.state_dict()
    assert all(torch.equal(sd[k], v + 0.25) for k, v in plain.state_dict().items())
    assert all(torch.equal(sd[k], v) for k, v in before.items())  # the adapters keep their init


def test_plan_refuses_bad_ranks_and_mae_plans(lib):
    import ctypes as C
    from headct_foundation_amd import _lib
    base = dict(input_size=16, patch_size=8, in_chans=1, mask_ratio=0.75, pos_embed=1, encoder_depth=1, encoder_embed_dim=48,
                encoder_mlp_dim=96, encoder_num_heads=3, decoder_depth=1, decoder_embed_dim=48, decoder_mlp_dim=96, decoder_num_heads=3)
    for kw, ok in ((dict(encoder_only=1, lora_rank=128), True), (dict(encoder_only=1, lora_rank=32), True),
                   (dict(encoder_only=1, lora_rank=8), False), (dict(encoder_only=1, lora_rank=-32), False),
                   (dict(encoder_only=0, lora_rank=128), False), (dict(encoder_only=0, lora_rank=0), True)):
        cfg = _lib.MaeConfig(**base, **kw)
        h = lib.hct_mae_plan_create(C.byref(cfg), 2, _lib.HCT_F32)
        assert bool(h) == ok, kw
        if h:
            n = lib.hct_mae_plan_num_params(h)
            info = _lib.ParamInfo()
            names = []
            for i in range(n):
                _lib.check(lib.hct_mae_plan_param_info(h, i, C.byref(info)))
                names.append(info.name.decode())
            assert sum("lora" in s for s in names) == (4 if kw["lora_rank"] else 0)
            assert lib.hct_mae_plan_set_requires_grad(h, 0, 0) == 0 and lib.hct_mae_plan_set_requires_grad(h, n, 0) != 0
            lib.hct_mae_plan_destroy(h)
        else:
            assert lib.hct_last_error_string()


def test_main_downstream_accepts_lora(lib, monkeypatch, tmp_path):
    import main_downstream
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("MODEL:\n  NAME: vit\n")
    argv = ["main_downstream.py", "--cfg", str(cfg), "--model_name", "vit", "--classifier", "linear", "--opts", "TRAIN.LORA", "True",
            "VIT.INPUT_SIZE", "24", "VIT.PATCH_SIZE", "12", "VIT.HIDDEN_SIZE", "48", "VIT.MLP_DIM", "96", "VIT.NUM_LAYERS", "2",
            "VIT.NUM_HEADS", "3"]
    monkeypatch.setattr(sys, "argv", argv)
    _, config = main_downstream.parse_option()
    assert config.TRAIN.LORA is True
    model, classifier = main_downstream.build_model(config, torch.device("cpu"))
    assert model.lora and sum("lora" in n for n, _ in model.named_parameters()) == 8
    from headct_foundation_amd.misc import set_requires_grad_false
    set_requires_grad_false(model, lora=config.TRAIN.LORA)
    n_train = sum(p.numel() for p in model.parameters() if p.requires_grad)
    assert 0 < n_train < sum(p.numel() for p in model.parameters())
