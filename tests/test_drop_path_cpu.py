"""CPU: stochastic depth (drop path) -- the yardstick tests/drop_path_ref.py held to the written definition (rates, pinned seeds, kept
share, what a dropped branch does to the gradients, inertness at rate 0), the host's rate / site helpers against it, the config key and
flag, and the constructors' refusals."""
import math
import sys

import numpy as np
import pytest
import torch

from oracle import mae_oracle as O
from tests import drop_path_ref as P
from tests import dropout_ref as R
from tests import lora_ref


# ---- rates ---------------------------------------------------------------------------------------------------------------------------
def test_rates():
    from headct_foundation_amd import dropout
    assert P.drop_path_rates(0.5, 1) == [0.0] and P.drop_path_rates(0.9, 1) == [0.0]
    assert P.drop_path_rates(0.5, 2) == [0.0, 0.5]
    q = P.drop_path_rates(0.1, 12)
    r = float(np.float32(0.1))
    assert len(q) == 12 and q[0] == 0.0 and q[11] == r
    for j, v in enumerate(q):  # double arithmetic on the fp32 rate, then one cast: the values are fp32 numbers
        assert v == float(np.float32(r * j / 11)) and v == float(np.float32(v))
    assert q[5] != r * 5 / 11, "the cast to fp32 is visible"
    assert all(a < b for a, b in zip(q, q[1:]))
    for rate, depth in ((0.5, 1), (0.5, 2), (0.1, 12), (0.5, 3), (0.0, 4)):  # the host's helper is the same function
        assert dropout.drop_path_rates(rate, depth) == P.drop_path_rates(rate, depth)
    assert P.drop_path_rates(0.5, 3) == [0.0, 0.25, 0.5]
    for j in range(3):
        assert dropout.path_site(j, 0) == P.path_site(j, 0) == 1 + 4 * j + 1 == dropout.block_site(j, dropout.PROJ)
        assert dropout.path_site(j, 1) == P.path_site(j, 1) == 1 + 4 * j + 3 == dropout.block_site(j, dropout.DROP2)
    for bad in (-0.1, 1.0, 1.5):
        with pytest.raises(ValueError, match="drop_path_rate"):
            dropout.drop_path_rates(bad, 3)
    with pytest.raises(ValueError):
        dropout.path_site(0, 2)


# ---- the decision --------------------------------------------------------------------------------------------------------------------
def test_pinned_seeds():
    """The two seeds the GPU tests rest on, from the counter definition: (b >> 2, 0, 1, site), word b & 3."""
    assert P.keep_tables(P.SEED_MIXED, P.PATH_RATE, 3, 4) == P.KEEP_MIXED
    for j in (1, 2):
        for branch in (0, 1):
            assert 0 < sum(P.KEEP_MIXED[j][branch]) < 4, "every branch with q > 0 keeps some samples and drops some"
    assert P.keep_tables(P.SEED_ONE, P.PATH_RATE, 3, 1) == P.KEEP_ONE
    # by hand: block 1's attention branch, sample 1 -> counter (0, 0, 1, 6), word 1
    w = R.philox4x32_10(0, 0, 1, 6, P.SEED_MIXED & 0xFFFFFFFF, P.SEED_MIXED >> 32)
    assert [int(int(w[i]) >= (1 << 30)) for i in range(4)] == P.KEEP_MIXED[1][0]
    # the third counter word tells the family from the element masks of the same site
    assert not np.array_equal(P.path_words(P.SEED_MIXED, 6, 64), R.stream_words(P.SEED_MIXED, 6, 64))
    # multipliers: 1 / (1 - q) in fp32 where kept, 0 where dropped, exactly 1 at q = 0
    s = P.path_scales(P.SEED_MIXED, P.path_site(1, 0), 0.25, 4)
    assert s.dtype == np.float32 and s.tolist() == [float(np.float32(1) / np.float32(0.75)), 0.0, float(np.float32(1) / np.float32(0.75)), float(np.float32(1) / np.float32(0.75))]
    assert P.path_scales(P.SEED_MIXED, 2, 0.0, 7).tolist() == [1.0] * 7


@pytest.mark.parametrize("q", [0.1, 0.5])
def test_kept_share(q):
    n = 100000
    kept = int(P.path_keep(0x9E3779B97F4A7C15, 14, q, n).sum())
    qf = float(np.float32(q))
    assert abs(kept - n * (1 - qf)) <= 4 * math.sqrt(n * qf * (1 - qf)), kept


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
def _case_params(case=P.PATH_CASE, lora=False):
    from headct_foundation_amd.dino_model import ViTBackbone
    m = ViTBackbone(**{k: case[k] for k in ("in_chans", "img_size", "patch_size", "hidden_size", "mlp_dim", "num_layers", "num_heads",
                                          "num_register_tokens", "qkv_bias")}, lora=lora, compute_dtype="fp32")
    p = O.make_vit_params({k: tuple(v.shape) for k, v in m.state_dict().items()}, case["seed"])
    for k in p:
        if k in ("cls_token", "register_tokens"):
            p[k] = p[k] * 5.0
    return p


def _ref(p, x, masks, case=P.PATH_CASE):
    pv = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    tok = R.vit_forward(pv, x, case["patch_size"], case["num_heads"], case["num_layers"], masks)
    lora_ref.case_loss(tok).backward()
    return tok.detach(), {k: v.grad for k, v in pv.items() if v.grad is not None}


def test_a_dropped_branch_gets_no_gradient():
    """Seed 1, B = 1 keeps everything except the MLP branch of block 2: that branch's parameters (the MLP and the norm in front of it) see
    a gradient of exactly zero, the attention branch of the same block does not, and the residual stream passes the gradient on."""
    case = dict(P.PATH_CASE, batch=1)
    p = _case_params(case)
    x = P.path_case_input(case)
    tok, g = _ref(p, x, P.PathMasks(P.SEED_ONE, 0.0, P.PATH_RATE, 3, 1), case)
    for k in g:
        if k.startswith(("blocks.2.mlp.", "blocks.2.ffn_norm.")):
            assert torch.count_nonzero(g[k]) == 0, k
        elif k.startswith("blocks.2.attn.") and not k.endswith("qkv.bias"):
            assert float(g[k].abs().max()) > 0, k
    assert sum(k.startswith(("blocks.2.mlp.", "blocks.2.ffn_norm.")) for k in g) == 6
    assert float(g["blocks.1.mlp.linear1.weight"].abs().max()) > 0 and float(g["blocks.0.attn.proj.weight"].abs().max()) > 0
    plain, _ = _ref(p, x, R.Ones(), case)
    assert not torch.equal(tok, plain)


@pytest.mark.parametrize("p_drop", [0.0, 0.25])
def test_rate_zero_path_masks_are_the_dropout_masks(p_drop):
    """At drop path rate 0, PathMasks is dropout_ref.Masks (p > 0) / Ones (p = 0), bit for bit: the mask tensors and a whole step."""
    seed, B = P.SEED_MIXED, 4
    mine = P.PathMasks(seed, p_drop, 0.0, 3, B)
    theirs = R.Masks(seed, p_drop) if p_drop > 0 else R.Ones()
    for site in range(0, 13):
        assert torch.equal(mine.stream(site, (B, 3, 8)), theirs.stream(site, (B, 3, 8)))
    assert torch.equal(mine.attn(5, B, 3, 11), theirs.attn(5, B, 3, 11))
    params, x = _case_params(), P.path_case_input()
    a, b = _ref(params, x, mine), _ref(params, x, theirs)
    assert torch.equal(a[0], b[0]) and all(torch.equal(a[1][k], b[1][k]) for k in a[1])
    # ... and at rate 0.5 the proj_drop / drop2 sites of blocks 1 and 2 carry the per-sample factor, the other sites do not
    half = P.PathMasks(seed, p_drop, P.PATH_RATE, 3, B)
    for site in (0, 1, 2, 3, 4, 5, 7, 9, 11):
        assert torch.equal(half.stream(site, (B, 3, 8)), theirs.stream(site, (B, 3, 8))), site
    z = half.stream(6, (B, 3, 8)) + torch.zeros(B, 3, 8)
    assert torch.count_nonzero(z[1]) == 0 and torch.count_nonzero(z[0]) > 0


# ---- configuration and arguments -----------------------------------------------------------------------------------------------------
def _parse(monkeypatch, tmp_path, *extra, yaml="MODEL:\n  NAME: vit\n"):
    import main_downstream
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(yaml)
    monkeypatch.setattr(sys, "argv", ["main_downstream.py", "--cfg", str(cfg), "--model_name", "vit", *extra])
    return main_downstream.parse_option()[1]


def test_config_key_and_flag(monkeypatch, tmp_path):
    import config as cfgmod
    assert cfgmod._C.VIT.DROP_PATH_RATE == 0.0
    assert _parse(monkeypatch, tmp_path).VIT.DROP_PATH_RATE == 0.0
    over = "MODEL:\n  NAME: vit\nVIT:\n  DROP_PATH_RATE: 0.3\n"
    assert _parse(monkeypatch, tmp_path, yaml=over).VIT.DROP_PATH_RATE == 0.3                      # the yaml override stands when the flag is absent
    assert _parse(monkeypatch, tmp_path, "--drop_path", "0", yaml=over).VIT.DROP_PATH_RATE == 0.0  # ... and --drop_path 0 reaches the config
    assert _parse(monkeypatch, tmp_path, "--drop_path", "0.1").VIT.DROP_PATH_RATE == 0.1
    assert _parse(monkeypatch, tmp_path, "--opts", "VIT.DROP_PATH_RATE", "0.2").VIT.DROP_PATH_RATE == 0.2
    c = _parse(monkeypatch, tmp_path, "--drop_path", "0.1", "--opts", "VIT.INPUT_SIZE", "24", "VIT.HIDDEN_SIZE", "48", "VIT.MLP_DIM", "96",
               "VIT.NUM_LAYERS", "3", "VIT.NUM_HEADS", "3")
    import main_downstream
    vit, _ = main_downstream.build_model(c, torch.device("cpu"))
    assert vit.drop_path_rate == 0.1 and vit._ccfg.drop_path_rate == np.float32(0.1)


def test_dino_entry_point_gives_the_rate_to_the_student_only(monkeypatch):
    import os
    import main_pretrain_dino as M
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    monkeypatch.setattr(sys, "argv", ["main_pretrain_dino.py", "--cfg", os.path.join(root, "configs/dino/dino_tiny_plumbing.yaml"), "--drop_path", "0.2"])
    config = M.parse_option()[1]
    assert config.VIT.DROP_PATH_RATE == 0.2
    student, teacher = M.build_pair(config, torch.device("cpu"), config.VIT.DROP_PATH_RATE), M.build_pair(config, torch.device("cpu"))
    assert student.backbone.drop_path_rate == 0.2 and teacher.backbone.drop_path_rate == 0.0
    assert list(student.state_dict()) == list(teacher.state_dict()), "drop path adds no parameters"


@pytest.mark.parametrize("bad", [-0.1, 1, 1.5])
def test_constructors_refuse(bad):
    from headct_foundation_amd import ViT
    from headct_foundation_amd.dino_model import ViTBackbone
    kw = dict(in_chans=1, img_size=16, patch_size=8, hidden_size=48, mlp_dim=96, num_layers=2, num_heads=3)
    for ctor in (ViTBackbone, ViT):
        with pytest.raises(ValueError, match="drop_path_rate"):
            ctor(**kw, drop_path_rate=bad)
    ok = ViTBackbone(**kw, drop_path_rate=0.5)
    assert ok.drop_path_rate == 0.5 and ok.last_dropout_seed is None
    assert ViT(**kw, drop_path_rate=0.5).drop_path_rate == 0.5  # forward only: accepted and inert
    assert ViTBackbone(**kw).drop_path_rate == 0.0
