"""CPU: the iBOT yardstick (tests/ibot_ref.py) against torch autograd in float64, the mask generator's contract, the host's row indices
and weights against a brute-force build, the config keys, the case lists of tests/test_ibot_gpu.py against the loop limits they are
there to cross, the header's declarations, and the parameter layout with and without the mask token."""
import os
import re
import sys

import numpy as np
import pytest
import torch

from tests import ibot_ref as IR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64


# ---- the restated loss -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["centering", "sinkhorn_knopp"])
def test_restated_gradient_is_autograds(form):
    M, K, n_g, Ts, Tt = 7, 12, 4, 0.1, 0.04
    g = torch.Generator().manual_seed(5)
    s = torch.randn(M, K, generator=g, dtype=F64).requires_grad_(True)
    t = torch.randn(M, K, generator=g, dtype=F64)
    w = torch.rand(M, generator=g, dtype=F64)
    w[3] = 0.0
    center = 0.1 * torch.randn(K, generator=g, dtype=F64)
    sk = IR.sk_logs(t, Tt, 3, n_total=11) if form == "sinkhorn_knopp" else None
    loss, ds, csum = IR.ibot_loss(s, t, w, 1.0 / n_g, Ts, Tt, center=center, sk=sk, dloss=2.5)
    (loss * 2.5).backward()
    assert torch.allclose(s.grad, ds.detach(), rtol=1e-12, atol=1e-15)
    assert torch.count_nonzero(ds[3]) == 0, "a row of weight 0 has a zero gradient"
    assert torch.allclose(csum, t.sum(0))
    if form == "sinkhorn_knopp":  # what Sinkhorn-Knopp is for: after the row pass every row of q sums to 1 / N * N = 1
        lc, lr, log_n = sk
        q = torch.exp(t / Tt + lr[:, None] + lc[None, :] + log_n)
        assert torch.allclose(q.sum(1), torch.ones(M, dtype=F64), atol=1e-12)


def test_unit_weight_one_sample_is_soft_target_cross_entropy():
    """w = 1 on every row and n_g = 1: the restatement is sum_i CE(softmax target q_i, logits s_i / T_s)."""
    M, K, Ts, Tt = 5, 16, 0.1, 0.04
    g = torch.Generator().manual_seed(6)
    s, t = torch.randn(M, K, generator=g, dtype=F64), torch.randn(M, K, generator=g, dtype=F64)
    center = torch.zeros(K, dtype=F64)
    loss, _, _ = IR.ibot_loss(s, t, torch.ones(M, dtype=F64), 1.0, Ts, Tt, center=center)
    want = torch.nn.functional.cross_entropy(s / Ts, torch.softmax(t / Tt, dim=1), reduction="sum")
    assert abs(float(loss) - float(want)) <= 1e-12 * abs(float(want))


def test_restated_assembly():
    B, L, Rn, D = 2, 5, 2, 4
    g = np.random.default_rng(0)
    tok, cls, reg, pos, mt = (g.standard_normal(s).astype(np.float32) for s in ((B * L, D), (D,), (Rn, D), (L, D), (D,)))
    mask = IR.mask_pattern("never", B, L, 1)
    h0 = IR.assemble_fwd(tok, cls, reg, pos, mt, mask)
    assert np.array_equal(h0[1, 0], cls) and np.array_equal(h0[0, 2], reg[1])
    for b in range(B):
        for l in range(L):
            assert np.array_equal(h0[b, 1 + Rn + l], (mt if mask[b, l] else tok[b * L + l]) + pos[l])
    dh0 = g.integers(-8, 9, (B, 1 + Rn + L, D)).astype(np.float32)
    bw = IR.assemble_bwd(dh0, mask, Rn)
    t = torch.from_numpy(tok).double().requires_grad_(True)
    m_ = torch.from_numpy(mt).double().requires_grad_(True)
    rows = torch.where(torch.from_numpy(mask.astype(bool))[:, :, None], m_.expand(B, L, D), t.view(B, L, D))
    (rows * torch.from_numpy(dh0[:, 1 + Rn:]).double()).sum().backward()
    assert np.array_equal(bw["dtok"], t.grad.numpy()) and np.array_equal(bw["dmask_token"], m_.grad.numpy())
    assert bw["n_masked"] == int(mask.sum())
    for kind in IR.MASK_PATTERNS:
        m = IR.mask_pattern(kind, IR.ASM_B, IR.ASM_L)
        assert m.shape == (IR.ASM_B, IR.ASM_L)
    assert IR.mask_pattern("none", 3, 27).sum() == 0 and IR.mask_pattern("one", 3, 27).sum() == 1 and IR.mask_pattern("all", 3, 27).all()
    s = IR.mask_pattern("sample", 3, 27)
    assert s[1].all() and s.sum() == 27
    n = IR.mask_pattern("never", 3, 27)
    assert (n.sum(0) == 0).any() and (n.sum(0) == 3).any() and 0 < n.sum() < 81


# ---- the generator ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [2, 8])
def test_mask_generator_contract(grid):
    from headct_foundation_amd.ibot import IBotMaskGenerator
    L = grid ** 3
    for n_g, ratio, prob in ((8, (0.1, 0.5), 0.5), (4, (0.1, 0.5), 0.5), (6, (0.3, 0.3), 1.0), (5, (0.05, 0.9), 0.4)):
        gen = IBotMaskGenerator(grid, ratio, prob, seed=11)
        for _ in range(5):
            IR.generator_contract(gen(n_g), n_g, L, ratio, prob)
    a, b, c = (IBotMaskGenerator(grid, seed=s) for s in (3, 3, 4))
    ma, mb, mc = [a(8) for _ in range(3)], [b(8) for _ in range(3)], [c(8) for _ in range(3)]
    assert all(np.array_equal(x, y) for x, y in zip(ma, mb)), "reproducible per seed"
    assert not all(np.array_equal(x, y) for x, y in zip(ma, mc)), "different across seeds"
    assert not np.array_equal(ma[0], ma[1]), "fresh masks per call"
    with pytest.raises(ValueError, match="0 samples"):
        IBotMaskGenerator(grid, sample_prob=0.5)(1)
    for bad in (dict(ratio=(0.0, 0.5)), dict(ratio=(0.6, 0.5)), dict(ratio=(0.1, 1.5)), dict(sample_prob=0.0), dict(sample_prob=1.5)):
        with pytest.raises(ValueError):
            IBotMaskGenerator(grid, **bad)


def test_mask_generator_is_blockwise_at_512():
    """Cuboids, not scattered patches: at L = 512 a masked patch has, on average, clearly more masked face neighbours than uniform
    masking at the same ratio gives (expected share = the ratio itself, at most 0.5)."""
    from headct_foundation_amd.ibot import IBotMaskGenerator
    gen = IBotMaskGenerator(8, (0.3, 0.5), 1.0, seed=2)
    m = gen(16).reshape(16, 8, 8, 8).astype(bool)
    same = int((m[:, 1:] & m[:, :-1]).sum()) + int((m[:, :, 1:] & m[:, :, :-1]).sum()) + int((m[:, :, :, 1:] & m[:, :, :, :-1]).sum())
    share = 2.0 * same / (6.0 * m.sum())  # masked neighbours per masked patch / 6 (edges of the grid count as unmasked)
    assert share > 0.6, share


def test_rows_and_weights_against_brute_force():
    from headct_foundation_amd.ibot import IBotMaskGenerator, ibot_rows_and_weights, pad_head_rows
    for grid, Rn, n_g in ((2, 0, 4), (2, 1, 4), (3, 4, 6)):
        masks = IBotMaskGenerator(grid, seed=grid + Rn)(n_g)
        rows, weights, M = ibot_rows_and_weights(masks, Rn)
        want_r, want_w = IR.rows_and_weights(masks, Rn)
        assert rows.dtype == np.int32 and weights.dtype == np.float32 and M == int(masks.sum()) == len(rows)
        assert np.array_equal(rows, want_r) and np.array_equal(weights.view(np.int32), want_w.view(np.int32))
        per_sample = np.bincount(rows // (1 + Rn + grid ** 3), weights=weights.astype(np.float64), minlength=n_g)
        assert np.allclose(per_sample[masks.sum(1) > 0], 1.0), "the weights of one sample's masked patches sum to 1"
    assert [pad_head_rows(n) for n in (1, 16, 17, 32)] == [16, 16, 32, 32] and IR.HEAD_ROW_MULTIPLE == 16


# ---- config ------------------------------------------------------------------------------------------------------------------------------
def _parse(monkeypatch, tmp_path, *extra):
    import main_pretrain_dino
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("MODEL:\n  NAME: dino\nDINO:\n  USE_BN: False\n")  # (the reference yaml's setting; config.py's default is True)
    monkeypatch.setattr(sys, "argv", ["main_pretrain_dino.py", "--cfg", str(cfg), "--model_name", "dino", *extra])
    return main_pretrain_dino.parse_option()[1]


def test_config_keys_flags_and_validation(lib, monkeypatch, tmp_path):
    import config as cfgmod
    d = cfgmod._C.DINO
    assert d.IBOT_WEIGHT == 0.0 and list(d.IBOT_MASK_RATIO) == [0.1, 0.5] and d.IBOT_MASK_PROB == 0.5
    c = _parse(monkeypatch, tmp_path)
    assert c.DINO.IBOT_WEIGHT == 0.0 and list(c.DINO.IBOT_MASK_RATIO) == [0.1, 0.5] and c.DINO.IBOT_MASK_PROB == 0.5
    c = _parse(monkeypatch, tmp_path, "--ibot_weight", "1.0", "--ibot_mask_ratio", "0.2", "0.4", "--ibot_mask_prob", "0.75")
    assert c.DINO.IBOT_WEIGHT == 1.0 and list(c.DINO.IBOT_MASK_RATIO) == [0.2, 0.4] and c.DINO.IBOT_MASK_PROB == 0.75
    c = _parse(monkeypatch, tmp_path, "--ibot_weight", "0")
    assert c.DINO.IBOT_WEIGHT == 0.0
    c = _parse(monkeypatch, tmp_path, "--opts", "DINO.IBOT_WEIGHT", "0.5")
    assert c.DINO.IBOT_WEIGHT == 0.5
    for bad, key in ((("--ibot_weight", "-1"), "IBOT_WEIGHT"), (("--ibot_weight", "nan"), "IBOT_WEIGHT"),
                     (("--ibot_mask_ratio", "0.5", "0.2"), "IBOT_MASK_RATIO"), (("--ibot_mask_ratio", "0", "0.2"), "IBOT_MASK_RATIO"),
                     (("--ibot_mask_ratio", "0.1", "1.2"), "IBOT_MASK_RATIO"), (("--ibot_mask_prob", "0"), "IBOT_MASK_PROB"),
                     (("--ibot_mask_prob", "1.5"), "IBOT_MASK_PROB")):
        with pytest.raises(ValueError, match=key):
            _parse(monkeypatch, tmp_path, *bad)
    with pytest.raises(ValueError, match="USE_BN"):
        _parse(monkeypatch, tmp_path, "--ibot_weight", "1.0", "--opts", "DINO.USE_BN", "True")
    _parse(monkeypatch, tmp_path, "--opts", "DINO.USE_BN", "True")  # alone it stays what it was


# ---- the GPU file's case lists cross the limits they are there to cross ------------------------------------------------------------------------
def test_gpu_case_lists_cross_the_loop_limits():
    # assembly: one float4 per row / a row of 65 float4s that straddles forward blocks and takes the 128-thread row loops; R = 0 and R > 0
    assert set(IR.ASM_D) == {4, 260} and 260 // 4 > 64 and (260 // 4) % IR.ASM_FWD_BLOCK != 0 and set(IR.ASM_R) == {0, 2}
    assert IR.ASM_B * IR.ASM_L < IR.MASK_ROWS_PER_BLOCK, "the small cases are one block of level 1; the big case crosses both levels"
    big = IR.ASM_BIG
    rows = big["B"] * big["L"]
    nblk = -(-rows // IR.MASK_ROWS_PER_BLOCK)
    assert nblk > 1 and rows % IR.MASK_ROWS_PER_BLOCK != 0, "several level-1 blocks, the last one ragged"
    assert nblk > IR.MASK_FOLD_BATCH and nblk % IR.MASK_FOLD_BATCH != 0, "level 2: a full batch and a ragged one"
    assert big["D"] > IR.ASM_COLS_PER_TRIP and big["D"] % 4 == 0, "a second trip of the column loop"
    assert big["L"] % IR.MASK_ROWS_PER_BLOCK != 0, "a level-1 block spans two samples"
    # loss: the issue's shapes, and the limits of the kernel as built
    shapes = IR.LOSS_SHAPES
    assert {(1, 4), (3, 1028), (37, 2052), (130, 2052)} <= set(shapes)
    Ms, Ks = {m for m, _ in shapes}, {k for _, k in shapes}
    assert any(k < IR.LOSS_CHUNK for k in Ks) and IR.LOSS_CHUNK in Ks and any(k > 2 * IR.LOSS_CHUNK and k % IR.LOSS_CHUNK for k in Ks)
    assert any(m < IR.LOSS_ROWS_PER_SPLIT for m in Ms) and IR.LOSS_ROWS_PER_SPLIT in Ms and IR.LOSS_ROWS_PER_SPLIT + 1 in Ms
    assert any(m > 2 * IR.LOSS_ROWS_PER_SPLIT and m % IR.LOSS_ROWS_PER_SPLIT for m in Ms), "three splits, the last one ragged"
    assert all(k % 4 == 0 for k in Ks) and set(IR.LOSS_SCALES) == {1.0, 8.0}
    for M, K in shapes:
        inp = IR.loss_inputs(M, K, 1.0, torch.float32)
        w = inp["weight"]
        if M > 1:
            assert int((w == 0).sum()) == 1, "one weight is 0"
        if M > 2:
            assert len(set(w[w > 0].tolist())) > 1, "the weights differ per row"


def test_constants_are_the_sources():
    """The named limits are the ones the kernels are built with."""
    el = open(os.path.join(ROOT, "headct_foundation_amd", "csrc", "elementwise.hip")).read()
    dn = open(os.path.join(ROOT, "headct_foundation_amd", "csrc", "dino.hip")).read()
    assert f"constexpr int kMaskRowsPerBlock = {IR.MASK_ROWS_PER_BLOCK};" in el and f"constexpr int kMaskFoldBatch = {IR.MASK_FOLD_BATCH};" in el
    assert f"constexpr int kIbotRowsPerSplit = {IR.LOSS_ROWS_PER_SPLIT};" in dn and f"blockIdx.x * {IR.LOSS_CHUNK} + threadIdx.x * 4" in dn


# ---- header, bindings, layout ----------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("hct_vit_assemble_masked_fwd", "hct_vit_assemble_masked_bwd", "hct_vit_assemble_masked_bwd_workspace_bytes",
               "hct_vit_forward_parts_masked", "hct_ibot_loss_workspace_bytes", "hct_ibot_loss", "hct_ibot_loss_sk")


def test_header_declares_and_library_exports_the_new_symbols(lib):
    from headct_foundation_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "headct_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(hct_[a-z0-9_]+)\s*\(", code))
    for s in NEW_SYMBOLS:
        assert s in declared and s in _lib._PROTOS and hasattr(lib, s), s
    # the newest field of hct_mae_config, ahead of the trailing double (tests/test_patch_dropout_cpu.py pins that one as the last 8 bytes)
    assert re.search(r"float drop_path_rate;\s*int mask_token;\s*double patch_dropout;\s*\} hct_mae_config;", code)
    assert [f[0] for f in _lib.MaeConfig._fields_[-3:]] == ["drop_path_rate", "mask_token", "patch_dropout"]
    assert _lib.MaeConfig.mask_token.offset == _lib.MaeConfig.drop_path_rate.offset + 4
    # host-side refusals need no GPU
    assert lib.hct_ibot_loss_workspace_bytes(9800, 65536) == (-(-2 * 9800 * 8 // 256) * 256) + (-(-154 * 64 * 4 // 256) * 256) + 154 * 65536 * 4
    assert lib.hct_vit_assemble_masked_bwd_workspace_bytes(5, 216, 1028) == 9 * 1028 * 4
    assert lib.hct_ibot_loss(None, None, 0, 1, 4, None, None, 0.1, 0.04, 1.0, None, None, None, None, None, 0, None) != 0
    assert b"hct_ibot_loss" in lib.hct_last_error_string()


def _tiny(**kw):
    from headct_foundation_amd.dino_model import ViTBackbone
    return ViTBackbone(in_chans=1, img_size=24, patch_size=12, hidden_size=48, mlp_dim=96, num_layers=2, num_heads=3, num_register_tokens=1,
                       qkv_bias=True, compute_dtype="fp32", **kw)


def test_backbone_without_mask_token_has_todays_layout(lib):
    import ctypes as C
    from headct_foundation_amd import _lib
    from tests import drop_path_ref as P
    plain, flagged, with_kw = _tiny(), _tiny(mask_token=True), _tiny(mask_token=False)
    keys = list(plain.state_dict())
    assert "mask_token" not in keys and list(with_kw.state_dict()) == keys
    assert [l[:4] for l in plain._layout] == [l[:4] for l in with_kw._layout] and plain._flat.numel() == with_kw._flat.numel()
    assert set(flagged.state_dict()) == set(keys) | {"mask_token"}
    assert tuple(flagged.mask_token.shape) == (1, 48) and torch.count_nonzero(flagged.mask_token) == 0
    # the flagged plan's other parameters keep their order; the new one sits with the other tokens of the embedding stage
    names = [l[0] for l in flagged._layout]
    assert [n for n in names if n != "mask_token"] == [l[0] for l in plain._layout]
    assert names.index("mask_token") == names.index("register_tokens") + 1
    # the MAE plan refuses the flag
    from headct_foundation_amd import MaskedAutoencoderViT
    from oracle import mae_oracle as O
    mae = MaskedAutoencoderViT(**O.CONFIGS["micro"].ctor_kwargs(), compute_dtype="fp32")
    ccfg = _lib.MaeConfig.from_buffer_copy(mae._ccfg)
    ccfg.mask_token = 1
    assert not lib.hct_mae_plan_create(C.byref(ccfg), 1, _lib.HCT_F32) and b"mask_token" in lib.hct_last_error_string()
    assert "mask_token" in dict(mae.named_parameters()) and mae._ccfg.mask_token == 0, "the MAE's own decoder mask_token is untouched"


def test_param_scales_treat_the_backbone_mask_token_as_a_token(lib):
    from headct_foundation_amd import MaskedAutoencoderViT, layer_decay_scales, no_decay_scales, vit_layer_id
    from headct_foundation_amd.dino_model import DINOHead, MultiCropWrapper
    from oracle import mae_oracle as O
    vit = _tiny(mask_token=True)
    assert vit_layer_id("mask_token", 2) == 0 == vit_layer_id("cls_token", 2)
    sc = layer_decay_scales(vit, 0.5)
    assert sc["mask_token"] == sc["cls_token"] == 0.5 ** 3
    wd = no_decay_scales(vit)
    assert wd["mask_token"] == 0.0 and set(wd) == set(no_decay_scales(_tiny())) | {"mask_token"}
    student = MultiCropWrapper(vit, DINOHead(48, 512, hidden_dim=64, bottleneck_dim=32))
    assert "backbone.mask_token" in no_decay_scales(student)
    mae = MaskedAutoencoderViT(**O.CONFIGS["micro"].ctor_kwargs(), compute_dtype="fp32")
    assert "mask_token" not in no_decay_scales(mae), "the MAE's decoder mask_token keeps its weight decay"


def test_sinkhorn_logs_signature_keeps_its_default():
    import inspect
    from headct_foundation_amd.dino import sinkhorn_knopp_logs
    sig = inspect.signature(sinkhorn_knopp_logs)
    assert list(sig.parameters) == ["teacher", "teacher_temp", "n_iters", "world", "n_total"] and sig.parameters["n_total"].default is None
