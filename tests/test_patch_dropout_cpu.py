"""CPU: the patch-dropout yardstick (tests/patch_dropout_ref.py) against torch, the keep-count rule, the configuration surface and
refusals, and the new symbols of the cross-compiled library."""
import ctypes as C
import sys

import numpy as np
import pytest
import torch

from headct_foundation_amd import _lib, dropout
from oracle import mae_oracle as O
from tests import dropout_ref as R
from tests import patch_dropout_ref as PD

VIT_ARGS = ("in_chans", "img_size", "patch_size", "hidden_size", "mlp_dim", "num_layers", "num_heads", "num_register_tokens", "qkv_bias")


# ---- the yardstick against torch -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["random", "ties", "all_equal", "permutation"])
def test_rank_is_torch_stable_argsort(kind):
    B, L = 3, 27
    g = torch.Generator().manual_seed(3)
    noise = {"random": torch.rand(B, L, generator=g), "ties": torch.randint(0, 4, (B, L), generator=g).float(), "all_equal": torch.full((B, L), 0.5),
             "permutation": torch.stack([torch.randperm(L, generator=g).float() / L for _ in range(B)])}[kind]
    ids_shuffle, ids_restore = PD.rank(noise.numpy())
    want = torch.argsort(noise, dim=1, stable=True)
    assert torch.equal(torch.from_numpy(ids_shuffle), want)
    assert torch.equal(torch.from_numpy(ids_restore), torch.argsort(want, dim=1, stable=True))
    if kind == "all_equal":
        assert np.array_equal(ids_shuffle[0], np.arange(L))


@pytest.mark.parametrize("Rn,use_pos", [(0, True), (2, True), (2, False)])
def test_assembly_is_indexing_plus_autograd(Rn, use_pos):
    """float64: forward by torch indexing, backward by autograd."""
    B, L, K, D = 3, 8, 5, 12
    g = torch.Generator().manual_seed(11)
    tok = torch.randn(B * K, D, generator=g, dtype=torch.float64, requires_grad=True)
    cls = torch.randn(D, generator=g, dtype=torch.float64, requires_grad=True)
    reg = torch.randn(Rn, D, generator=g, dtype=torch.float64, requires_grad=True) if Rn else None
    pos = torch.randn(L, D, generator=g, dtype=torch.float64, requires_grad=True) if use_pos else None
    noise = torch.rand(B, L, generator=g)
    noise[:, 6] = 2.0  # position 6 is kept by nobody
    ids_shuffle, ids_restore = PD.rank(noise.numpy())
    keep = torch.from_numpy(ids_shuffle[:, :K])
    patch = tok.view(B, K, D) + (pos[keep] if use_pos else 0)
    h = torch.cat([cls.expand(B, 1, D)] + ([reg.expand(B, Rn, D)] if Rn else []) + [patch], dim=1)
    n = lambda t: None if t is None else t.detach().numpy().astype(np.float32)
    got = PD.assemble_fwd(n(tok), n(cls), n(reg), n(pos), ids_shuffle, B, K)
    assert got.shape == (B, 1 + Rn + K, D) and np.array_equal(got, PD.assemble_fwd(n(tok), n(cls), n(reg), n(pos), ids_shuffle, B, K))
    np.testing.assert_allclose(got, h.detach().numpy(), rtol=0, atol=1e-6)
    dh = torch.randn(B, 1 + Rn + K, D, generator=g, dtype=torch.float64)
    h.backward(dh)
    back = PD.assemble_bwd(dh.numpy(), ids_restore, L, K, Rn)
    np.testing.assert_allclose(back["dtok"], tok.grad.numpy(), rtol=0, atol=0)
    np.testing.assert_allclose(back["dcls"], cls.grad.numpy(), rtol=0, atol=1e-12)
    if Rn:
        np.testing.assert_allclose(back["dreg"], reg.grad.numpy(), rtol=0, atol=1e-12)
    if use_pos:
        np.testing.assert_allclose(back["dpos"], pos.grad.numpy(), rtol=0, atol=1e-12)
    assert not back["dpos"][6].any() and not back["abs"]["dpos"][6].any(), "a position nobody kept gets an exact 0"


def _case_params(case):
    from headct_foundation_amd.dino_model import ViTBackbone
    m = ViTBackbone(**{k: case[k] for k in VIT_ARGS}, compute_dtype="fp32")
    return O.make_vit_params({k: tuple(v.shape) for k, v in m.state_dict().items()}, case["seed"])


def test_rate_zero_is_dropout_ref_vit_forward():
    case = R.VIT_CASE
    p, x = _case_params(case), R.vit_case_input()
    for masks in (R.Ones(), R.Masks(77, 0.25)):
        a = PD.vit_forward_keep(p, x, None, 0.0, case["patch_size"], case["num_heads"], case["num_layers"], masks)
        b = R.vit_forward(p, x, case["patch_size"], case["num_heads"], case["num_layers"], masks)
        assert torch.equal(a, b)
    half = PD.vit_forward_keep(p, x, PD.case_noise(case, 8), PD.RATE_8, case["patch_size"], case["num_heads"], case["num_layers"], R.Ones())
    assert half.shape == (case["batch"], 1 + 1 + 4, case["hidden_size"])


def test_case_noise_has_its_ties():
    for case, L, rate in ((R.VIT_CASE, 8, PD.RATE_8), (PD.KEEP_CASE_27, 27, PD.RATE_27)):
        n = PD.case_noise(case, L)
        K = PD.keep_count(L, rate)
        ids_shuffle, _ = PD.rank(n.numpy())
        assert ids_shuffle[0, :2].tolist() == [0, 1] and float(n[0, 0]) == float(n[0, 1])
        a, b = ids_shuffle[-1, K - 1], ids_shuffle[-1, K]
        assert float(n[-1, a]) == float(n[-1, b]) and a < b, "the tie across the keep boundary goes to the lower index"


# ---- the keep count ------------------------------------------------------------------------------------------------------------------
def test_keep_count_rule():
    """int(L * (1 - rate)) with the rate and the arithmetic in double: (10, 0.1) keeps 9, (10, 0.7) keeps 3."""
    for f in (PD.keep_count, dropout.patch_keep_count):
        assert f(10, 0.1) == 9 and f(10, 0.7) == 3 and f(8, 0.5) == 4 and f(27, 0.4) == 16 and f(512, 0.75) == 128 and f(512, 0.0) == 512
        for bad in (1.0, -0.1, 1.5):
            with pytest.raises(ValueError):
                f(8, bad)
        with pytest.raises(ValueError, match="K|keeps"):
            f(8, 0.9)  # int(0.8) = 0
    # precondition: the case tells the rule from a rate carried as a float (0.1f = 0.100000001...), which keeps 8 of 10
    assert int(10 * (1 - float(np.float32(0.1)))) == 8


def test_native_plan_keep_count_and_refusals(lib):
    from headct_foundation_amd import MaskedAutoencoderViT
    from headct_foundation_amd.dino_model import ViTBackbone
    err = lambda: lib.hct_last_error_string().decode()
    vit = ViTBackbone(1, 40, 8, 48, 96, 2, 3, compute_dtype="fp32")  # L = 125
    base = _lib.MaeConfig.from_buffer_copy(vit._ccfg)
    assert base.patch_dropout == 0.0
    for rate in (0.0, 0.1, 0.7, 0.5, 0.99):
        cfg = _lib.MaeConfig.from_buffer_copy(base)
        cfg.patch_dropout = rate
        h = lib.hct_mae_plan_create(C.byref(cfg), 2, _lib.HCT_F32)
        assert h, err()
        assert lib.hct_mae_plan_len_keep(h) == PD.keep_count(125, rate)
        lib.hct_mae_plan_destroy(h)
    ten = ViTBackbone(1, (8, 8, 8), 8, 48, 96, 1, 3, compute_dtype="fp32")  # L = 1: any rate leaves nothing
    cfg = _lib.MaeConfig.from_buffer_copy(ten._ccfg)
    cfg.patch_dropout = 0.5
    assert not lib.hct_mae_plan_create(C.byref(cfg), 2, _lib.HCT_F32) and "patch_dropout" in err()
    for bad in (1.0, -0.25, 1.5, float("nan")):
        cfg = _lib.MaeConfig.from_buffer_copy(base)
        cfg.patch_dropout = bad
        assert not lib.hct_mae_plan_create(C.byref(cfg), 2, _lib.HCT_F32)
        assert "patch_dropout" in err() and "0 <= r < 1" in err()
    mae = MaskedAutoencoderViT(**O.CONFIGS["micro"].ctor_kwargs(), compute_dtype="fp32")
    mcfg = _lib.MaeConfig.from_buffer_copy(mae._ccfg)
    mcfg.patch_dropout = 0.5  # a plan with a decoder masks by mask_ratio
    assert not lib.hct_mae_plan_create(C.byref(mcfg), 2, _lib.HCT_F32)
    assert "patch_dropout" in err() and "encoder-only" in err()
    # the encoder-only plan still ignores mask_ratio, with and without the rate
    for rate, want in ((0.0, 125), (0.5, 62)):
        cfg = _lib.MaeConfig.from_buffer_copy(base)
        cfg.mask_ratio, cfg.patch_dropout = 0.9, rate
        h = lib.hct_mae_plan_create(C.byref(cfg), 2, _lib.HCT_F32)
        assert h and lib.hct_mae_plan_len_keep(h) == want
        lib.hct_mae_plan_destroy(h)


def test_constructor():
    from headct_foundation_amd.dino_model import ViTBackbone
    m = ViTBackbone(1, 16, 8, 48, 96, 2, 3, num_register_tokens=1, patch_dropout=0.5)
    assert m.patch_dropout == 0.5 and m.patch_keep == 4 and m.len_keep == m.num_patches == 8 and m.num_tokens == 10
    assert m._ccfg.patch_dropout == 0.0 and m._ccfg_keep.patch_dropout == 0.5
    m0 = ViTBackbone(1, 16, 8, 48, 96, 2, 3, num_register_tokens=1)
    assert m0.patch_dropout == 0.0 and m0.patch_keep == 8 and m0._ccfg_keep is None
    assert list(m.state_dict()) == list(m0.state_dict()), "patch dropout adds no parameters"
    for bad in (1.0, -0.1, 0.9):  # 0.9 of 8 patches keeps none
        with pytest.raises(ValueError, match="patch_dropout"):
            ViTBackbone(1, 16, 8, 48, 96, 2, 3, patch_dropout=bad)
    with pytest.raises(_lib.HctError, match="no CPU fallback"):
        m.train()(torch.zeros(2, 1, 16, 16, 16))


# ---- configuration and arguments -----------------------------------------------------------------------------------------------------
def _parse(monkeypatch, tmp_path, *extra, yaml="MODEL:\n  NAME: vit\n"):
    import main_downstream
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(yaml)
    monkeypatch.setattr(sys, "argv", ["main_downstream.py", "--cfg", str(cfg), "--model_name", "vit", *extra])
    return main_downstream.parse_option()[1]


def test_config_key_and_flag(monkeypatch, tmp_path):
    import config as cfgmod
    import main_downstream
    assert cfgmod._C.VIT.PATCH_DROPOUT == 0.0
    assert _parse(monkeypatch, tmp_path).VIT.PATCH_DROPOUT == 0.0
    over = "MODEL:\n  NAME: vit\nVIT:\n  PATCH_DROPOUT: 0.3\n"
    assert _parse(monkeypatch, tmp_path, yaml=over).VIT.PATCH_DROPOUT == 0.3
    assert _parse(monkeypatch, tmp_path, "--patch_dropout", "0", yaml=over).VIT.PATCH_DROPOUT == 0.0  # 0 reaches the config
    assert _parse(monkeypatch, tmp_path, "--patch_dropout", "0.25").VIT.PATCH_DROPOUT == 0.25
    assert _parse(monkeypatch, tmp_path, "--opts", "VIT.PATCH_DROPOUT", "0.2").VIT.PATCH_DROPOUT == 0.2
    for bad in ("1", "-0.1", "1.5", "nan"):
        with pytest.raises(ValueError, match="PATCH_DROPOUT"):
            _parse(monkeypatch, tmp_path, "--patch_dropout", bad)
    with pytest.raises(ValueError, match="PATCH_DROPOUT"):
        _parse(monkeypatch, tmp_path, yaml="MODEL:\n  NAME: vit\nVIT:\n  PATCH_DROPOUT: 1.0\n")
    small = ["--opts", "VIT.INPUT_SIZE", "24", "VIT.HIDDEN_SIZE", "48", "VIT.MLP_DIM", "96", "VIT.NUM_LAYERS", "2", "VIT.NUM_HEADS", "3"]
    c = _parse(monkeypatch, tmp_path, "--patch_dropout", "0.5", *small)
    vit, _ = main_downstream.build_model(c, torch.device("cpu"))
    assert vit.patch_dropout == 0.5 and vit.patch_keep == 4 and vit._ccfg_keep.patch_dropout == 0.5
    locked = _parse(monkeypatch, tmp_path, "--patch_dropout", "0.5", "--lock", *small)
    assert locked.VIT.PATCH_DROPOUT == 0.5 and locked.TRAIN.LOCK
    vit, _ = main_downstream.build_model(locked, torch.device("cpu"))
    assert vit.patch_dropout == 0.0 and vit._ccfg_keep is None, "a locked backbone is built without the rate"


def test_dino_entry_point_has_no_flag():
    import main_pretrain_dino as M
    import inspect
    assert "patch_dropout" not in inspect.getsource(M)


# ---- the library -----------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_in_the_library(lib):
    for name in ("hct_vit_assemble_keep_fwd", "hct_vit_assemble_keep_bwd", "hct_vit_forward_parts_keep"):
        assert name in _lib._PROTOS
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == len(_lib._PROTOS[name][1])
    assert C.sizeof(_lib.MaeConfig) % 8 == 0 and _lib.MaeConfig.patch_dropout.offset == C.sizeof(_lib.MaeConfig) - 8, "the trailing double"
    # refusals that need no device: bad arguments return before any launch
    err = lambda: lib.hct_last_error_string().decode()
    one = C.c_void_p(16)  # never dereferenced: the argument checks come first
    assert lib.hct_vit_assemble_keep_fwd(one, _lib.HCT_F32, one, None, None, one, 1, 8, 9, 0, 4, one, None) != 0 and "hct_vit_assemble_keep_fwd" in err()
    assert lib.hct_vit_assemble_keep_fwd(one, _lib.HCT_F32, one, None, None, one, 1, 8, 4, 0, 6, one, None) != 0 and "D % 4" in err()
    assert lib.hct_vit_assemble_keep_fwd(one, _lib.HCT_F32, one, None, None, one, 1, 8, 4, 2, 4, one, None) != 0, "R > 0 needs reg"
    assert lib.hct_vit_assemble_keep_bwd(one, None, 1, 8, 0, 0, 4, None, _lib.HCT_F32, None, None, None, None) != 0 and "hct_vit_assemble_keep_bwd" in err()
    assert lib.hct_vit_assemble_keep_bwd(one, None, 1, 8, 4, 0, 4, None, _lib.HCT_F32, None, None, one, None) != 0, "dpos needs the ids"
    assert lib.hct_vit_forward_parts_keep(None, None, 1, _lib.HCT_F32, None, None) != 0 and "hct_vit_forward_parts_keep" in err()
