"""CPU: the dropout mask's definition (numpy Philox against known answers, keep fractions), the torch restatements of
tests/dropout_ref.py against the oracle, and the host layer's acceptance of a dropout rate.  No device call."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from oracle import mae_oracle as O
from tests import dropout_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KNOWN = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("ctr,key,want", KNOWN)
def test_philox_known_answers(ctr, key, want):
    got = R.philox4x32_10(*ctr, *key)
    assert tuple(int(np.asarray(v).reshape(-1)[0]) for v in got) == want


def test_philox_is_vectorised_consistently():
    ctrs = np.array([k[0] for k in KNOWN], dtype=np.uint64)
    got = R.philox4x32_10(ctrs[:1, 0], ctrs[:1, 1], ctrs[:1, 2], ctrs[:1, 3], 0, 0)
    assert [int(v[0]) for v in got] == list(KNOWN[0][2])
    # word e & 3 of group e >> 2: the first four elements of a stream are the four words of counter 0
    assert list(R.stream_words(0, 0, 4)) == list(KNOWN[0][2]) and len(R.stream_words(0, 0, 7)) == 7


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_keep_fraction_and_independence(p):
    n = 1 << 20
    m = R.stream_mask(1234, 3, (n,), p)
    bound = 5 * np.sqrt(p * (1 - p) / n)
    assert abs(m.mean() - (1 - p)) <= bound, (m.mean(), bound)
    other_site, other_seed = R.stream_mask(1234, 4, (n,), p), R.stream_mask(1235, 3, (n,), p)
    for o in (other_site, other_seed):  # different masks, and independent ones: they agree where chance says
        agree = (o == m).mean()
        assert abs(agree - ((1 - p) ** 2 + p ** 2)) <= 5 * np.sqrt(0.25 / n) and not np.array_equal(o, m)
    a = R.attn_mask(99, 5, 2, 3, 65, p)
    assert a.shape == (2, 3, 65, 65) and abs(a.mean() - (1 - p)) <= 5 * np.sqrt(p * (1 - p) / a.size)
    assert not np.array_equal(a[0, 0], a[0, 1]) and not np.array_equal(a[0, 0], a[1, 0])


def test_threshold_and_scale_are_those_of_the_fp32_rate():
    assert R.threshold(0.0) == 0 and R.threshold(0.5) == 1 << 31 and R.threshold(0.25) == 1 << 30
    assert R.threshold(0.1) == int(np.floor(float(np.float32(0.1)) * 2.0 ** 32)) == 429496736
    assert R.scale(0.5) == 2.0 and R.scale(0.0) == 1.0 and R.scale(0.1) == float(np.float32(1) / (np.float32(1) - np.float32(0.1)))
    assert R.stream_mask(7, 1, (64,), 0.0).all()  # rate 0 keeps everything


def test_sdpa_with_mask_form():
    g = torch.Generator().manual_seed(3)
    q, k, v = (torch.randn(2, 3, 17, 16, generator=g, dtype=torch.float64) for _ in range(3))
    Z = torch.from_numpy(R.attn_mask(5, 9, 2, 3, 17, 0.25)).double() * R.scale(0.25)
    want = (torch.softmax((q @ k.transpose(-1, -2)) * 16 ** -0.5, dim=-1) * Z) @ v
    assert torch.allclose(R.sdpa_dropout(q, k, v, Z), want, rtol=1e-12, atol=1e-14)
    # the mask acts behind the normaliser: a row's kept probabilities do not sum to one
    assert not torch.allclose((torch.softmax(q @ k.transpose(-1, -2), -1) * Z).sum(-1), torch.ones(2, 3, 17, dtype=torch.float64))


def test_restatement_without_dropout_is_the_oracle():
    cfg = O.CONFIGS["tiny"]  # the tiny_b2_s0 configuration of the golden files
    params, x, noise = O.make_params(cfg, 0), O.make_volume(cfg, 2, 0), O.make_noise(cfg, 2, 0)
    o_loss, _, _, o_grads, _ = O.forward_backward(cfg, params, x, noise)
    loss, grads = R.mae_forward_backward(cfg, params, x, noise, R.Ones())
    assert abs(float(loss) - float(o_loss)) <= 1e-6 * abs(float(o_loss))
    assert set(grads) == set(o_grads)
    for n in grads:
        assert float((grads[n] - o_grads[n]).norm()) <= 1e-5 * float(o_grads[n].norm()) + 1e-12, n


def test_vit_restatement_without_dropout_is_the_oracle():
    from headct_foundation_amd.dino_model import ViTBackbone
    c = R.VIT_CASE
    m = ViTBackbone(**{k: c[k] for k in ("in_chans", "img_size", "patch_size", "hidden_size", "mlp_dim", "num_layers", "num_heads",
                                       "num_register_tokens", "qkv_bias")}, compute_dtype="fp32")
    p = O.make_vit_params({k: tuple(v.shape) for k, v in m.state_dict().items()}, c["seed"])
    x = R.vit_case_input()
    want, _ = O.vit_forward(p, x, c["patch_size"], c["num_heads"], c["num_layers"])
    got = R.vit_forward(p, x, c["patch_size"], c["num_heads"], c["num_layers"], R.Ones())
    assert torch.allclose(got, want, rtol=1e-6, atol=1e-6)
    dropped = R.vit_forward(p, x, c["patch_size"], c["num_heads"], c["num_layers"], R.Masks(11, 0.25))
    assert not torch.allclose(dropped, want, rtol=1e-3, atol=1e-3)


def test_models_accept_a_dropout_rate(lib):
    import headct_foundation_amd as pkg
    from headct_foundation_amd.dino_model import ViTBackbone
    cfg = O.CONFIGS["micro"]
    kw = dict(cfg.ctor_kwargs(), compute_dtype="fp32")
    vkw = dict(in_chans=1, img_size=16, patch_size=8, hidden_size=48, mlp_dim=96, num_layers=1, num_heads=3)
    m = pkg.MaskedAutoencoderViT(**dict(kw, dropout_rate=0.1))
    assert m.dropout_rate == pytest.approx(0.1) and m._ccfg.dropout_rate == pytest.approx(0.1) and m.last_dropout_seed is None
    assert ViTBackbone(**vkw, dropout_rate=0.1).dropout_rate == pytest.approx(0.1)
    assert pkg.ViT(**vkw, dropout_rate=0.1).dropout_rate == pytest.approx(0.1)
    # the state dict does not depend on the rate
    assert list(m.state_dict()) == list(pkg.MaskedAutoencoderViT(**kw).state_dict())
    for ctor, k in ((pkg.MaskedAutoencoderViT, kw), (ViTBackbone, vkw), (pkg.ViT, vkw)):
        with pytest.raises(ValueError, match="dropout_rate 1"):
            ctor(**dict(k, dropout_rate=1.0))
        with pytest.raises(ValueError, match="between 0 and 1"):
            ctor(**dict(k, dropout_rate=-0.1))
        with pytest.raises(ValueError, match="between 0 and 1"):
            ctor(**dict(k, dropout_rate=1.5))
    m.set_dropout_seed(2 ** 64 + 5)
    assert m._next_dropout_seed == 5


def test_symbols_sites_and_host_side_refusals(lib):
    from headct_foundation_amd import _lib, build, dropout
    hdr = open(os.path.join(ROOT, "include", "headct_hip.h")).read()
    for s in ("hct_dropout_mask", "hct_dropout_apply", "hct_attention_dropout_fwd", "hct_attention_dropout_bwd", "hct_mae_plan_set_dropout"):
        assert re.search(r"\b" + s + r"\s*\(", hdr) and s in _lib.exported_symbols() and hasattr(lib, s), s
    assert "dropout.hip" in build.SOURCES
    assert dropout.SITE_EMBEDDING == 0 and dropout.block_site(0, dropout.ATTN) == 1 and dropout.block_site(3, dropout.DROP2) == 16
    assert (dropout.ATTN, dropout.PROJ, dropout.DROP1, dropout.DROP2) == (R.ATTN, R.PROJ, R.DROP1, R.DROP2)
    with pytest.raises(ValueError):
        dropout.check_rate(1.0)
    # p = 1 and p < 0 are refused by name before any launch
    for p in (1.0, -0.25):
        assert lib.hct_dropout_mask(1, 0, 0, 16, 0, 0, p, None, None) != 0 and b"0 <= p < 1" in lib.hct_last_error_string()
        assert lib.hct_attention_dropout_fwd(None, 1, 4, 1, 16, 0, p, 1, 0, None, None, None) != 0 and b"0 <= p < 1" in lib.hct_last_error_string()
    base = dict(input_size=16, patch_size=8, in_chans=1, mask_ratio=0.75, pos_embed=1, encoder_depth=1, encoder_embed_dim=48,
                encoder_mlp_dim=96, encoder_num_heads=3, decoder_depth=1, decoder_embed_dim=48, decoder_mlp_dim=96, decoder_num_heads=3)
    sizes = {}
    for rate, ok in ((0.0, True), (0.25, True), (1.0, False), (-0.5, False)):
        h = lib.hct_mae_plan_create(C.byref(_lib.MaeConfig(**base, dropout_rate=rate)), 2, _lib.HCT_F32)
        assert bool(h) == ok, rate
        if h:
            sizes[rate] = lib.hct_mae_plan_workspace_bytes(h)
            assert lib.hct_mae_plan_set_dropout(h, 1, 7) == (1 if rate > 0 else 0) and lib.hct_mae_plan_set_dropout(h, 0, 7) == 0
            lib.hct_mae_plan_destroy(h)
    h0 = lib.hct_mae_plan_create(C.byref(_lib.MaeConfig(**base)), 2, _lib.HCT_F32)
    assert lib.hct_mae_plan_workspace_bytes(h0) == sizes[0.0] < sizes[0.25]  # rate 0: the workspace of a plan without the field
    lib.hct_mae_plan_destroy(h0)
