"""GPU: stochastic depth (drop path) on the HIP ViT path against tests/drop_path_ref.py -- the table of per-sample multipliers bit for
bit, the streaming pass, pinned-seed parity of the backbone in fp32 and bf16 (with and without element dropout, with LoRA), a dropped
branch's exact zeros, inertness, determinism, refusals, and short engine-style runs."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from headct_foundation_amd import _lib, dropout
from headct_foundation_amd._lib import HCT_BF16, HCT_F32
from oracle import mae_oracle as O
from tests import drop_path_ref as P
from tests import dropout_ref as R
from tests import lora_ref
from tests.util import grads_by_name, rel_err

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x9E3779B97F4A7C15  # a seed with both key words in use
PASS_SITE = 3              # at q = 0.5 this seed keeps samples [1, 0, 1, 0, 1, ...] there: mixed for every B >= 2
P_MODEL = 0.25


def _st():
    return torch.cuda.current_stream().cuda_stream


def _dt(t):
    return HCT_BF16 if t.dtype == torch.bfloat16 else HCT_F32


def _rand(shape, dev, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(dtype).to(dev)


# ---- 1. the table --------------------------------------------------------------------------------------------------------------------
# B = 1, 3, 5: word indices 0 .. 3 and a second counter; 64 and 257: many counters, 257 with a ragged last group
@pytest.mark.parametrize("B", [1, 3, 5, 64, 257])
def test_table_is_the_numpy_table(lib, cuda, B):
    sites = [6, 7, 14, 2]  # four sites, 6 and 7 neighbours
    rates = [0.5, 0.5, 0.1, 0.0]
    got = dropout.path_scales(SEED, sites, rates, B, device=cuda)
    assert got.shape == (4, B) and got.dtype == torch.float32
    want = np.stack([P.path_scales(SEED, s, q, B) for s, q in zip(sites, rates)])
    assert np.array_equal(got.cpu().numpy(), want)
    assert torch.equal(got[3], torch.ones(B, device=cuda)), "the q = 0 row is exactly 1.0"
    for row, q in zip(got.cpu().numpy()[:3], rates[:3]):
        assert set(np.unique(row)) <= {0.0, np.float32(R.scale(q))}
    if B == 257:
        assert not torch.equal(got[0], got[1]), "neighbouring sites decide independently"
        assert 0 < int((got[0] == 0).sum()) < B and 0 < int((got[2] == 0).sum()) < B // 4


# ---- 2. the streaming pass -----------------------------------------------------------------------------------------------------------
def _apply(lib, x, y, res, B, seg, scales, site, p):
    _lib.check(lib.hct_residual_drop_apply(x.data_ptr(), _dt(x), y.data_ptr(), _dt(y), _lib.ptr(res), B, seg, scales.data_ptr(), SEED, site, p,
                                           _st()), "hct_residual_drop_apply")
    torch.cuda.synchronize()


# (3, 5, 20): segments of 100 elements = 25 groups; (5, 17, 192); (2, 1100, 500): 275 000 groups, more than one sweep of the grid
# (1024 blocks x 256 threads), so threads loop
@pytest.mark.parametrize("shape", [(3, 5, 20), (5, 17, 192), (2, 1100, 500)])
@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_residual_drop_apply(lib, cuda, shape, p, residual, dtype):
    B, q = shape[0], 0.5
    s_np = P.path_scales(SEED, PASS_SITE, q, B)
    assert (s_np == 0).any() and (s_np != 0).any(), "precondition: a dropped and a kept sample"
    scales = dropout.path_scales(SEED, [PASS_SITE], [q], B, device=cuda)[0].contiguous()
    x = _rand(shape, cuda, dtype, 1)
    res = _rand(shape, cuda, torch.float32, 3) if residual else None
    out_dtype = torch.float32 if residual else dtype
    y = torch.full(shape, float("nan"), dtype=out_dtype, device=cuda)
    _apply(lib, x, y, res, B, shape[1] * shape[2], scales, PASS_SITE, p)
    Z = torch.from_numpy(R.stream_mask(SEED, PASS_SITE, shape, p)).to(cuda).float() * R.scale(p) if p > 0 else torch.ones(shape, device=cuda)
    c = Z * torch.from_numpy(s_np).to(cuda).view(B, 1, 1)   # one combined multiplier, rounded once
    want = x.float() * c                                    # ... the product rounded ...
    if residual:
        want = want + res                                   # ... and the sum rounded: no fused multiply-add
    assert torch.equal(y, want if out_dtype == torch.float32 else want.to(dtype))
    for b in np.flatnonzero(s_np == 0):  # a dropped sample: the residual alone, bit for bit (zeros without one)
        assert torch.equal(y[b], res[b] if residual else torch.zeros_like(y[b]))


def test_residual_drop_apply_refuses_samples_that_split_a_group(lib, cuda):
    """[3, 1, 6]: segments of 6 elements would start inside a group of four; one sample may end ragged."""
    x = _rand((3, 1, 6), cuda, torch.float32, 2)
    y = torch.full_like(x, float("nan"))
    scales = dropout.path_scales(SEED, [PASS_SITE], [0.5], 3, device=cuda)[0].contiguous()
    with pytest.raises(_lib.HctError, match="multiple of 4"):
        _apply(lib, x, y, None, 3, 6, scales, PASS_SITE, 0.25)
    assert torch.isnan(y).all()
    x8 = _rand((3, 1, 8), cuda, torch.float32, 3)
    with pytest.raises(_lib.HctError, match="residual form writes fp32"):
        _apply(lib, x8.bfloat16(), torch.empty_like(x8).bfloat16(), x8, 3, 8, scales, PASS_SITE, 0.25)
    one = dropout.path_scales(SEED, [PASS_SITE], [0.5], 1, device=cuda)[0].contiguous()  # sample 0 is kept there
    v, out = x.reshape(-1)[:11].contiguous(), torch.full((11,), float("nan"), device=cuda)
    _apply(lib, v, out, None, 1, 11, one, PASS_SITE, 0.25)
    Z = torch.from_numpy(R.stream_mask(SEED, PASS_SITE, (11,), 0.25)).to(cuda).float() * R.scale(0.25)
    assert torch.equal(out, v * (Z * one))


# ---- the model -----------------------------------------------------------------------------------------------------------------------
def _vit(dtype, p_drop, rate, lora=False, cuda=None, case=P.PATH_CASE):
    from headct_foundation_amd.dino_model import ViTBackbone
    m = ViTBackbone(**{k: case[k] for k in ("in_chans", "img_size", "patch_size", "hidden_size", "mlp_dim", "num_layers", "num_heads",
                                          "num_register_tokens", "qkv_bias")}, lora=lora, dropout_rate=p_drop, drop_path_rate=rate,
                    compute_dtype=dtype)
    p = O.make_vit_params({k: tuple(v.shape) for k, v in m.state_dict().items()}, case["seed"])
    for k in p:  # adapters that do something, tokens that matter
        if k.endswith("lora_matrix_A"):
            p[k] = p[k] * 50.0
        if k.endswith("lora_matrix_B"):
            p[k] = p[k] * 0.25
        if k in ("cls_token", "register_tokens"):
            p[k] = p[k] * 5.0
    m.load_state_dict(p, strict=True)
    return m.to(cuda), p


def _vit_step(m, x, seed=None):
    m.zero_grad()
    if seed is not None:
        m.set_dropout_seed(seed)
    tok = m(x)[0]
    lora_ref.case_loss(tok).backward()
    torch.cuda.synchronize()
    return tok.detach().float().cpu(), grads_by_name(m)


_REF = {}


def _vit_ref(p, x, masks, trainable=None, case=P.PATH_CASE, key=None):
    """(tokens, gradients) of the restatement; computed once per `key` and shared (read only)."""
    if key is not None and key in _REF:
        return _REF[key]
    pv = {k: v.clone().requires_grad_(trainable is None or trainable(k)) for k, v in p.items()}
    tok = R.vit_forward(pv, x, case["patch_size"], case["num_heads"], case["num_layers"], masks)
    lora_ref.case_loss(tok).backward()
    out = tok.detach(), {k: v.grad for k, v in pv.items() if v.grad is not None}
    if key is not None:
        _REF[key] = out
    return out


def _same(a, b):
    return torch.equal(a[0], b[0]) and a[1].keys() == b[1].keys() and all(torch.equal(a[1][k], b[1][k]) for k in a[1])


# ---- 3. / 4. pinned seed against the restatement -------------------------------------------------------------------------------------
@pytest.mark.parametrize("p_drop", [0.0, P_MODEL])
@pytest.mark.parametrize("dtype,tol", [("fp32", 1e-3), ("bf16", 5e-2)])
def test_backbone_pinned_seed_vs_restatement(lib, cuda, dtype, tol, p_drop):
    """Three blocks, q = [0, .25, .5], four samples, seed 20140: every branch with q > 0 keeps some samples and drops some.  fp32 1e-3
    (the bar of the dropout test); bf16 5e-2 against the fp32 restatement (the bar of the bf16 ViT dropout test)."""
    m, p = _vit(dtype, p_drop, P.PATH_RATE, cuda=cuda)
    x = P.path_case_input()
    tok, grads = _vit_step(m.train(), x.to(cuda), P.SEED_MIXED)
    assert m.last_dropout_seed == P.SEED_MIXED
    r_tok, r_grads = _vit_ref(p, x, P.PathMasks(P.SEED_MIXED, p_drop, P.PATH_RATE, 3, 4), key=("path", p_drop))
    plain, _ = _vit_ref(p, x, P.PathMasks(P.SEED_MIXED, p_drop, 0.0, 3, 4), key=("plain", p_drop))
    assert rel_err(r_tok, plain) > 0.05, "drop path at 0.5 moves the tokens: the comparison discriminates"
    print("tokens", dtype, p_drop, rel_err(tok, r_tok))
    assert rel_err(tok, r_tok) <= tol
    assert set(grads) == set(r_grads)
    worst = max((rel_err(grads[k], r_grads[k]), k) for k in grads)
    print("worst gradient", dtype, p_drop, worst)
    assert worst[0] <= tol, worst
    if dtype == "fp32":
        for k in grads:  # the bias gradients of proj / linear2 take the column sums of the masked gradient
            if k.endswith(("proj.bias", "linear2.bias")):
                assert (grads[k] - r_grads[k]).abs().max() <= 1e-6 + 1e-3 * r_grads[k].abs().max(), k


# ---- 5. a dropped branch -------------------------------------------------------------------------------------------------------------
def test_dropped_branch_has_exactly_zero_gradients(lib, cuda):
    """B = 1, seed 1 keeps everything except the MLP branch of block 2."""
    case = dict(P.PATH_CASE, batch=1)
    m, p = _vit("fp32", 0.0, P.PATH_RATE, cuda=cuda, case=case)
    x = P.path_case_input(case)
    tok, grads = _vit_step(m.train(), x.to(cuda), P.SEED_ONE)
    for k in ("mlp.linear1.weight", "mlp.linear1.bias", "mlp.linear2.weight", "mlp.linear2.bias", "ffn_norm.weight", "ffn_norm.bias"):
        assert torch.count_nonzero(grads["blocks.2." + k]) == 0, k
    assert float(grads["blocks.2.attn.proj.weight"].abs().max()) > 0
    r_tok, r_grads = _vit_ref(p, x, P.PathMasks(P.SEED_ONE, 0.0, P.PATH_RATE, 3, 1), case=case)
    assert rel_err(tok, r_tok) <= 1e-3 and set(grads) == set(r_grads)
    for k in grads:
        if torch.count_nonzero(r_grads[k]) == 0:
            assert torch.count_nonzero(grads[k]) == 0, k
        else:
            assert rel_err(grads[k], r_grads[k]) <= 1e-3, (k, rel_err(grads[k], r_grads[k]))


# ---- 6. LoRA -------------------------------------------------------------------------------------------------------------------------
def test_lora_step_vs_restatement(lib, cuda):
    from headct_foundation_amd.misc import set_requires_grad_false
    m, p = _vit("fp32", 0.0, P.PATH_RATE, lora=True, cuda=cuda)
    set_requires_grad_false(m, lora=True)
    x = P.path_case_input()
    tok, grads = _vit_step(m.train(), x.to(cuda), P.SEED_MIXED)
    r_tok, r_grads = _vit_ref(p, x, P.PathMasks(P.SEED_MIXED, 0.0, P.PATH_RATE, 3, 4), trainable=lora_ref.trainable)
    assert rel_err(tok, r_tok) <= 1e-3
    assert set(grads) == set(r_grads) and sum("lora" in k for k in grads) == 12
    worst = max((rel_err(grads[k], r_grads[k]), k) for k in grads)
    print("worst gradient, lora", worst)
    assert worst[0] <= 1e-3, worst


# ---- 7. inert cases, bit for bit -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_eval_mode_rate_zero_and_one_block_are_inert(lib, cuda, dtype):
    x = P.path_case_input().to(cuda)
    v0, _ = _vit(dtype, 0.0, 0.0, cuda=cuda)
    vd, _ = _vit(dtype, 0.0, P.PATH_RATE, cuda=cuda)
    want = _vit_step(v0.train(), x)
    assert v0.last_dropout_seed is None, "a rate-0 model draws no seed"
    assert _same(want, _vit_step(vd.eval(), x)) and vd.last_dropout_seed is None
    dropped = _vit_step(vd.train(), x, P.SEED_MIXED)  # a dropped training step ...
    assert not torch.equal(dropped[0], want[0]) and vd.last_dropout_seed == P.SEED_MIXED
    assert _same(want, _vit_step(vd.eval(), x))       # ... leaves the eval-mode model the rate-0 model
    assert _same(want, _vit_step(v0.eval(), x))
    # one block: q = [0] whatever the rate -- training mode is the rate-0 model and draws nothing from torch's generator
    one = dict(P.PATH_CASE, num_layers=1)
    o0, _ = _vit(dtype, 0.0, 0.0, cuda=cuda, case=one)
    od, _ = _vit(dtype, 0.0, P.PATH_RATE, cuda=cuda, case=one)
    torch.manual_seed(5)
    probe = torch.rand(3)
    torch.manual_seed(5)
    got = _vit_step(od.train(), x)
    assert torch.equal(torch.rand(3), probe) and od.last_dropout_seed is None
    assert _same(_vit_step(o0.train(), x), got)


# ---- 8. determinism ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_determinism_and_seed_draw(lib, cuda, dtype):
    m, _ = _vit(dtype, 0.0, P.PATH_RATE, cuda=cuda)
    m.train()
    x = P.path_case_input().to(cuda)
    a, b, c = _vit_step(m, x, P.SEED_MIXED), _vit_step(m, x, P.SEED_MIXED), _vit_step(m, x, P.SEED_MIXED + 1)
    assert P.keep_tables(P.SEED_MIXED + 1, P.PATH_RATE, 3, 4) != P.KEEP_MIXED, "precondition: the next seed decides differently"
    assert _same(a, b) and not torch.equal(a[0], c[0])
    # unpinned: the seed comes from torch's CPU generator -- reproducible under manual_seed, fresh per forward
    torch.manual_seed(77)
    d = _vit_step(m, x)
    s1 = m.last_dropout_seed
    e = _vit_step(m, x)
    s2 = m.last_dropout_seed
    torch.manual_seed(77)
    f = _vit_step(m, x)
    assert s1 != s2 and m.last_dropout_seed == s1 and _same(d, f)
    if P.keep_tables(s1, P.PATH_RATE, 3, 4) != P.keep_tables(s2, P.PATH_RATE, 3, 4):
        assert not torch.equal(d[0], e[0])


# ---- 9. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals(lib, cuda):
    from headct_foundation_amd import MaskedAutoencoderViT
    from headct_foundation_amd.dino_model import ViTBackbone
    err = lambda: lib.hct_last_error_string().decode()
    mae = MaskedAutoencoderViT(**O.CONFIGS["micro"].ctor_kwargs(), compute_dtype="fp32")
    cfg = _lib.MaeConfig.from_buffer_copy(mae._ccfg)
    h = lib.hct_mae_plan_create(C.byref(cfg), 2, HCT_F32)
    assert h, err()
    lib.hct_mae_plan_destroy(h)
    cfg.drop_path_rate = 0.1  # a plan with a decoder has no stochastic depth
    assert not lib.hct_mae_plan_create(C.byref(cfg), 2, HCT_F32)
    assert "drop_path_rate" in err() and "encoder-only" in err()
    vit = ViTBackbone(1, 16, 8, 48, 96, 3, 3, compute_dtype="fp32", drop_path_rate=0.5)
    for bad in (1.0, -0.25, 1.5):
        vcfg = _lib.MaeConfig.from_buffer_copy(vit._ccfg)
        vcfg.drop_path_rate = bad
        assert not lib.hct_mae_plan_create(C.byref(vcfg), 2, HCT_F32)
        assert "drop_path_rate" in err() and "0 <= r < 1" in err()
        with pytest.raises(ValueError, match="drop_path_rate"):
            ViTBackbone(1, 16, 8, 48, 96, 3, 3, drop_path_rate=bad)
    out = torch.zeros(1, 4, device=cuda)
    rc = lib.hct_drop_path_scales(SEED, (C.c_int * 1)(6), (C.c_float * 1)(1.0), 1, 4, out.data_ptr(), _st())
    assert rc != 0 and "0 <= p < 1" in err()
    with pytest.raises(ValueError, match="drop_path_rate"):
        dropout.path_scales(SEED, [6], [1.0], 4, device=cuda)


# ---- 10. engine level ----------------------------------------------------------------------------------------------------------------
def _options(module, argv):
    old = sys.argv
    try:
        sys.argv = argv
        return module.parse_option()[1]
    finally:
        sys.argv = old


def test_downstream_style_run_with_drop_path(lib, cuda, tmp_path):
    """Three fine-tuning steps of the model main_downstream.py builds at --drop_path 0.2 --layer_decay 0.75 (linear classifier, synthetic
    labelled volumes, cut ViT), then an evaluation pass whose loss is that of a rate-0 backbone holding the same weights."""
    import main_downstream as M
    from headct_foundation_amd import cross_entropy, layer_decay_scales
    from headct_foundation_amd.data import SyntheticLabelled
    from headct_foundation_amd.optim import HipAdamW, clip_grad_norm_
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("MODEL:\n  NAME: vit\n")
    opts = ["VIT.INPUT_SIZE", "24", "VIT.PATCH_SIZE", "12", "VIT.HIDDEN_SIZE", "48", "VIT.MLP_DIM", "96", "VIT.NUM_LAYERS", "3", "VIT.NUM_HEADS", "3"]
    base = ["main_downstream.py", "--cfg", str(cfg), "--model_name", "vit", "--classifier", "linear"]
    config = _options(M, base + ["--drop_path", "0.2", "--layer_decay", "0.75", "--opts"] + opts)
    assert config.VIT.DROP_PATH_RATE == 0.2 and config.TRAIN.LAYER_DECAY == 0.75
    torch.manual_seed(5)
    vit, cls = M.build_model(config, cuda)
    assert vit.drop_path_rate == 0.2
    opts_ = [HipAdamW(cls, lr=1e-3, weight_decay=0.04), HipAdamW(vit, lr=1e-4, weight_decay=0.04)]
    opts_[1].set_scales(layer_decay_scales(vit, config.TRAIN.LAYER_DECAY))
    v, t, _ = SyntheticLabelled(1, 8, config.VIT.IN_CHANS, 24, 2, cuda, seed=0).batches[0]
    losses = []
    vit.train()
    cls.train()
    for _ in range(3):
        for o in opts_:
            o.zero_grad()
        loss = cross_entropy(cls(vit(v)[0]), t)
        loss.backward()
        clip_grad_norm_(cls, 1.0)
        clip_grad_norm_(vit, 1.0)
        for o in opts_:
            o.step()
        losses.append(float(loss.detach()))
    assert all(np.isfinite(losses)) and max(losses) < 5 * min(losses) and vit.last_dropout_seed is not None
    v0, _ = M.build_model(_options(M, base + ["--drop_path", "0", "--opts"] + opts), torch.device("cpu"))
    assert v0.drop_path_rate == 0.0
    v0.load_state_dict({k: p.detach().cpu() for k, p in vit.state_dict().items()}, strict=True)
    v0 = v0.to(cuda).eval()
    cls.eval()
    with torch.no_grad():
        a, b = cls(vit.eval()(v)[0]), cls(v0(v)[0])
    assert torch.equal(a, b) and float(F.cross_entropy(a.float(), t.long())) == float(F.cross_entropy(b.float(), t.long()))


def test_dino_iteration_with_drop_path(lib, cuda):
    """One DINO iteration of the pair main_pretrain_dino.py builds from dino_tiny_plumbing.yaml at --drop_path 0.2: the student drops paths,
    the teacher (in training mode too, as the engine keeps it) does not -- its outputs are those of a run at rate 0 on the same weights."""
    import main_pretrain_dino as M
    from engine_pretrain_dino import _forward_loss
    from headct_foundation_amd.dino import DINOLoss, SyntheticCrops
    base = ["main_pretrain_dino.py", "--cfg", os.path.join(ROOT, "configs/dino/dino_tiny_plumbing.yaml")]
    config, config0 = _options(M, base + ["--drop_path", "0.2"]), _options(M, base)
    assert config.VIT.DROP_PATH_RATE == 0.2 and config0.VIT.DROP_PATH_RATE == 0.0
    torch.manual_seed(3)
    student, teacher = M.build_pair(config, cuda, config.VIT.DROP_PATH_RATE), M.build_pair(config, cuda)
    teacher.load_state_dict(student.state_dict())
    teacher0 = M.build_pair(config0, cuda, config0.VIT.DROP_PATH_RATE)
    teacher0.load_state_dict(student.state_dict())
    assert student.backbone.drop_path_rate == 0.2 and teacher.backbone.drop_path_rate == 0.0
    n_crops = 2 + config.DINO.LOCAL_CROP_NUM
    crops = next(iter(SyntheticCrops(1, config.DATA.BATCH_SIZE, n_crops, config.VIT.IN_CHANS, config.VIT.INPUT_SIZE, cuda, 0)))
    crit = DINOLoss(out_dim=config.DINO.HEAD_N_PROTOTYPES, ncrops=n_crops, warmup_teacher_temp=config.DINO.WARMUP_TEACHER_TEMP,
                    teacher_temp=config.DINO.TEACHER_TEMP, warmup_teacher_temp_epochs=config.DINO.WARMUP_TEACHER_EPOCHS,
                    nepochs=config.TRAIN.MAX_EPOCHS).to(cuda)
    student.train()
    teacher.train()
    teacher0.train()
    loss = _forward_loss(student, teacher, crops, crit, 0, cuda)
    loss.backward()
    torch.cuda.synchronize()
    assert np.isfinite(float(loss.detach()))
    assert student.backbone.last_dropout_seed is not None and teacher.backbone.last_dropout_seed is None
    with torch.no_grad():
        t, t0 = teacher(list(crops[:2]))["dino_output"], teacher0(list(crops[:2]))["dino_output"]
    assert torch.equal(t, t0) and teacher.backbone.last_dropout_seed is None
