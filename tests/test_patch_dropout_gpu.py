"""GPU: patch dropout on the HIP ViT path against tests/patch_dropout_ref.py -- the two assembly kernels one by one through the C ABI
(bit-equal copies and single additions, exact integer sums, the in-order fp32 bound on Gaussian sums, exact zeros for positions nobody
kept, NaN-filled guarded outputs), the plan and the module against the restatement with pinned noise (fp32 1e-3, bf16 5e-2 against the
restatement with bf16-rounded storage: the bars tests/test_drop_path_gpu.py holds the same model to), inertness, plan coexistence,
determinism, refusals, and main_downstream.py end to end."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from headct_foundation_amd import _lib
from headct_foundation_amd._lib import HCT_BF16, HCT_F32
from oracle import mae_oracle as O
from tests import drop_path_ref as P
from tests import dropout_ref as R
from tests import lora_ref
from tests import patch_dropout_ref as PD
from tests.util import grads_by_name, rel_err

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16 = torch.float32, torch.bfloat16
VIT_ARGS = ("in_chans", "img_size", "patch_size", "hidden_size", "mlp_dim", "num_layers", "num_heads", "num_register_tokens", "qkv_bias")
SEED = 0x9E3779B97F4A7C15


def _st():
    return torch.cuda.current_stream().cuda_stream


def _code(dtype):
    return HCT_BF16 if dtype == BF16 else HCT_F32


def _bits(t):
    return t.view({4: torch.int32, 2: torch.int16}[t.element_size()])


class _Out:
    """An output inside a larger buffer: body NaN, a guard band of at least one row (a multiple of 64 elements) on each side."""

    def __init__(self, shape, dtype, dev):
        n = math.prod(shape)
        self.guard = -(-max(shape[-1], 1) // 64) * 64
        buf = torch.full((n + 2 * self.guard,), float("nan"), dtype=dtype, device=dev)
        buf[:self.guard] = 7777.0
        buf[self.guard + n:] = 7777.0
        self.buf, self.n = buf, n
        self.before = (buf[:self.guard].clone(), buf[self.guard + n:].clone())
        self.t = buf[self.guard:self.guard + n].view(shape)
        self.ptr = self.t.data_ptr()

    def result(self):
        assert torch.equal(_bits(self.buf[:self.guard]), _bits(self.before[0])), "guard band below the output was written"
        assert torch.equal(_bits(self.buf[self.guard + self.n:]), _bits(self.before[1])), "guard band above the output was written"
        return self.t.cpu()


def _p(o):
    return None if o is None else (o.ptr if isinstance(o, _Out) else o.data_ptr())


def _noise(kind, B, L, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "equal":  # every value ties: the shuffle is the identity, positions K .. L - 1 are kept by nobody
        return torch.full((B, L), 0.25)
    return torch.stack([torch.randperm(L, generator=g).float() / L for _ in range(B)])


# ---- 1. the kernels, one by one ------------------------------------------------------------------------------------------------------
# D = 4: one float4, 63 idle lanes; 48: the model case; 1028 = 257 float4s: a second pass of the 256-thread block with one lane working
@pytest.mark.parametrize("tdt", [F32, BF16])
@pytest.mark.parametrize("D", [4, 48, 1028])
@pytest.mark.parametrize("L", [8, 27])
@pytest.mark.parametrize("B", [1, 3])
def test_assemble_keep_fwd(lib, cuda, B, L, D, tdt):
    g = torch.Generator().manual_seed(100 * B + L + D)
    for K in (1, L - 1, L):
        for Rn in (0, 2):
            for use_pos in (True, False):
                for kind in ("equal", "perm"):
                    ids_shuffle, _ = PD.rank(_noise(kind, B, L, K + Rn).numpy())
                    tok = torch.randn(B * K, D, generator=g).to(tdt)
                    cls, reg, pos = torch.randn(D, generator=g), torch.randn(Rn, D, generator=g) if Rn else None, torch.randn(L, D, generator=g)
                    dev = [t.to(cuda) if t is not None else None for t in (tok, cls, reg, pos)]
                    ids_d = torch.from_numpy(ids_shuffle).to(torch.int32).to(cuda)
                    outs = []
                    for _ in range(2):
                        h0 = _Out((B, 1 + Rn + K, D), F32, cuda)
                        _lib.check(lib.hct_vit_assemble_keep_fwd(dev[0].data_ptr(), _code(tdt), dev[1].data_ptr(), _p(dev[2]), dev[3].data_ptr() if use_pos else None,
                                                                 ids_d.data_ptr(), B, L, K, Rn, D, h0.ptr, _st()), "hct_vit_assemble_keep_fwd")
                        outs.append(h0)
                    torch.cuda.synchronize()
                    got = outs[0].result()
                    assert torch.equal(_bits(got), _bits(outs[1].result()))
                    want = PD.assemble_fwd(tok.float().numpy(), cls.numpy(), reg.numpy() if Rn else None, pos.numpy() if use_pos else None, ids_shuffle, B, K)
                    assert np.array_equal(got.numpy().view(np.int32), want.view(np.int32)), (K, Rn, use_pos, kind)


@pytest.mark.parametrize("tdt", [F32, BF16])
@pytest.mark.parametrize("D", [4, 48, 1028])
@pytest.mark.parametrize("L", [8, 27])
@pytest.mark.parametrize("B", [1, 3])
def test_assemble_keep_bwd(lib, cuda, B, L, D, tdt):
    g = torch.Generator().manual_seed(200 * B + L + D)
    for K in (1, L - 1, L):
        for Rn in (0, 2):
            for kind in ("equal", "perm"):
                _, ids_restore = PD.rank(_noise(kind, B, L, K + Rn).numpy())
                idr_d = torch.from_numpy(ids_restore).to(torch.int32).to(cuda)
                for values in ("int", "gauss"):
                    dh = torch.randint(-8, 9, (B, 1 + Rn + K, D), generator=g).float() if values == "int" else torch.randn(B, 1 + Rn + K, D, generator=g)
                    dh_d = dh.to(cuda)
                    ref = PD.assemble_bwd(dh.numpy(), ids_restore, L, K, Rn)
                    # every output there, then each one missing in turn (a null gradient is skipped, the others are unchanged)
                    for missing in (None, "dtok", "dcls", "dreg", "dpos") if values == "int" else (None,):
                        runs = []
                        for _ in range(2):
                            o = dict(dtok=_Out((B * K, D), tdt, cuda), dcls=_Out((D,), F32, cuda), dreg=_Out((Rn, D), F32, cuda) if Rn else None,
                                     dpos=_Out((L, D), F32, cuda))
                            if missing:
                                o[missing] = None
                            _lib.check(lib.hct_vit_assemble_keep_bwd(dh_d.data_ptr(), idr_d.data_ptr(), B, L, K, Rn, D, _p(o["dtok"]), _code(tdt), _p(o["dcls"]),
                                                                     _p(o["dreg"]), _p(o["dpos"]), _st()), "hct_vit_assemble_keep_bwd")
                            runs.append(o)
                        torch.cuda.synchronize()
                        got = {k: v.result() for k, v in runs[0].items() if v is not None}
                        for k, v in got.items():
                            assert torch.equal(_bits(v), _bits(runs[1][k].result())), (k, "a second identical call differs")
                        what = (K, Rn, kind, values, missing)
                        if "dtok" in got:  # a copy and one cast: torch's
                            assert torch.equal(_bits(got["dtok"]), _bits(dh[:, 1 + Rn:, :].reshape(B * K, D).to(tdt))), what
                        for k in ("dcls", "dreg", "dpos"):
                            if k not in got:
                                continue
                            assert not torch.isnan(got[k]).any(), (k, what)
                            err = np.abs(got[k].numpy().astype(np.float64) - ref[k])
                            if values == "int":
                                assert not err.any(), (k, what, "an integer-valued sum is exact in any order")
                            else:  # the in-order fp32 sum of at most B terms
                                assert (err <= B * 2.0 ** -24 * ref["abs"][k]).all(), (k, what, float(err.max()))
                        if "dpos" in got:
                            never = ~(ids_restore < K).any(axis=0)
                            assert never.sum() == (L - K if kind == "equal" else never.sum())
                            assert torch.count_nonzero(got["dpos"][torch.from_numpy(never)]) == 0, "a position nobody kept gets an exact 0"
                            assert not torch.signbit(got["dpos"][torch.from_numpy(never)]).any()


def test_kernel_refusals(lib, cuda):
    err = lambda: lib.hct_last_error_string().decode()
    t = torch.zeros(64, device=cuda)
    ids = torch.zeros(64, dtype=torch.int32, device=cuda)
    out = _Out((2, 5, 4), F32, cuda)
    for K, D, Rn, reg in ((0, 4, 0, None), (9, 4, 0, None), (4, 6, 0, None), (4, 4, 2, None)):
        rc = lib.hct_vit_assemble_keep_fwd(t.data_ptr(), HCT_F32, t.data_ptr(), reg, t.data_ptr(), ids.data_ptr(), 2, 8, K, Rn, D, out.ptr, _st())
        assert rc != 0 and "hct_vit_assemble_keep_fwd" in err()
    assert lib.hct_vit_assemble_keep_bwd(t.data_ptr(), None, 2, 8, 4, 0, 4, None, HCT_F32, None, None, out.ptr, _st()) != 0 and "hct_vit_assemble_keep_bwd" in err()
    torch.cuda.synchronize()
    assert torch.isnan(out.result()).all(), "a refused call writes nothing"


# ---- the model -----------------------------------------------------------------------------------------------------------------------
CASES = {"L8": (R.VIT_CASE, 8, PD.RATE_8, 4), "L27": (PD.KEEP_CASE_27, 27, PD.RATE_27, 16)}


def _vit(case, dtype, cuda, rate=None, p_drop=0.0, path=0.0, lora=False):
    from headct_foundation_amd.dino_model import ViTBackbone
    kw = {} if rate is None else dict(patch_dropout=rate)
    m = ViTBackbone(**{k: case[k] for k in VIT_ARGS}, lora=lora, dropout_rate=p_drop, drop_path_rate=path, compute_dtype=dtype, **kw)
    p = O.make_vit_params({k: tuple(v.shape) for k, v in m.state_dict().items()}, case["seed"])
    for k in p:  # adapters that do something, tokens and positions that matter
        if k.endswith("lora_matrix_A"):
            p[k] = p[k] * 50.0
        if k.endswith("lora_matrix_B"):
            p[k] = p[k] * 0.25
        if k in ("cls_token", "register_tokens"):
            p[k] = p[k] * 5.0
    m.load_state_dict(p, strict=True)
    return m.to(cuda), p


def _step(m, x, noise=None, seed=None):
    m.zero_grad()
    if seed is not None:
        m.set_dropout_seed(seed)
    tok = m(x, noise=noise)[0] if noise is not None else m(x)[0]
    lora_ref.case_loss(tok).backward()
    torch.cuda.synchronize()
    return tok.detach().float().cpu(), grads_by_name(m)


_REF = {}


def _ref(key, p, x, noise, rate, case, masks, trainable=None, emulate=False):
    """(tokens, gradients) of the restatement; computed once per key and shared (read only)."""
    if key in _REF:
        return _REF[key]
    old = O._EMU[0]
    O._EMU[0] = emulate
    try:
        pv = {k: v.clone().requires_grad_(trainable is None or trainable(k)) for k, v in p.items()}
        tok = PD.vit_forward_keep(pv, x, noise, rate, case["patch_size"], case["num_heads"], case["num_layers"], masks)
        lora_ref.case_loss(tok).backward()
    finally:
        O._EMU[0] = old
    _REF[key] = tok.detach(), {k: v.grad for k, v in pv.items() if v.grad is not None}
    return _REF[key]


def _same(a, b):
    return torch.equal(a[0], b[0]) and a[1].keys() == b[1].keys() and all(torch.equal(a[1][k], b[1][k]) for k in a[1])


def _compare(got, want, tol, what):
    tok, grads = got
    r_tok, r_grads = want
    assert tok.shape == r_tok.shape
    print(what, "tokens", rel_err(tok, r_tok))
    assert rel_err(tok, r_tok) <= tol, (what, rel_err(tok, r_tok))
    assert set(grads) == set(r_grads), set(grads) ^ set(r_grads)
    worst = max((rel_err(grads[k], r_grads[k]), k) for k in grads)
    print(what, "worst gradient", worst)
    assert worst[0] <= tol, (what, worst)


# ---- 2. plan and module against the restatement, pinned noise -------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,tol", [("fp32", 1e-3), ("bf16", 5e-2)])
@pytest.mark.parametrize("name", ["L8", "L27"])
def test_backbone_vs_restatement(lib, cuda, name, dtype, tol):
    case, L, rate, K = CASES[name]
    m, p = _vit(case, dtype, cuda, rate)
    assert m.patch_keep == K == PD.keep_count(L, rate)
    x, noise = R.vit_case_input(case), PD.case_noise(case, L)
    got = _step(m.train(), x.to(cuda), noise.to(cuda))
    assert got[0].shape == (case["batch"], 1 + case["num_register_tokens"] + K, case["hidden_size"])
    emu = dtype == "bf16"
    want = _ref((name, emu), p, x, noise, rate, case, R.Ones(), emulate=emu)
    other, _ = _ref((name, "other"), p, x, -noise, rate, case, R.Ones())  # the K patches of HIGHEST noise instead
    assert rel_err(want[0], other) > 0.5, "another kept set gives unrelated patch rows: the comparison tells which patches were kept"
    _compare(got, want, tol, (name, dtype))
    # the ids the plan ranked are the yardstick's, all L of them
    plan = m._plans[(case["batch"], K)]
    ids_shuffle, ids_restore = PD.rank(noise.numpy())
    assert np.array_equal(plan.activation("ids_shuffle").cpu().numpy(), ids_shuffle)
    assert np.array_equal(plan.activation("ids_restore").cpu().numpy(), ids_restore)
    if dtype == "fp32":
        never = torch.from_numpy(~(ids_restore < K).any(axis=0))
        dpos = got[1]["patch_embedding.position_embeddings"][0]
        assert torch.count_nonzero(dpos[never]) == 0 and torch.count_nonzero(want[1]["patch_embedding.position_embeddings"][0][never]) == 0


@pytest.mark.parametrize("dtype,tol", [("fp32", 1e-3), ("bf16", 5e-2)])
@pytest.mark.parametrize("name", ["L8", "L27"])
def test_backbone_with_dropout_drop_path_and_lora(lib, cuda, name, dtype, tol):
    """Element dropout 0.25, drop path 0.5 (two blocks: q = [0, 0.5]) and the LoRA adapters on at the same time, seed pinned: site 0 and
    every block site act on the [B, 1 + R + K, D] tensor."""
    from headct_foundation_amd.misc import set_requires_grad_false
    case, L, rate, K = CASES[name]
    B = case["batch"]
    m, p = _vit(case, dtype, cuda, rate, p_drop=0.25, path=0.5, lora=True)
    set_requires_grad_false(m, lora=True)
    x, noise = R.vit_case_input(case), PD.case_noise(case, L)
    got = _step(m.train(), x.to(cuda), noise.to(cuda), SEED)
    assert m.last_dropout_seed == SEED
    emu = dtype == "bf16"
    want = _ref((name, "all", emu), p, x, noise, rate, case, P.PathMasks(SEED, 0.25, 0.5, case["num_layers"], B), trainable=lora_ref.trainable, emulate=emu)
    assert sum("lora" in k for k in got[1]) == 4 * case["num_layers"]
    _compare(got, want, tol, (name, dtype, "dropout + drop path + lora"))


# ---- 3. inertness ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_rate_zero_and_eval_mode_are_inert(lib, cuda, dtype):
    case, L, rate, K = CASES["L8"]
    x = R.vit_case_input(case).to(cuda)
    B = case["batch"]
    base, _ = _vit(case, dtype, cuda)                 # built without the argument
    zero, _ = _vit(case, dtype, cuda, 0.0)
    half, _ = _vit(case, dtype, cuda, rate)
    want = _step(base.train(), x)
    state = torch.cuda.get_rng_state(cuda)
    assert _same(want, _step(zero.train(), x))
    assert _same(want, _step(half.eval(), x))
    assert torch.equal(torch.cuda.get_rng_state(cuda), state), "neither forward drew from the device generator"
    assert list(zero._plans) == [(B, L)] and list(half._plans) == [(B, L)], "no new plan"
    dropped = _step(half.train(), x)                    # a training step that drops ...
    assert dropped[0].shape[1] == 1 + case["num_register_tokens"] + K
    assert not torch.equal(torch.cuda.get_rng_state(cuda), state), "default noise comes from the device generator"
    assert _same(want, _step(half.eval(), x))           # ... leaves the eval-mode model the model of every patch
    with torch.no_grad():
        assert torch.equal(half.eval()(x)[0], base.eval()(x)[0])


# ---- 4. both plans at one batch size -----------------------------------------------------------------------------------------------------
def test_train_eval_train_at_one_batch_size(lib, cuda):
    case, L, rate, K = CASES["L27"]
    B = case["batch"]
    m, _ = _vit(case, "fp32", cuda, rate)
    x, noise = R.vit_case_input(case).to(cuda), PD.case_noise(case, L).to(cuda)
    first = _step(m.train(), x, noise)
    m.zero_grad()
    tok = m.train()(x, noise=noise)[0]                  # forward of a training step ...
    with torch.no_grad():
        every = m.eval()(x)[0]                          # ... a validation forward at the same batch size in between ...
    assert every.shape[1] == 1 + case["num_register_tokens"] + L and set(m._plans) == {(B, K), (B, L)}
    lora_ref.case_loss(tok).backward()                  # ... and its backward still finds its activations
    torch.cuda.synchronize()
    assert _same(first, (tok.detach().float().cpu(), grads_by_name(m)))
    # a second forward of the SAME plan before the backward is still refused
    tok = m.train()(x, noise=noise)[0]
    m(x, noise=noise)
    with pytest.raises(_lib.HctError, match="stale"):
        lora_ref.case_loss(tok).backward()
    # the eval plan trains too: a backward through the full forward after the keep plan ran
    m.zero_grad()
    full = m.eval()(x)[0]
    m.train()(x, noise=noise)
    lora_ref.case_loss(full).backward()
    torch.cuda.synchronize()
    ref, _ = _vit(case, "fp32", cuda)
    assert _same(_step(ref.eval(), x), (full.detach().float().cpu(), grads_by_name(m)))


# ---- 5. determinism, default noise, lists ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_determinism_default_noise_and_lists(lib, cuda, dtype):
    case, L, rate, K = CASES["L8"]
    B = case["batch"]
    m, _ = _vit(case, dtype, cuda, rate)
    m.train()
    x, noise = R.vit_case_input(case).to(cuda), PD.case_noise(case, L).to(cuda)
    a = _step(m, x, noise)
    assert _same(a, _step(m, x, noise)), "two runs with the same noise agree bit for bit"
    assert _same(a, _step(m, [x[:1], x[1:]], noise)), "a list of parts is their concatenation"
    ids = lambda: m._plans[(B, K)].activation("ids_shuffle").cpu().numpy().copy()  # of the last forward
    torch.manual_seed(7)
    d = _step(m, x)
    ids_d = ids()
    e = _step(m, x)
    ids_e = ids()
    torch.manual_seed(7)
    f = _step(m, x)
    torch.manual_seed(7)
    drawn = torch.rand(B, L, device=cuda)
    assert _same(d, f) and _same(d, _step(m, x, drawn)), "the default noise is torch.rand(B, L, device=x.device) of the device generator"
    assert np.array_equal(ids_d, PD.rank(drawn.cpu().numpy())[0])
    assert not np.array_equal(ids_d[:, :K], ids_e[:, :K]) and not torch.equal(d[0], e[0]), "fresh noise per forward"
    with pytest.raises(_lib.HctError, match="noise"):
        m(x, noise=torch.rand(B, L + 1, device=cuda))


# ---- 6. C-level refusals -----------------------------------------------------------------------------------------------------------------
def test_plan_refusals(lib, cuda):
    case, L, rate, K = CASES["L8"]
    B = case["batch"]
    err = lambda: lib.hct_last_error_string().decode()
    m, _ = _vit(case, "fp32", cuda, rate)
    x, noise = R.vit_case_input(case).to(cuda), PD.case_noise(case, L).to(cuda)
    _step(m.train(), x, noise)
    _step(m.eval(), x)
    keep, full = m._plans[(B, K)], m._plans[(B, L)]
    assert lib.hct_mae_plan_len_keep(keep.handle) == K and lib.hct_mae_plan_len_keep(full.handle) == L
    ptrs = (C.c_void_p * 1)(x.data_ptr())
    assert lib.hct_vit_forward(keep.handle, x.data_ptr(), HCT_F32, _st()) != 0 and "hct_vit_forward_parts_keep" in err()
    assert lib.hct_vit_forward_parts(keep.handle, ptrs, 1, HCT_F32, _st()) != 0 and "patch_dropout" in err()
    assert lib.hct_vit_forward_parts_keep(full.handle, ptrs, 1, HCT_F32, noise.data_ptr(), _st()) != 0 and "without patch_dropout" in err()
    assert lib.hct_vit_forward_parts_keep(keep.handle, ptrs, 1, HCT_F32, None, _st()) != 0 and "hct_vit_forward_parts_keep" in err()
    three = (C.c_void_p * 3)(x.data_ptr(), x.data_ptr(), x.data_ptr())
    assert lib.hct_vit_forward_parts_keep(keep.handle, three, 3, HCT_F32, noise.data_ptr(), _st()) != 0 and "multiple of the number of parts" in err()
    torch.cuda.synchronize()


# ---- 7. main_downstream.py end to end ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("head,port", [("linear", "29671"), ("attentive", "29672")])
def test_main_downstream_with_patch_dropout(lib, cuda, tmp_path, head, port):
    """One epoch on synthetic data at --patch_dropout 0.5: the run ends with finite losses, its log names K of L, and the saved backbone in
    eval mode gives, on a validation batch, bit for bit the logits of a rate-0 backbone holding the same weights (every patch)."""
    from headct_foundation_amd.classifier import AttentionClassifier, LinearClassifier
    from headct_foundation_amd.data import SyntheticLabelled
    from headct_foundation_amd.dino_model import ViTBackbone
    dims = dict(in_chans=3, img_size=24, patch_size=12, hidden_size=48, mlp_dim=96, num_layers=2, num_heads=3, pos_embed="sincos", compute_dtype="fp32")
    vit = ViTBackbone(**dims)
    torch.save({"state_dict": {"module." + k: v for k, v in vit.state_dict().items()}, "epoch": 3}, tmp_path / "pre.pt")
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("MODEL:\n  NAME: vit\nMAE:\n  COMPUTE_DTYPE: fp32\n")
    opts = ["DATA.SYNTHETIC", "True", "DATA.SYNTHETIC_SAMPLES", "8", "VIT.INPUT_SIZE", "24", "VIT.PATCH_SIZE", "12", "VIT.HIDDEN_SIZE", "48",
            "VIT.MLP_DIM", "96", "VIT.NUM_LAYERS", "2", "VIT.NUM_HEADS", "3", "TRAIN.VAL_EVERY", "1", "MODEL.DIR", str(tmp_path / "out"),
            "MODEL.SAVE_NAME", "ft.pt", "LOG.OUTPUT_DIR", str(tmp_path / "log"), "PREDS_SAVE_NAME", "run"]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nproc-per-node", "1", "--master-port", port, os.path.join(ROOT, "main_downstream.py"),
           "--cfg", str(cfg), "--model_name", "vit", "--model_load_path", str(tmp_path / "pre.pt"), "--classifier", head, "--batch_size", "4",
           "--max_epochs", "1", "--grad_clip", "1.0", "--base_lr", "1e-4", "--patch_dropout", "0.5", "--opts"] + opts
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-4000:]
    assert "VIT.PATCH_DROPOUT 0.5: each training sample keeps 4 of 8 patches, 5 tokens per sample instead of 9" in log, log[-4000:]
    assert "Final test loss" in log and "Loss is" not in log, log[-4000:]  # ("Loss is ...": the engine's stop on a non-finite loss)
    sd = torch.load(tmp_path / "out" / "ft.pt", weights_only=True)["state_dict"]
    sd = {k[len("module."):] if k.startswith("module.") else k: v for k, v in sd.items()}
    a, b = ViTBackbone(**dims, patch_dropout=0.5), ViTBackbone(**dims)
    a.load_state_dict(sd, strict=True)
    b.load_state_dict(sd, strict=True)
    a, b = a.to(cuda).eval(), b.to(cuda).eval()
    cls = (LinearClassifier(48, 2) if head == "linear" else AttentionClassifier(dim=48, num_classes=2, num_heads=12, num_queries=1, compute_dtype="fp32"))
    cls.load_state_dict(torch.load(tmp_path / "out" / "ft_classifier.pt", weights_only=True)["state_dict"], strict=True)
    cls = cls.to(cuda).eval()
    v, _, _ = SyntheticLabelled(1, 4, 3, 24, 2, cuda, seed=1000).batches[0]
    with torch.no_grad():
        ta, tb = a(v)[0], b(v)[0]
        assert ta.shape == (4, 9, 48) and torch.equal(ta, tb)
        la, lb = cls(ta), cls(tb)
    assert torch.equal(la, lb) and torch.isfinite(la).all()
    with torch.no_grad():
        assert a.train()(v)[0].shape == (4, 5, 48), "the same weights in training mode keep 4 of 8 patches"
