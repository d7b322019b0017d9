"""GPU: the DINOv2 additions on the HIP path against tests/dino_v2_ref.py in float64 -- the two Sinkhorn-Knopp log-sum-exp passes one by
one, DINOLoss(centering="sinkhorn_knopp"), that the default mode and a zero KoLeo weight change nothing, hct_koleo_fwd / _bwd, the KoLeo
term through a tiny student, and the entry point with both switched on.  Outputs sit in NaN-filled buffers between guard bands, inputs
are followed by NaN rows.  Every comparison prints its figure before it asserts.

Observed on one MI355X (2026-10-20; the worst case of each group):
  hct_dino_sk_col_lse   largest error 3.05e-05 (130 x 2052, bf16, logits x 8: bound 2.14e-04); worst error / bound 0.235 over the 18 cases
  hct_dino_sk_row_lse   largest error 6.85e-07 (130 x 2052, bf16, logits x 8: bound 2.89e-04); worst error / bound 0.009 over the 10 cases
  two ranks against one lc 1.53e-05, lr 2.86e-06 (bound 1.50e-03); one rank against float64: lc 2.42e-05
  DINOLoss sinkhorn     fp32: loss 8.1e-07 (bar 2e-5), gradient 6.6e-07 (bar 1e-4); bf16: loss 4.5e-07, gradient 3.84e-03 (bar 6e-3)
  hct_koleo_fwd / _bwd  fp32: loss 6.0e-08, dist 1.5e-07, inv_norm 1.1e-07, dx 8.9e-07 (bound 2.4e-05 at d_min 0.1); bf16 rows: loss 8.6e-08,
                        dist 1.7e-07, dx 3.73e-03 (bound 4.01e-03: the bf16 store's 2^-8 against the row's largest element)
  through the model     class tokens at distance >= 0.994, margin 1.8e-03; error / tolerance 0.072
"""
import logging
import math
import os
import re
import subprocess
import sys

import pytest
import torch

from headct_foundation_amd import _lib
from tests import dino_v2_ref as R
from tests.test_assembly_kernels_gpu import _Out, _bits, _code, _st
from tests.util import rel_err

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16 = torch.float32, torch.bfloat16
GUARD_ROWS = 4
LOSS_BAR, GRAD_BAR = 2e-5, {F32: 1e-4, BF16: 6e-3}  # what tests/test_dino_gpu.py holds hct_dino_loss to


def _in(t, dev):
    """`t` on the device with GUARD_ROWS rows of NaN behind it."""
    buf = torch.full((t.shape[0] + GUARD_ROWS,) + tuple(t.shape[1:]), float("nan"), dtype=t.dtype, device=dev)
    buf[:t.shape[0]] = t.to(dev)
    return buf[:t.shape[0]]


def _ws(nbytes, dev):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=dev)


# ---- the two passes, one by one ---------------------------------------------------------------------------------------------------------
SK_CASES = [(R_, K, dt, 2.0, given) for (R_, K) in R.SK_SHAPES for dt in (F32, BF16) for given in (False, True)] + [(4, 1028, F32, 8.0, True), (130, 2052, BF16, 8.0, False)]


def _sk_case(R_, K, dt, scale):
    t = R.sk_inputs(R_, K, seed=101 + R_ + K, scale=scale, dtype=dt)  # the reference reads the rounded values
    inv = R.inv_temp32(0.04)
    _, lr1, lc1 = R.sk_log(t, 0.04, n_iters=1, inv_temp=inv)  # shifts of realistic size: the reference's own after one round, as fp32
    return t, inv, lr1.float(), lc1.float()


@pytest.mark.parametrize("R_,K,dt,scale,lr_given", SK_CASES)
def test_sk_col_lse(lib, cuda, R_, K, dt, scale, lr_given):
    t, inv, lr, _ = _sk_case(R_, K, dt, scale)
    lr = lr if lr_given else None
    want = R.col_lse(t, inv, lr)
    td, lrd = _in(t, cuda), (_in(lr, cuda) if lr_given else None)
    out, ws = _Out((K,), F32, cuda), _ws(lib.hct_dino_sk_workspace_bytes(R_, K), cuda)
    _lib.check(lib.hct_dino_sk_col_lse(td.data_ptr(), _code(dt), R_, K, inv, _lib.ptr(lrd), out.ptr, ws.data_ptr(), ws.numel(), _st()), "hct_dino_sk_col_lse")
    torch.cuda.synchronize()
    got = out.result().double()
    arg = float((t.double() * inv + (lr.double()[:, None] if lr_given else 0.0)).abs().max())
    bound = R.lse_bound(arg, 16, want.abs().numpy())
    err = (got - want).abs().numpy()
    print(f"col_lse {R_}x{K} {dt} scale {scale} lr {lr_given}: max error {err.max():.2e}, smallest bound {bound.min():.2e}, worst error / bound {(err / bound).max():.3f}")
    assert bool(torch.isfinite(got).all()) and bool((err <= bound).all())


@pytest.mark.parametrize("R_,K,dt,scale,_unused", SK_CASES[:16:2] + SK_CASES[16:])
def test_sk_row_lse(lib, cuda, R_, K, dt, scale, _unused):
    t, inv, _, lc = _sk_case(R_, K, dt, scale)
    want = R.row_lse(t, inv, lc)
    td, lcd = _in(t, cuda), _in(lc, cuda)
    out = _Out((R_,), F32, cuda)
    _lib.check(lib.hct_dino_sk_row_lse(td.data_ptr(), _code(dt), R_, K, inv, lcd.data_ptr(), out.ptr, _st()), "hct_dino_sk_row_lse")
    torch.cuda.synchronize()
    got = out.result().double()
    arg = float((t.double() * inv + lc.double()[None, :]).abs().max())
    bound = R.lse_bound(arg, 4 * -(-K // 1024), want.abs().numpy())
    err = (got - want).abs().numpy()
    print(f"row_lse {R_}x{K} {dt} scale {scale}: max error {err.max():.2e}, smallest bound {bound.min():.2e}, worst error / bound {(err / bound).max():.3f}")
    assert bool(torch.isfinite(got).all()) and bool((err <= bound).all())


def test_two_emulated_ranks_are_one_rank_on_the_concatenated_batch(lib, cuda):
    """The column pass on each half, combine_lse over the list, the row pass on each half with N = all rows, three rounds: lc and the
    two halves of lr are those of one rank on the whole batch.  Each pass inherits the error of the one before and adds its own bound b,
    so after n rounds lr is within 2 n b of the exact value; two such computations are compared: 4 n b."""
    from headct_foundation_amd.dino import combine_lse, sinkhorn_knopp_logs, sk_col_lse, sk_row_lse
    R_, K, n = 38, 1028, 3  # 19 rows per half: a full 16-row split and a ragged one on each "rank", 16 + 16 + 6 on the whole batch
    t = R.sk_inputs(R_, K, seed=7)
    inv = R.inv_temp32(0.04)
    whole = _in(t, cuda)
    halves = [_in(t[:19], cuda), _in(t[19:], cuda)]
    lc1, lr1, log_n = sinkhorn_knopp_logs(whole, 0.04, n)
    lrs = [None, None]
    for _ in range(n):
        lc = -math.log(K) - combine_lse([sk_col_lse(h, inv, l) for h, l in zip(halves, lrs)])
        lrs = [-math.log(R_) - sk_row_lse(h, inv, lc) for h in halves]
    torch.cuda.synchronize()
    assert log_n == math.log(R_)
    q_ref, lr_ref, lc_ref = R.sk_log(t, 0.04, n, inv_temp=inv)
    arg = float((t.double() * inv).abs().max()) + float(lr_ref.abs().max()) + float(lc_ref.abs().max())
    b = float(R.lse_bound(arg, 16, arg))
    e_lc, e_lr = float((lc.cpu() - lc1.cpu()).abs().max()), float((torch.cat(lrs).cpu() - lr1.cpu()).abs().max())
    print(f"two ranks vs one: lc {e_lc:.2e}, lr {e_lr:.2e}, bound {4 * n * b:.2e}; one rank vs float64: lc {float((lc1.cpu().double() - lc_ref).abs().max()):.2e}")
    assert e_lc <= 4 * n * b and e_lr <= 4 * n * b
    assert float((lc1.cpu().double() - lc_ref).abs().max()) <= 2 * n * b and float((lr1.cpu().double() - lr_ref).abs().max()) <= 2 * n * b


# ---- DINOLoss(centering="sinkhorn_knopp") -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("K", [1028, 4100])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("V", [2, 4])
def test_dino_loss_sinkhorn_knopp(lib, cuda, V, B, K, dt):
    from headct_foundation_amd.dino import DINOLoss
    student = R.sk_inputs(V * B, K, seed=201, dtype=dt)
    teacher = R.sk_inputs(2 * B, K, seed=202, dtype=dt)
    q, _, _ = R.sk_log(teacher, 0.04, 3)
    want, dwant = R.dino_loss_from_q(student, q, V, 0.1)
    crit = DINOLoss(K, V, 0.04, 0.04, 0, 5, centering="sinkhorn_knopp").to(cuda)
    crit.center.copy_(R.sk_inputs(1, K, seed=203, scale=0.3))
    center0 = crit.center.clone()
    s = _in(student, cuda).requires_grad_(True)
    loss = crit(s, _in(teacher, cuda), 0)
    (loss * 3.0).backward()  # the incoming gradient scales dstudent
    torch.cuda.synchronize()
    e_loss, e_grad = abs(float(loss) - float(want)) / abs(float(want)), rel_err(s.grad.float() / 3.0, dwant)
    print(f"sinkhorn loss V{V} B{B} K{K} {dt}: loss {e_loss:.2e} / {LOSS_BAR:.0e}, gradient {e_grad:.2e} / {GRAD_BAR[dt]:.0e}")
    assert e_loss < LOSS_BAR and e_grad < GRAD_BAR[dt]
    assert torch.equal(_bits(crit.center), _bits(center0)), "the centre is not to be touched in this mode"
    with torch.no_grad():  # validation: the same mode, no gradient storage
        again = crit(s.detach(), _in(teacher, cuda), 0)
    assert float(again) == float(loss)


# ---- inertness ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, BF16])
def test_default_mode_is_hct_dino_loss_bit_for_bit(lib, cuda, dt):
    from headct_foundation_amd.dino import DINOLoss
    V, B, K = 4, 3, 4100
    student, teacher = R.sk_inputs(V * B, K, seed=301, dtype=dt).to(cuda), R.sk_inputs(2 * B, K, seed=302, dtype=dt).to(cuda)
    center = R.sk_inputs(1, K, seed=303, scale=0.3).to(cuda)
    crit = DINOLoss(K, V, 0.04, 0.04, 0, 5).to(cuda)
    assert crit.centering == "centering"
    crit.center.copy_(center)
    s = student.clone().requires_grad_(True)
    loss = crit(s, teacher, 0)
    loss.backward()
    # the same call by hand
    ws = _ws(lib.hct_dino_loss_workspace_bytes(V, B, K), cuda)
    l2, g2, csum = torch.empty(1, device=cuda), torch.empty_like(student), torch.empty(K, device=cuda)
    _lib.check(lib.hct_dino_loss(student.data_ptr(), teacher.data_ptr(), _code(dt), V, B, K, center.data_ptr(), 0.1, 0.04, l2.data_ptr(), g2.data_ptr(), None,
                                 csum.data_ptr(), ws.data_ptr(), ws.numel(), _st()), "hct_dino_loss")
    c2 = center.clone()
    _lib.check(lib.hct_dino_center_update(c2.data_ptr(), csum.data_ptr(), K, 0.9, float(2 * B), _st()), "hct_dino_center_update")
    torch.cuda.synchronize()
    assert torch.equal(_bits(loss.detach().reshape(1)), _bits(l2)) and torch.equal(_bits(s.grad), _bits(g2)) and torch.equal(_bits(crit.center), _bits(c2))


def _tiny(cuda, extra=()):
    import main_pretrain_dino as M
    from headct_foundation_amd.dino import DINOLoss, SyntheticCrops
    old = sys.argv
    try:
        sys.argv = ["main_pretrain_dino.py", "--cfg", os.path.join(ROOT, "configs/dino/dino_tiny_plumbing.yaml"), *extra]
        config = M.parse_option()[1]
    finally:
        sys.argv = old
    torch.manual_seed(3)
    student = M.build_pair(config, cuda, return_cls=config.DINO.KOLEO_WEIGHT > 0)
    teacher = M.build_pair(config, cuda)
    teacher.load_state_dict(student.state_dict())
    for p in teacher.parameters():
        p.requires_grad_(False)
    n_crops = 2 + config.DINO.LOCAL_CROP_NUM
    loader = SyntheticCrops(2, config.DATA.BATCH_SIZE, n_crops, config.VIT.IN_CHANS, config.VIT.INPUT_SIZE, cuda, 0)
    crit = DINOLoss(config.DINO.HEAD_N_PROTOTYPES, n_crops, 0.04, 0.07, 1, 2, centering=config.DINO.CENTERING, sk_iters=config.DINO.SK_ITERS).to(cuda)
    return M, config, student.train(), teacher.train(), loader, crit


def _epoch(config, student, teacher, loader, crit, cuda):
    from engine_pretrain_dino import train_one_epoch
    from headct_foundation_amd.dino import DinoOptimizer, wd_cosine_scheduler
    from headct_foundation_amd.lr_sched import get_cosine_schedule_with_warmup
    opt = DinoOptimizer(student, lr=1e-3, weight_decay=0.04)
    sched = get_cosine_schedule_with_warmup(opt.primary, 1, 4, lr_end=1e-6)
    wd, mom = wd_cosine_scheduler(0.04, 0.4, 2, len(loader)), wd_cosine_scheduler(0.99, 1.0, 2, len(loader))
    return train_one_epoch(config, student, loader, opt, sched, wd, mom, 0, 2, crit, momentum_model=teacher, logger=logging.getLogger("dino_v2"), device=cuda)


def test_zero_koleo_weight_changes_nothing(lib, cuda, caplog):
    from engine_pretrain_dino import _forward_loss
    M, config, student, teacher, loader, crit = _tiny(cuda)
    assert config.DINO.KOLEO_WEIGHT == 0.0 and student.return_cls is False
    crops = next(iter(loader))
    with torch.no_grad():
        out = student(list(crops))
        assert list(out) == ["dino_output"]
        by_hand = crit(out["dino_output"].float(), teacher(list(crops[:2]))["dino_output"].float(), 0)
    crit.center.zero_()
    loss = _forward_loss(student, teacher, crops, crit, 0, cuda)
    assert float(loss) == float(by_hand)
    crit.center.zero_()
    with caplog.at_level(logging.INFO, logger="dino_v2"):
        stats = _epoch(config, student, teacher, loader, crit, cuda)
    assert sorted(stats) == ["loss", "lr", "wd"] and "koleo" not in caplog.text and "dino_loss" not in caplog.text
    assert re.search(r"Epoch 1/2 \[1/2\]  Loss: \d+\.\d{4}$", caplog.text, flags=re.M)


def test_positive_koleo_weight_adds_two_meters(lib, cuda, caplog):
    M, config, student, teacher, loader, crit = _tiny(cuda, ("--koleo_weight", "0.1", "--centering", "sinkhorn_knopp"))
    with caplog.at_level(logging.INFO, logger="dino_v2"):
        stats = _epoch(config, student, teacher, loader, crit, cuda)
    assert sorted(stats) == ["dino_loss", "koleo_loss", "loss", "lr", "wd"] and all(math.isfinite(v) for v in stats.values())
    assert abs(stats["loss"] - (stats["dino_loss"] + 0.1 * stats["koleo_loss"])) <= 1e-5 * abs(stats["loss"])
    assert "koleo_loss:" in caplog.text and "dino_loss:" in caplog.text
    assert not bool(crit.center.any())  # Sinkhorn-Knopp through the engine leaves the centre where it was


# ---- hct_koleo_fwd / hct_koleo_bwd ------------------------------------------------------------------------------------------------------
def _koleo_call(lib, cuda, x, tokens):
    """The kernels on rows `x` [n, D]: contiguous (tokens = 1) or as the class-token rows of a NaN-filled [n, tokens, D] tensor; dx goes
    to the same layout.  Returns the outputs and the whole dx buffer."""
    n, D = x.shape
    xin = torch.full((n + GUARD_ROWS, tokens, D), float("nan"), dtype=x.dtype, device=cuda)
    xin[:n, 0] = x.to(cuda)
    dxo = _Out((n, tokens, D), x.dtype, cuda)
    o = dict(loss=_Out((1,), F32, cuda), nn=_Out((n,), torch.int32, cuda), dist=_Out((n,), F32, cuda), inv=_Out((n,), F32, cuda))
    g = torch.tensor([1.7], device=cuda)
    _lib.check(lib.hct_koleo_fwd(xin.data_ptr(), _code(x.dtype), n, D, tokens * D, o["loss"].ptr, o["nn"].ptr, o["dist"].ptr, o["inv"].ptr, _st()), "hct_koleo_fwd")
    _lib.check(lib.hct_koleo_bwd(xin.data_ptr(), _code(x.dtype), n, D, tokens * D, o["nn"].ptr, o["dist"].ptr, o["inv"].ptr, g.data_ptr(), dxo.ptr, tokens * D, _st()),
               "hct_koleo_bwd")
    torch.cuda.synchronize()
    return {k: v.result() for k, v in o.items()}, dxo.result()


@pytest.mark.parametrize("tokens", [1, 3])
@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("n,D", R.KOLEO_SHAPES)
def test_koleo_kernels(lib, cuda, n, D, dt, tokens):
    x = R.koleo_inputs(n, D, seed=21, dtype=dt)
    loss, dx, idx, d, margin = R.koleo(x, dloss=1.7)  # the reference reads the rounded values
    assert margin >= 1e-3, "the reference's own choice of neighbours is not clear on these inputs"
    if n >= 6:
        assert idx[1:4].tolist() == [0, 0, 0]  # three rows choose row 0: the gather path
    got, dx_all = _koleo_call(lib, cuda, x, tokens)
    assert torch.equal(got["nn"].long(), idx)
    d_min = float(d.min())
    b32, b = R.koleo_bound(d_min), R.koleo_bound(d_min, dt)
    e_loss = abs(float(got["loss"]) - float(loss)) / max(1.0, abs(float(loss)))
    e_dist = float(((got["dist"].double() - d).abs() / d).max())
    e_inv = float((got["inv"].double() * x.double().norm(dim=1) - 1.0).abs().max())
    gdx = dx_all[:, 0].double()
    e_dx = float(((gdx - dx).abs().max(dim=1).values / dx.abs().max(dim=1).values).max())
    print(f"koleo {n}x{D} {dt} tokens {tokens}: loss {e_loss:.2e} dist {e_dist:.2e} inv_norm {e_inv:.2e} / {b32:.2e}; dx {e_dx:.2e} / {b:.2e}; margin {margin:.1e}")
    assert e_loss <= b32 and e_dist <= b32 and e_inv <= R.KOLEO_BAR[F32]
    assert bool(((gdx - dx).abs() <= b * dx.abs().max(dim=1, keepdim=True).values).all())  # element by element, on the scale of its row
    if tokens > 1:
        assert bool(torch.isnan(dx_all[:, 1:]).all()), "dx was written between the class-token rows"


def test_koleo_loss_function_on_a_strided_view(lib, cuda):
    """koleo_loss on tokens[:, 0, :] is the kernels' result, and its autograd gradient lands in the class-token rows only."""
    from headct_foundation_amd.dino import HctError, koleo_loss
    n, T, D = 64, 5, 768
    x = R.koleo_inputs(n, D, seed=22, dtype=BF16)
    loss, dx, idx, d, margin = R.koleo(x, dloss=0.5)
    assert margin >= 1e-3
    tokens = torch.randn(n, T, D, device=cuda).to(BF16)
    tokens[:, 0] = x.to(cuda)
    tokens.requires_grad_(True)
    out = koleo_loss(tokens[:, 0, :])
    (out * 0.5).backward()
    torch.cuda.synchronize()
    b = R.koleo_bound(float(d.min()), BF16)
    g = tokens.grad.cpu()
    assert abs(float(out) - float(loss)) <= R.koleo_bound(float(d.min())) * max(1.0, abs(float(loss)))
    assert bool(((g[:, 0].double() - dx).abs() <= b * dx.abs().max(dim=1, keepdim=True).values).all()) and not bool(g[:, 1:].any())
    with pytest.raises(HctError, match="n >= 2"):
        koleo_loss(tokens[:1, 0, :])
    with pytest.raises(HctError, match="n >= 2"):
        koleo_loss(tokens[:, 0, :6])


# ---- the KoLeo term through the model -----------------------------------------------------------------------------------------------------
def test_koleo_gradient_adds_to_the_heads_at_the_class_tokens(lib, cuda):
    """A tiny fp32 student (one block, width 64, 9 tokens, 4 volumes per crop): the gradient that reaches the class tokens with weight w is
    the gradient at weight 0 plus w times the reference's KoLeo gradient of those tokens, and the backbone's parameter gradients move."""
    from engine_pretrain_dino import _forward_loss
    from headct_foundation_amd.dino import DINOLoss
    from headct_foundation_amd.dino_model import DINOHead, MultiCropWrapper, ViTBackbone
    torch.manual_seed(5)
    B, V, w = 4, 3, 0.1
    mk = lambda: MultiCropWrapper(ViTBackbone(in_chans=1, img_size=24, patch_size=12, hidden_size=64, mlp_dim=128, num_layers=1, num_heads=4,
                                              compute_dtype="fp32"),
                                  DINOHead(64, 256, hidden_dim=64, bottleneck_dim=32, compute_dtype="fp32"), return_cls=True).to(cuda).train()
    student, teacher = mk(), mk()
    crops = [torch.randn(B, 1, 24, 24, 24, device=cuda) for _ in range(V)]
    crit = DINOLoss(256, V, 0.04, 0.04, 0, 2).to(cuda)
    seen = {}

    class Hooked(torch.nn.Module):
        def forward(self, x):
            out = student(x)
            seen["cls"] = out["cls_tokens"].detach().clone()
            out["cls_tokens"].register_hook(lambda g: seen.__setitem__("grad", g.detach().clone()))
            return out

    def run(weight):
        for p in student.parameters():
            p.grad = None
        crit.center.zero_()
        _forward_loss(Hooked(), teacher, crops, crit, 0, cuda, weight).backward()
        torch.cuda.synchronize()
        return seen["grad"].cpu().double(), {k: p.grad.detach().clone() for k, p in student.backbone.named_parameters() if p.grad is not None}

    g0, p0 = run(0.0)
    gw, pw = run(w)
    cls = seen["cls"].cpu()
    assert cls.dtype == F32 and tuple(cls.shape) == (V * B, 64)
    want, d_min, margin = torch.zeros(V * B, 64, dtype=torch.float64), math.inf, math.inf
    for c in range(2):
        _, dx, _, d, m = R.koleo(cls[c * B:(c + 1) * B])
        want[c * B:(c + 1) * B] = dx
        d_min, margin = min(d_min, float(d.min())), min(margin, m)
    # a fair comparison needs the reference's neighbours to be clear of the kernel's own rounding: a cosine of two unit rows of 64 elements is
    # off by at most (64 + 8) 2^-24 = 4.3e-6 in fp32, so two candidates 5e-5 apart cannot swap
    print(f"class tokens: smallest distance {d_min:.3e}, smallest margin {margin:.3e}")
    assert margin >= 5e-5
    b = R.koleo_bound(d_min)
    scale = (w * want).abs().max(dim=1, keepdim=True).values
    err = (gw - (g0 + w * want)).abs()
    tol = b * scale + 2 * R.EPS32 * g0.abs()  # the sum of the two gradients is rounded once more
    print(f"additivity: worst error / tolerance {float((err / tol.clamp_min(1e-300)).max()):.3f}, koleo share {float(scale.max()):.2e} against {float(g0.abs().max()):.2e}")
    assert bool((err[:2 * B] <= tol[:2 * B]).all()) and torch.equal(gw[2 * B:], g0[2 * B:])
    assert p0.keys() == pw.keys() and any(not torch.equal(p0[k], pw[k]) for k in p0)


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
def test_entry_point_with_sinkhorn_knopp_and_koleo(cuda, tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1", "--master-addr", "127.0.0.1", "--master-port", "29541",
           os.path.join(ROOT, "main_pretrain_dino.py"), "--local_rank", "0", "--model_name", "dino", "--batch_size", "2", "--max_epochs", "1",
           "--base_lr", "5e-4", "--cfg", os.path.join(ROOT, "configs/dino/dino_tiny_plumbing.yaml"), "--optimizer", "AdamW", "--scheduler", "cosine",
           "--centering", "sinkhorn_knopp", "--koleo_weight", "0.1",
           "--opts", "DATA.SYNTHETIC_SAMPLES", "4", "MODEL.DIR", str(tmp_path / "ckpt"), "LOG.OUTPUT_DIR", str(tmp_path / "log"), "OUTPUT", str(tmp_path / "json")]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = re.findall(r"Epoch 1/1 \[(\d)/2\]  Loss: (\S+)  dino_loss: (\S+)  koleo_loss: (\S+)", r.stdout)
    assert [l[0] for l in lines] == ["1", "2"] and all(math.isfinite(float(v)) for l in lines for v in l[1:])
    assert "train completed" in r.stdout and "test completed" in r.stdout
    assert "CENTERING: sinkhorn_knopp" in r.stdout and "KOLEO_WEIGHT: 0.1" in r.stdout
