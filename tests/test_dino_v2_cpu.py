"""CPU: the DINOv2 additions off the GPU -- the yardstick tests/dino_v2_ref.py against itself (log-domain Sinkhorn-Knopp = the direct
form, finite where fp32 overflows) and against torch autograd (KoLeo), `combine_lse` on plain vectors and over two gloo ranks, the config
keys, the entry point's flags, DINOLoss's default and refusals, and that the new symbols are declared, bound and exported."""
import math
import os
import re
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F

from headct_foundation_amd import _lib
from headct_foundation_amd.dino import DINOLoss, HctError, combine_lse, koleo_loss
from tests import dino_v2_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- Sinkhorn-Knopp: the two forms of the yardstick -----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.SK_SHAPES)
def test_sk_log_is_sk_direct(shape):
    t = R.sk_inputs(*shape, seed=11, scale=1.0)
    for temp in (0.04, 0.07):
        q, lr, lc = R.sk_log(t, temp)
        want = R.sk_direct(t, temp)
        rel = float(((q - want).abs() / want).max())
        print(shape, temp, f"max relative difference {rel:.2e}")
        assert rel <= 1e-12
        assert float((q.sum(dim=1) - 1.0).abs().max()) <= 1e-12  # every sample's row sums to 1
        assert lr.shape == (shape[0],) and lc.shape == (shape[1],)


def test_sk_log_is_finite_where_fp32_direct_is_not():
    t = R.sk_inputs(4, 1028, seed=12, scale=8.0)
    assert float(t.max()) / 0.04 > 88.0
    assert not bool(torch.isfinite(R.sk_direct(t, 0.04, dtype=torch.float32)).all())
    q, lr, lc = R.sk_log(t, 0.04)
    assert all(bool(torch.isfinite(v).all()) for v in (q, lr, lc))
    assert float((q.sum(dim=1) - 1.0).abs().max()) <= 1e-12


def test_dino_loss_from_q_is_the_centred_loss_for_a_softmax_q():
    """With q = softmax((t - c) / T) the restatement is the reference's centred DINO loss (oracle/dino_oracle.py)."""
    from oracle import dino_oracle as D
    V, B, K = 4, 3, 20
    s, t, c = R.sk_inputs(V * B, K, 1), R.sk_inputs(2 * B, K, 2), R.sk_inputs(1, K, 3, scale=0.3)
    q = torch.softmax((t.double() - c.double()) / 0.05, dim=-1)
    loss, grad = R.dino_loss_from_q(s, q, V, 0.1)
    so = s.double().clone().requires_grad_(True)
    want = D.dino_loss(so, t.double(), c.double(), V, 0.1, 0.05)
    want.backward()
    assert abs(float(loss) - float(want)) <= 1e-12 and float((grad - so.grad).abs().max()) <= 1e-12


# ---- KoLeo: the yardstick against autograd ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,D", R.KOLEO_SHAPES)
def test_koleo_ref_is_torch_autograd(n, D):
    x = R.koleo_inputs(n, D, seed=21).double()
    loss, dx, idx, d, margin = R.koleo(x, dloss=1.7)
    leaf = x.clone().requires_grad_(True)
    xh = F.normalize(leaf, eps=1e-8, p=2, dim=-1)
    with torch.no_grad():
        dots = xh @ xh.t()
        dots.view(-1)[:: n + 1].fill_(-1)
        I = dots.argmax(dim=1)
    want = -torch.log(F.pairwise_distance(xh, xh[I], eps=1e-8) + 1e-8).mean()
    (grad,) = torch.autograd.grad(want * 1.7, leaf)
    assert torch.equal(idx, I) and abs(float(loss) - float(want)) <= 1e-12
    assert float((dx - grad).abs().max()) <= 1e-12 * max(1.0, float(grad.abs().max()))
    if n >= 6:  # the fan: rows 1, 2 and 3 all choose row 0
        assert idx[1:4].tolist() == [0, 0, 0] and int(idx[0]) == 1


# ---- combine_lse -------------------------------------------------------------------------------------------------------------------------
def test_combine_lse_of_two_halves_is_the_whole_batch():
    t = R.sk_inputs(10, 36, seed=31, scale=3.0).double() / 0.04
    whole = torch.logsumexp(t, dim=0)
    halves = [torch.logsumexp(t[:5], dim=0), torch.logsumexp(t[5:], dim=0)]
    assert float((combine_lse(halves) - whole).abs().max()) <= 1e-12
    assert float((combine_lse(tuple(halves[::-1])) - whole).abs().max()) <= 1e-12
    assert combine_lse(whole) is whole  # no process group: the identity
    f = combine_lse([h.float() for h in halves])
    assert f.dtype == torch.float32 and float((f.double() - whole).abs().max()) <= 4 * R.EPS32 * float(whole.abs().max())


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _lse_worker(rank, world, port):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        t = R.sk_inputs(10, 36, seed=31, scale=3.0).double() / 0.04
        mine = torch.logsumexp(t[5 * rank:5 * rank + 5], dim=0)
        keep = mine.clone()
        got = combine_lse(mine)
        assert torch.equal(mine, keep), "the local vector is not to be overwritten"
        assert float((got - torch.logsumexp(t, dim=0)).abs().max()) <= 1e-12
    finally:
        dist.destroy_process_group()


def test_combine_lse_world2_gloo():
    ctx = mp.get_context("spawn")
    port = _free_port()
    procs = [ctx.Process(target=_lse_worker, args=(r, 2, port)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(120)
        assert p.exitcode == 0


# ---- configuration, entry point, module defaults --------------------------------------------------------------------------------------
def _parse(monkeypatch, *extra):
    import main_pretrain_dino as M
    monkeypatch.setattr(sys, "argv", ["main_pretrain_dino.py", "--cfg", os.path.join(ROOT, "configs/dino/dino_tiny_plumbing.yaml"), *extra])
    return M.parse_option()[1]


def test_config_keys_defaults_and_flags(monkeypatch):
    from config import _C
    assert (_C.DINO.CENTERING, _C.DINO.SK_ITERS, _C.DINO.KOLEO_WEIGHT) == ("centering", 3, 0.0)
    c = _parse(monkeypatch)
    assert (c.DINO.CENTERING, c.DINO.SK_ITERS, c.DINO.KOLEO_WEIGHT) == ("centering", 3, 0.0)
    c = _parse(monkeypatch, "--centering", "sinkhorn_knopp", "--koleo_weight", "0.1")
    assert (c.DINO.CENTERING, c.DINO.KOLEO_WEIGHT) == ("sinkhorn_knopp", 0.1)
    c = _parse(monkeypatch, "--koleo_weight", "0", "--opts", "DINO.KOLEO_WEIGHT", "0.5", "DINO.SK_ITERS", "5")  # 0 reaches the config
    assert (c.DINO.KOLEO_WEIGHT, c.DINO.SK_ITERS) == (0.0, 5)
    for bad in (("--centering", "softmax"), ("--koleo_weight", "-0.1"), ("--opts", "DINO.SK_ITERS", "0")):
        with pytest.raises(ValueError, match="DINO"):
            _parse(monkeypatch, *bad)


def test_entry_point_builds_the_student_with_class_tokens_only_under_koleo(monkeypatch):
    import main_pretrain_dino as M
    cpu = torch.device("cpu")
    off, on = _parse(monkeypatch), _parse(monkeypatch, "--koleo_weight", "0.1")
    assert M.build_pair(off, cpu).return_cls is False
    student = M.build_pair(on, cpu, return_cls=on.DINO.KOLEO_WEIGHT > 0)
    assert student.return_cls is True and list(student.state_dict()) == list(M.build_pair(off, cpu).state_dict())


def test_dino_loss_modes_and_refusals():
    crit = DINOLoss(16, 4, 0.04, 0.07, 3, 10)
    assert crit.centering == "centering" and crit.sk_iters == 3
    sk = DINOLoss(16, 4, 0.04, 0.07, 3, 10, centering="sinkhorn_knopp", sk_iters=2)
    assert sk.centering == "sinkhorn_knopp" and sk.sk_iters == 2
    assert list(sk.state_dict()) == list(crit.state_dict()) == ["center"]  # the buffer stays: checkpoints keep their layout
    sk.update_center  # still there
    with pytest.raises(ValueError, match="centering"):
        DINOLoss(16, 4, 0.04, 0.07, 3, 10, centering="softmax")
    with pytest.raises(ValueError, match="sk_iters"):
        DINOLoss(16, 4, 0.04, 0.07, 3, 10, centering="sinkhorn_knopp", sk_iters=0)
    with pytest.raises(HctError, match="no CPU fallback"):
        sk(torch.zeros(8, 16), torch.zeros(4, 16), 0)
    with pytest.raises(HctError, match="no CPU fallback"):
        koleo_loss(torch.zeros(4, 8))


def test_multicrop_wrapper_default_has_no_class_tokens():
    import inspect
    from headct_foundation_amd.dino_model import MultiCropWrapper
    assert inspect.signature(MultiCropWrapper.__init__).parameters["return_cls"].default is False


# ---- the library --------------------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("hct_dino_sk_workspace_bytes", "hct_dino_sk_col_lse", "hct_dino_sk_row_lse", "hct_dino_loss_sk_workspace_bytes", "hct_dino_loss_sk",
               "hct_koleo_fwd", "hct_koleo_bwd")


def test_new_symbols_are_declared_bound_and_exported(lib):
    with open(os.path.join(ROOT, "include", "headct_hip.h")) as f:
        hdr = f.read()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b" + s + r"\s*\(", hdr) and s in _lib.exported_symbols() and hasattr(lib, s), s
    from headct_foundation_amd import build
    assert "koleo.hip" in build.SOURCES


def test_host_visible_arguments_are_refused_before_any_launch(lib):
    HCT_E_BADARG, HCT_E_WORKSPACE = -1, -3  # include/headct_hip.h
    fake = 4096  # never dereferenced: every call below returns before a launch
    assert lib.hct_dino_sk_workspace_bytes(16, 1024) == 1024 * 8 and lib.hct_dino_sk_workspace_bytes(17, 1024) == 2 * 1024 * 8
    assert lib.hct_dino_loss_sk_workspace_bytes(10, 64, 65536) < lib.hct_dino_loss_workspace_bytes(10, 64, 65536)
    for rc in (lib.hct_dino_sk_col_lse(fake, 0, 4, 6, 25.0, None, fake, fake, 1 << 20, None), lib.hct_dino_sk_col_lse(fake, 0, 0, 8, 25.0, None, fake, fake, 1 << 20, None),
               lib.hct_dino_sk_col_lse(fake, 0, 4, 8, 0.0, None, fake, fake, 1 << 20, None), lib.hct_dino_sk_col_lse(None, 0, 4, 8, 25.0, None, fake, fake, 1 << 20, None)):
        assert rc == HCT_E_BADARG and b"hct_dino_sk_col_lse" in lib.hct_last_error_string()
    assert lib.hct_dino_sk_col_lse(fake, 0, 4, 8, 25.0, None, fake, fake, 8, None) == HCT_E_WORKSPACE
    for rc in (lib.hct_dino_sk_row_lse(fake, 0, 4, 6, 25.0, fake, fake, None), lib.hct_dino_sk_row_lse(fake, 0, 4, 8, 25.0, None, fake, None)):
        assert rc == HCT_E_BADARG and b"hct_dino_sk_row_lse" in lib.hct_last_error_string()
    for rc in (lib.hct_dino_loss_sk(fake, fake, 0, 1, 2, 8, fake, fake, 0.0, 0.1, 0.04, fake, None, None, fake, 1 << 20, None),
               lib.hct_dino_loss_sk(fake, fake, 0, 2, 2, 6, fake, fake, 0.0, 0.1, 0.04, fake, None, None, fake, 1 << 20, None),
               lib.hct_dino_loss_sk(fake, fake, 0, 2, 2, 8, None, fake, 0.0, 0.1, 0.04, fake, None, None, fake, 1 << 20, None),
               lib.hct_dino_loss_sk(fake, fake, 0, 2, 2, 8, fake, fake, 0.0, 0.1, 0.0, fake, None, None, fake, 1 << 20, None)):
        assert rc == HCT_E_BADARG and b"hct_dino_loss_sk" in lib.hct_last_error_string()
    assert lib.hct_dino_loss_sk(fake, fake, 0, 2, 2, 8, fake, fake, 0.0, 0.1, 0.04, fake, None, None, fake, 8, None) == HCT_E_WORKSPACE
    for rc in (lib.hct_koleo_fwd(fake, 0, 1, 8, 8, fake, fake, fake, fake, None), lib.hct_koleo_fwd(fake, 0, 4, 6, 8, fake, fake, fake, fake, None),
               lib.hct_koleo_fwd(fake, 0, 4, 8, 4, fake, fake, fake, fake, None), lib.hct_koleo_fwd(fake, 0, 4, 8, 10, fake, fake, fake, fake, None),
               lib.hct_koleo_fwd(fake + 4, 0, 4, 8, 8, fake, fake, fake, fake, None), lib.hct_koleo_fwd(fake, 2, 4, 8, 8, fake, fake, fake, fake, None),
               lib.hct_koleo_fwd(fake, 0, 4, 8192, 8192, fake, fake, fake, fake, None)):
        assert rc == HCT_E_BADARG and b"hct_koleo_fwd" in lib.hct_last_error_string()
    for rc in (lib.hct_koleo_bwd(fake, 0, 1, 8, 8, fake, fake, fake, None, fake, 8, None), lib.hct_koleo_bwd(fake, 0, 4, 8, 8, fake, fake, fake, None, fake, 6, None),
               lib.hct_koleo_bwd(fake, 0, 4, 8, 8, fake, fake, fake, None, None, 8, None)):
        assert rc == HCT_E_BADARG and b"hct_koleo_bwd" in lib.hct_last_error_string()
