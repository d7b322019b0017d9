"""CPU: mixup, CutMix and label smoothing -- the yardstick tests/mix_ref.py held to torch's own soft-target cross-entropy, the host-side
draws of `Mixup` (determinism, ranges, modes, boxes against rand_box3d_ref from the same generator state), the multi-label target
table, the config keys and flags, and that the two symbols are declared, bound and exported and refuse to run off the GPU."""
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from headct_foundation_amd import _lib
from headct_foundation_amd import HctError, MixedCriterion, Mixup, cross_entropy, mix_multilabel_targets, mix_volumes, rand_box3d, soft_cross_entropy
from tests import mix_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the yardstick against torch ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", R.XENT_EPS)
@pytest.mark.parametrize("B,Cn", [(1, 3), (2, 2), (3, 14), (5, 1), (64, 14), (257, 3)])
def test_soft_xent_ref_is_torch_soft_target_cross_entropy(B, Cn, eps):
    x, y, lam = R.xent_inputs(B, Cn)
    for use_lam in (True, False):
        l = lam.double().view(-1, 1) if use_lam else torch.ones(B, 1, dtype=torch.float64)
        onehot = lambda t: F.one_hot(t, Cn).double()
        leaf = x.double().clone().requires_grad_(True)
        want = F.cross_entropy(leaf, l * onehot(y) + (1 - l) * onehot(y.flip(0)), label_smoothing=eps)
        (grad,) = torch.autograd.grad(want, leaf)
        want = want.detach()
        loss, dl = R.soft_xent_ref(x, y, lam if use_lam else None, eps, R.DLOSS)
        assert abs(float(loss) - float(want)) <= 1e-12, (float(loss), float(want))
        assert float((dl - R.DLOSS * grad).abs().max()) <= 1e-12
    plain = F.cross_entropy(x.double(), y)
    assert abs(float(R.soft_xent_ref(x, y, None, 0.0)[0]) - float(plain)) <= 1e-12


def test_mix_volumes_ref_pairs_and_boxes():
    x = R.exact_volume(3, 1, 4)
    lam = torch.tensor([0.25, 0.5, 1.0])
    out = R.mix_volumes_ref(x, lam)
    assert torch.equal(out[0], 0.25 * x[0].double() + 0.75 * x[2].double()) and torch.equal(out[1], x[1].double()) and torch.equal(out[2], x[2].double())
    box = torch.tensor([[0, 1, 0, 4, -3, 9], [0, 4, 0, 4, 0, 4], [2, 2, 0, 4, 0, 4]], dtype=torch.int32)
    out = R.mix_volumes_ref(x, lam, box)
    assert torch.equal(out[0, :, :1], x[2, :, :1].double()) and torch.equal(out[0, :, 1:], x[0, :, 1:].double())
    assert torch.equal(out[1], x[1].double()) and torch.equal(out[2], x[2].double())  # the middle sample; an empty box with lam 1


# ---- Mixup.draw --------------------------------------------------------------------------------------------------------------------------
def test_draw_is_deterministic_per_seed_and_in_range():
    for mode in ("batch", "elem"):
        a, b, c = (Mixup(0.8, 1.0, mode=mode, seed=s) for s in (5, 5, 6))
        seq_a, seq_b, seq_c = ([m.draw(6, 24) for _ in range(20)] for m in (a, b, c))
        same = lambda p, q: all((u is None and v is None) or torch.equal(u, v) for u, v in zip(p, q))
        assert all(same(p, q) for p, q in zip(seq_a, seq_b))
        assert not all(same(p, q) for p, q in zip(seq_a, seq_c))
        for lam_x, box, lam_y in seq_a:
            assert lam_x.dtype == lam_y.dtype == torch.float32 and lam_x.shape == lam_y.shape == (6,)
            assert bool(((lam_x >= 0) & (lam_x <= 1) & (lam_y >= 0) & (lam_y <= 1)).all())
            assert box is None or (box.dtype == torch.int32 and box.shape == (6, 6) and int(box.min()) >= 0 and int(box.max()) <= 24)
        assert a.last_draw is seq_a[-1]


def test_draw_modes_prob_and_methods():
    batch = [Mixup(0.8, 0.0, mode="batch", seed=1).draw(8, 24) for _ in range(1)][0]
    assert len(set(batch[2].tolist())) == 1 and batch[1] is None and torch.equal(batch[0], batch[2])
    elem = Mixup(0.8, 0.0, mode="elem", seed=1).draw(8, 24)
    assert len(set(elem[2].tolist())) > 1 and elem[1] is None  # mixup alone never gives a box
    off = Mixup(0.8, 1.0, prob=0.0, mode="elem", seed=1)
    for _ in range(5):
        lam_x, box, lam_y = off.draw(8, 24)
        assert box is None and bool((lam_x == 1).all()) and bool((lam_y == 1).all())
    none = Mixup(0.0, 0.0).draw(4, 24)
    assert none[1] is None and bool((none[2] == 1).all())
    cut = Mixup(0.0, 1.0, mode="elem", seed=2)
    for _ in range(5):
        lam_x, box, lam_y = cut.draw(8, 24)
        assert box is not None and bool((lam_x == 1).all())  # CutMix alone always gives boxes; voxel lam 1: an empty box mixes nothing
    both = Mixup(0.8, 1.0, switch_prob=0.5, mode="elem", seed=3)
    kinds = [bool(b.any()) for _ in range(10) for b in both.draw(8, 24)[1]]
    assert any(kinds) and not all(kinds)
    assert all(bool(Mixup(0.8, 1.0, switch_prob=1.0, mode="elem", seed=4).draw(4, 24)[0].eq(1).all()) for _ in range(3))
    for bad in (dict(mixup_alpha=-1.0), dict(cutmix_alpha=-0.1), dict(prob=1.5), dict(switch_prob=-0.1), dict(mode="pair")):
        with pytest.raises(ValueError):
            Mixup(**{"mixup_alpha": 0.8, **bad})


@pytest.mark.parametrize("mode", ["batch", "elem"])
def test_boxes_equal_rand_box3d_ref_of_the_same_generator_state(mode):
    S, B, alpha, seed = 24, 5, 1.0, 11
    m = Mixup(0.0, alpha, mode=mode, seed=seed)
    rng = np.random.default_rng(seed)
    for _ in range(4):
        lam_x, box, lam_y = m.draw(B, S)
        want = []
        for _ in range(1 if mode == "batch" else B):
            assert rng.random() < 1.0             # the draw against prob
            lam = rng.beta(alpha, alpha)
            want.append(R.rand_box3d_ref(S, lam, rng))
        want = want * B if mode == "batch" else want
        assert box.tolist() == [list(w[0]) for w in want]
        for b in range(B):
            l0, h0, l1, h1, l2, h2 = box[b].tolist()
            assert float(lam_y[b]) == float(np.float32(1.0 - (h0 - l0) * (h1 - l1) * (h2 - l2) / S ** 3)) == float(np.float32(want[b][1]))
    rng_a, rng_b = np.random.default_rng(3), np.random.default_rng(3)
    for lam in (0.0, 0.3, 0.999, 1.0):
        assert rand_box3d(20, lam, rng_a) == R.rand_box3d_ref(20, lam, rng_b)
    box, lam = rand_box3d(20, 1.0, rng_a)  # cut length 0: an empty box, lam back to 1
    assert lam == 1.0 and not R.has_box(box, 20)


# ---- multi-label targets ---------------------------------------------------------------------------------------------------------------
def test_mix_multilabel_targets():
    nan = float("nan")
    y = torch.tensor([[1.0, 0.0, -1.0, 1.0], [0.0, 1.0, 1.0, nan], [1.0, 1.0, 0.0, 0.0]])
    lam = torch.tensor([0.25, 0.5, 1.0])
    out = mix_multilabel_targets(y, lam)
    want = torch.tensor([[1.0, 0.75, -1.0, 0.25],   # row 0 with row 2; entry 2 missing on this side
                         [0.0, 1.0, 1.0, -1.0],     # the middle row with itself; NaN is a missing entry
                         [1.0, 1.0, -1.0, 0.0]])    # row 2 with row 0 at lam 1; entry 2 missing on the other side
    assert torch.equal(out, want)
    assert torch.equal(mix_multilabel_targets(y[:, :2], torch.ones(3)), y[:, :2])


# ---- configuration and arguments -----------------------------------------------------------------------------------------------------
def _parse(monkeypatch, tmp_path, *extra, yaml="MODEL:\n  NAME: vit\n"):
    import main_downstream
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(yaml)
    monkeypatch.setattr(sys, "argv", ["main_downstream.py", "--cfg", str(cfg), "--model_name", "vit", *extra])
    return main_downstream.parse_option()[1]


def test_config_keys_flags_and_refusals(monkeypatch, tmp_path):
    import config as cfgmod
    import main_downstream
    t = cfgmod._C.TRAIN
    assert (t.MIXUP, t.CUTMIX, t.MIX_PROB, t.MIX_SWITCH_PROB, t.MIX_MODE, t.LABEL_SMOOTHING) == (0.0, 0.0, 1.0, 0.5, "batch", 0.0)
    c = _parse(monkeypatch, tmp_path)
    assert (c.TRAIN.MIXUP, c.TRAIN.CUTMIX, c.TRAIN.LABEL_SMOOTHING) == (0.0, 0.0, 0.0)
    assert main_downstream.build_criterion(c) is cross_entropy  # every knob at its default: exactly what the engine got before
    over = "MODEL:\n  NAME: vit\nTRAIN:\n  MIXUP: 0.3\n  CUTMIX: 0.4\n  LABEL_SMOOTHING: 0.2\n"
    c = _parse(monkeypatch, tmp_path, yaml=over)
    assert (c.TRAIN.MIXUP, c.TRAIN.CUTMIX, c.TRAIN.LABEL_SMOOTHING) == (0.3, 0.4, 0.2)
    c = _parse(monkeypatch, tmp_path, "--mixup", "0", "--cutmix", "0", "--smoothing", "0", yaml=over)  # 0 reaches the config
    assert (c.TRAIN.MIXUP, c.TRAIN.CUTMIX, c.TRAIN.LABEL_SMOOTHING) == (0.0, 0.0, 0.0)
    c = _parse(monkeypatch, tmp_path, "--mixup", "0.8", "--cutmix", "1.0", "--smoothing", "0.1", "--opts", "TRAIN.MIX_MODE", "elem",
               "TRAIN.MIX_PROB", "0.5", "SEED", "7")
    assert (c.TRAIN.MIXUP, c.TRAIN.CUTMIX, c.TRAIN.LABEL_SMOOTHING, c.TRAIN.MIX_MODE, c.TRAIN.MIX_PROB) == (0.8, 1.0, 0.1, "elem", 0.5)
    crit = main_downstream.build_criterion(c, seed=c.SEED + 1)
    assert isinstance(crit, MixedCriterion) and crit.smoothing == 0.1 and not crit.multilabel
    assert (crit.mixup.mixup_alpha, crit.mixup.cutmix_alpha, crit.mixup.prob, crit.mixup.mode) == (0.8, 1.0, 0.5, "elem")
    twin = Mixup(0.8, 1.0, prob=0.5, mode="elem", seed=8)
    assert all(torch.equal(a, b) for a, b in zip(crit.mixup.draw(4, 24)[::2], twin.draw(4, 24)[::2]))
    only = main_downstream.build_criterion(_parse(monkeypatch, tmp_path, "--smoothing", "0.1"))
    assert isinstance(only, MixedCriterion) and only.mixup is None
    for bad in (("--mixup", "-0.1"), ("--cutmix", "-1"), ("--smoothing", "1"), ("--smoothing", "-0.1"), ("--opts", "TRAIN.MIX_PROB", "1.5"),
                ("--opts", "TRAIN.MIX_SWITCH_PROB", "-0.5"), ("--opts", "TRAIN.MIX_MODE", "pair")):
        with pytest.raises(ValueError, match="TRAIN"):
            _parse(monkeypatch, tmp_path, *bad)
    multi = _parse(monkeypatch, tmp_path, "--mixup", "0.8", "--label_names", "a", "b", "--opts", "DATA.SYNTHETIC", "True")
    assert main_downstream.build_criterion(multi).multilabel
    with pytest.raises(ValueError, match="softmax mode only"):
        main_downstream.build_criterion(_parse(monkeypatch, tmp_path, "--smoothing", "0.1", "--label_names", "a", "b"))
    with pytest.raises(ValueError, match="softmax mode only"):
        MixedCriterion(None, 0.1, multilabel=True)


# ---- symbols and refusals off the GPU ----------------------------------------------------------------------------------------------------
def test_symbols_are_declared_bound_and_exported(lib):
    import headct_foundation_amd as pkg
    with open(os.path.join(ROOT, "include", "headct_hip.h")) as f:
        hdr = f.read()
    for s in ("hct_mix_volumes", "hct_mix_xent"):
        assert re.search(r"\b" + s + r"\s*\(", hdr) and s in _lib.exported_symbols() and hasattr(lib, s), s
    for s in ("Mixup", "MixedCriterion", "mix_volumes", "mix_multilabel_targets", "rand_box3d", "soft_cross_entropy"):
        assert hasattr(pkg, s), s
    from headct_foundation_amd import build
    assert "mixup.hip" in build.SOURCES


def test_no_cpu_fallback(lib):
    x = torch.zeros(2, 1, 4, 4, 4)
    with pytest.raises(HctError, match="no CPU fallback"):
        mix_volumes(x, torch.tensor([0.5, 0.5]))
    with pytest.raises(HctError, match="no CPU fallback"):
        Mixup(0.8, 0.0)(x)
    with pytest.raises(HctError, match="no CPU fallback"):
        soft_cross_entropy(torch.zeros(2, 3), torch.tensor([0, 1]))
    assert bool((x == 0).all())


def test_host_visible_arguments_are_refused_before_any_launch(lib):
    HCT_E_BADARG = -1  # include/headct_hip.h
    fake = 4096  # never dereferenced: every call below returns before a launch
    for rc in (lib.hct_mix_volumes(None, 2, 1, 8, fake, None, None), lib.hct_mix_volumes(fake, 2, 1, 8, None, None, None),
               lib.hct_mix_volumes(fake, 0, 1, 8, fake, None, None), lib.hct_mix_volumes(fake, 2, 1, 6, fake, None, None),
               lib.hct_mix_volumes(fake, 2, 1, 1028, fake, None, None), lib.hct_mix_volumes(fake, 65536, 1, 8, fake, None, None),
               lib.hct_mix_volumes(fake + 4, 2, 1, 8, fake, None, None)):
        assert rc == HCT_E_BADARG and b"hct_mix_volumes" in lib.hct_last_error_string()
    for rc in (lib.hct_mix_xent(fake, fake, None, 1.0, 4, 3, None, fake, fake, None), lib.hct_mix_xent(fake, fake, None, -0.1, 4, 3, None, fake, fake, None),
               lib.hct_mix_xent(fake, fake, None, float("nan"), 4, 3, None, fake, fake, None), lib.hct_mix_xent(fake, fake, None, 0.1, 0, 3, None, fake, fake, None),
               lib.hct_mix_xent(fake, fake, None, 0.1, 4, 0, None, fake, fake, None), lib.hct_mix_xent(fake, fake, None, 0.1, 4, 3, None, None, None, None),
               lib.hct_mix_xent(None, fake, None, 0.1, 4, 3, None, fake, fake, None), lib.hct_mix_xent(fake, None, None, 0.1, 4, 3, None, fake, fake, None)):
        assert rc == HCT_E_BADARG and b"hct_mix_xent" in lib.hct_last_error_string()
