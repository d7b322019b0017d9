"""GPU: mixup, CutMix and label smoothing for fine-tuning.  hct_mix_volumes and hct_mix_xent through the C ABI against the float64
restatements of tests/mix_ref.py, the autograd function over hct_mix_xent, one step through `MixedCriterion` against a torch
composition, training through engine_downstream.train_one_epoch, and main_downstream.py end to end.

hct_mix_volumes is held to equality wherever the arithmetic is exact: integer inputs with lam in {0, 1/4, 1/2, 1} (mix_ref.exact_volume
says why no operation rounds there) and every CutMix box, which is a bit copy.  With Gaussian inputs and arbitrary lam the bound is
|got - ref| <= 4 * 2^-24 * (|lam a| + |(1 - lam) c|) per element: the roundings are those of 1 - lam, of the product (1 - lam) c and
of the final sum, each at most 2^-24 relative, and one more is allowed for a form that rounds lam a as well.

hct_mix_xent is held to the project's fp32 bar for composite kernels (mix_ref.FP32_BAR = 1e-5): |loss - ref| <= 1e-5 |ref| + 2^-126
(the floor is fp32's smallest normal number, as in tests/test_multilabel_gpu.py) and |got - ref| B / g <= 1e-5 per gradient element,
the error in units of the per-element derivative softmax - t, which lies in [-1, 1].  The comparison with hct_softmax_xent (smoothing 0,
no lam) uses the same bars on the same inputs; that kernel forms (log z + m) - l[t], which at the row of the constant 1e4 rounds by
up to 2^-11 = 4.9e-4 per row, i.e. 4.9e-4 / B in the loss; the bar is at least 1e-5 * 200 / B there because the row of +-100 is scored
on a -100 logit (mix_ref.xent_inputs) and no row's loss is negative.

Measured on an MI355X: hct_mix_volumes with Gaussian inputs within 1.77 of the 4 units of its bound; hct_mix_xent's loss within 2.6e-7
of the float64 reference wherever it is not 0 (n_classes = 1: both are exactly 0), its gradient within 4.4e-7 of the per-element
derivative; against hct_softmax_xent the loss differs by at most 1.9e-6 of the reference (B = 2: the 1e4 row) and the gradient by 8.1e-8.
One step through `MixedCriterion` against the torch composition (float64; the model is fed its fp32 cast): data within 1.7e-7 and
inside the 4-unit bound, loss within 6.2e-7 relative, logit gradient within 2.6e-6 of the per-element derivative.

Every kernel call writes into NaN-filled or content-filled allocations whose guard bands must come back untouched, and is made
twice on fresh copies that must agree bit for bit."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from tests import mix_ref as R
from tests.test_assembly_kernels_gpu import _Out, _p, _st, _twice

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = torch.float32
TINY = 2.0 ** -126
HCT_E_BADARG = -1


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- 1. hct_mix_volumes ---------------------------------------------------------------------------------------------------------------
def _mix(lib, xd, lam, box):
    """One in-place call on a fresh copy of xd that sits between guard bands."""
    B, C, S = xd.shape[:3]
    o = _Out(tuple(xd.shape), F32, xd.device)
    o.t.copy_(xd)
    lamd = lam.to(xd.device)
    boxd = None if box is None else box.to(xd.device)
    rc = lib.hct_mix_volumes(o.ptr, B, C, S, lamd.data_ptr(), _p(boxd), _st())
    assert rc == 0, lib.hct_last_error_string()
    return {"x": o}


@pytest.mark.parametrize("B", R.VOL_B)
@pytest.mark.parametrize("S", R.VOL_S)
def test_mix_volumes_exact(lib, cuda, S, B):
    cases = R.box_cases(S)
    for C in R.VOL_C:
        x = R.exact_volume(B, C, S)
        xd = x.to(cuda)
        for r in range(len(R.EXACT_LAMS)):  # mixup: a different lam on each member of a pair, every lam on every member
            lam = torch.tensor([R.EXACT_LAMS[(b + r) % 4] for b in range(B)], dtype=F32)
            got = _twice(lambda: _mix(lib, xd, lam, None))["x"]
            assert torch.equal(got.double(), R.mix_volumes_ref(x, lam)), (S, B, C, "mixup", lam.tolist())
            if B % 2:
                assert torch.equal(_bits(got[B // 2]), _bits(x[B // 2])), "the middle sample of an odd batch changed"
            none = _twice(lambda: _mix(lib, xd, lam, torch.zeros(B, 6, dtype=torch.int32)))["x"]
            assert torch.equal(_bits(none), _bits(got)), "box == NULL differs from a table of empty boxes"
        for r in range(len(cases)):  # CutMix: every case on every member, a different one on its partner
            names = [cases[(r + 3 * b) % len(cases)][0] for b in range(B)]
            box = torch.tensor([cases[(r + 3 * b) % len(cases)][1] for b in range(B)], dtype=torch.int32)
            lam = torch.tensor([R.EXACT_LAMS[(b + r) % 4] for b in range(B)], dtype=F32)  # used by the members whose box is none
            got = _twice(lambda: _mix(lib, xd, lam, box))["x"]
            ref = R.mix_volumes_ref(x, lam, box)
            for b in range(B):
                assert torch.equal(got[b].double(), ref[b]), (S, B, C, f"sample {b}: {names[b]}; partner: {names[B - 1 - b]}", lam.tolist())
            if B % 2:
                assert torch.equal(_bits(got[B // 2]), _bits(x[B // 2]))


def test_mix_volumes_exact_past_one_trip_of_the_grid(lib, cuda):
    """B = 2, C = 1024, S = 20: 1024 pairs of volumes get ceil(4096 / 1024) = 4 blocks each where a volume has 2000 float4s, 8 blocks'
    worth, so every block takes its grid-stride loop twice -- the path of a fine-tuning batch ([64, 3, 96^3]: 20 trips).  The values
    are 1 + (flat index mod 131071): below 2^17, so the arithmetic of mix_ref.exact_volume stays exact, and different on neighbouring
    voxels, on neighbouring volumes and on the two members of a pair (1024 * 8000 mod 131071 = 65598)."""
    B, C, S = 2, 1024, 20
    x = (1 + torch.arange(B * C * S ** 3, dtype=torch.int64) % 131071).float().view(B, C, S, S, S)
    xd = x.to(cuda)
    cases = dict(R.box_cases(S))
    for lam, box in ((torch.tensor([0.25, 0.5]), None),
                     (torch.tensor([0.25, 0.5]), torch.tensor([cases["a float4 straddling both faces"], cases["high faces"]], dtype=torch.int32)),
                     (torch.tensor([0.25, 1.0]), torch.tensor([cases["no box: mixes with its lam"], cases["one voxel"]], dtype=torch.int32))):
        got = _twice(lambda: _mix(lib, xd, lam, box))["x"]
        assert torch.equal(got.double(), R.mix_volumes_ref(x, lam, box)), (lam.tolist(), None if box is None else box.tolist())


def test_mix_volumes_host_checks(lib, cuda):
    """What `mix_volumes` refuses on the host before it calls the library: the tensor's form, the tables' shapes, and the values of
    tables given on the CPU (tables on the device are taken as they are)."""
    from headct_foundation_amd import mix_volumes
    x = R.exact_volume(2, 1, 8).to(cuda)
    before = x.clone()
    lam = torch.tensor([0.5, 0.5])
    ok_box = torch.tensor([[0, 8, 0, 8, 0, 8], [0, 0, 0, 0, 0, 0]], dtype=torch.int32)
    for bad_x in (x.half(), x[:, :, :, :, :4], x[0], x.transpose(2, 3), x[:, :, ::2]):
        with pytest.raises(ValueError, match="contiguous fp32"):
            mix_volumes(bad_x, lam)
    for bad_lam, bad_box in ((torch.tensor([0.5]), None), (lam, ok_box[:1]), (lam, ok_box[:, :5])):
        with pytest.raises(ValueError, match="entries"):
            mix_volumes(x, bad_lam, bad_box)
    for bad_lam in (torch.tensor([0.5, 1.5]), torch.tensor([-0.1, 0.5]), torch.tensor([0.5, float("nan")])):
        with pytest.raises(ValueError, match=r"lam must lie in \[0, 1\]"):
            mix_volumes(x, bad_lam)
    for bad in ([[0, 9, 0, 8, 0, 8], [0, 0, 0, 0, 0, 0]], [[0, 8, 0, 8, 0, 8], [0, 0, -1, 0, 0, 0]]):
        with pytest.raises(ValueError, match="box bounds"):
            mix_volumes(x, lam, torch.tensor(bad, dtype=torch.int32))
    torch.cuda.synchronize()
    assert torch.equal(x, before)
    out = mix_volumes(x, lam, torch.tensor([[0, 80, 0, 8, -3, 8], [0, 0, 0, 0, 0, 0]], dtype=torch.int32, device=cuda))  # on the device: clamped
    assert out is x and torch.equal(x[0], before[1]) and torch.equal(x[1].double(), 0.5 * before[1].double() + 0.5 * before[0].double())


def test_mix_volumes_rounded(lib, cuda):
    B, C, S = R.ROUNDED_SHAPE
    g = torch.Generator().manual_seed(17)
    x = torch.randn(B, C, S, S, S, generator=g)
    lam = torch.rand(B, generator=g).float()
    got = _twice(lambda: _mix(lib, x.to(cuda), lam, None))["x"]
    ref = R.mix_volumes_ref(x, lam)
    l = lam.double().view(-1, 1, 1, 1, 1)
    bound = 4 * R.U * ((l * x.double()).abs() + ((1 - l) * x.flip(0).double()).abs())
    err = (got.double() - ref).abs()
    print(f"mix_volumes rounded: max err / (2^-24 (|lam a| + |(1 - lam) c|)) = {float((err / (bound / 4)).max()):.3f} (bar 4)")
    assert bool((err <= bound).all())
    box = torch.tensor([[0, S, 0, S, 1, 7], [0, 0, 0, 0, 0, 0], [2, 5, 3, 9, 0, S], [0, 0, 0, 0, 0, 0]], dtype=torch.int32)
    got = _twice(lambda: _mix(lib, x.to(cuda), lam, box))["x"]  # boxed members are bit copies of Gaussian values, the others within the bound
    ref = R.mix_volumes_ref(x, lam, box)
    assert torch.equal(_bits(got[0]), _bits(ref[0].float())) and torch.equal(_bits(got[2]), _bits(ref[2].float()))
    assert bool(((got.double() - ref).abs() <= bound).all())


def test_mix_volumes_refusals_touch_nothing(lib, cuda):
    B, C, S = 2, 1, 8
    x = R.exact_volume(B, C, S)
    o = _Out(tuple(x.shape), F32, cuda)
    o.t.copy_(x.to(cuda))
    lam = torch.tensor([0.5, 0.5], dtype=F32, device=cuda)
    for args in ((o.ptr, B, C, 6, lam.data_ptr()), (o.ptr + 4, B, C, 4, lam.data_ptr()), (o.ptr, 0, C, S, lam.data_ptr()), (o.ptr, B, C, S, None),
                 (None, B, C, S, lam.data_ptr())):
        assert lib.hct_mix_volumes(*args, None, _st()) == HCT_E_BADARG
        assert b"hct_mix_volumes" in lib.hct_last_error_string()
    torch.cuda.synchronize()
    assert torch.equal(_bits(o.result()), _bits(x))


# ---- 2. hct_mix_xent ------------------------------------------------------------------------------------------------------------------
def _xent(lib, xd, yd, lamd, eps, gd, want=("loss", "dlogits")):
    B, Cn = xd.shape
    outs = {}
    if "loss" in want:
        outs["loss"] = _Out((1,), F32, xd.device)
    if "dlogits" in want:
        outs["dlogits"] = _Out((B, Cn), F32, xd.device)
    rc = lib.hct_mix_xent(xd.data_ptr(), yd.data_ptr(), _p(lamd), eps, B, Cn, _p(gd), _p(outs.get("loss")), _p(outs.get("dlogits")), _st())
    assert rc == 0, lib.hct_last_error_string()
    return outs


def _check_xent(res, x, y, lam, eps, g, what):
    """Returns (relative loss error where the reference is a normal number, gradient error in units of the per-element derivative)."""
    B = x.shape[0]
    gv = 1.0 if g is None else g
    loss, grad = R.soft_xent_ref(x, y, lam, float(torch.tensor(eps, dtype=F32)), gv)
    rel = units = 0.0
    if "loss" in res:
        got = float(res["loss"][0])
        err = abs(got - float(loss))
        rel = err / abs(float(loss)) if abs(float(loss)) >= TINY else 0.0
        assert err <= R.FP32_BAR * abs(float(loss)) + TINY, (what, got, float(loss))
    if "dlogits" in res:
        assert not bool(torch.isnan(res["dlogits"]).any()), what
        units = float(((res["dlogits"].double() - grad).abs() * B / gv).max())
        assert units <= R.FP32_BAR, (what, units)
    return rel, units


@pytest.mark.parametrize("Cn", R.XENT_C)
@pytest.mark.parametrize("B", R.XENT_B)
def test_mix_xent_vs_float64(lib, cuda, B, Cn):
    x, y, lam = R.xent_inputs(B, Cn)
    xd, yd = x.to(cuda), y.to(cuda)
    gd = torch.tensor([R.DLOSS], dtype=F32, device=cuda)
    worst = [0.0, 0.0]
    for eps in R.XENT_EPS:
        for name, lv in (("NULL", None), ("ones", torch.ones(B)), ("random", lam)):
            lamd = None if lv is None else lv.to(cuda)
            for use_g in (False, True):
                res = _twice(lambda: _xent(lib, xd, yd, lamd, eps, gd if use_g else None))
                rel, units = _check_xent(res, x, y, lv, eps, R.DLOSS if use_g else None, f"{B}x{Cn} eps={eps} lam={name} dloss={use_g}")
                worst = [max(worst[0], rel), max(worst[1], units)]
    print(f"mix_xent {B}x{Cn}: loss max rel err {worst[0]:.2e}, gradient max err {worst[1]:.2e} in units of the per-element derivative")


@pytest.mark.parametrize("absent", ["loss", "dlogits"])
def test_mix_xent_null_outputs(lib, cuda, absent):
    """Each output NULL in turn: the other is what the full call gives, bit for bit."""
    x, y, lam = R.xent_inputs(257, 14)
    xd, yd, lamd = x.to(cuda), y.to(cuda), lam.to(cuda)
    gd = torch.tensor([R.DLOSS], dtype=F32, device=cuda)
    full = _twice(lambda: _xent(lib, xd, yd, lamd, 0.1, gd))
    (other,) = [k for k in ("loss", "dlogits") if k != absent]
    res = _twice(lambda: _xent(lib, xd, yd, lamd, 0.1, gd, (other,)))
    assert set(res) == {other} and torch.equal(_bits(res[other]), _bits(full[other]))


def test_mix_xent_reduces_to_softmax_xent(lib, cuda):
    """smoothing 0 and lam NULL: hct_softmax_xent's outputs within the bars (module docstring), on every shape of the grid."""
    worst = [0.0, 0.0]
    for B in R.XENT_B:
        for Cn in R.XENT_C:
            x, y, _ = R.xent_inputs(B, Cn)
            xd, yd = x.to(cuda), y.to(cuda)
            gd = torch.tensor([R.DLOSS], dtype=F32, device=cuda)
            mine = _twice(lambda: _xent(lib, xd, yd, None, 0.0, gd))

            def theirs():
                outs = {"loss": _Out((1,), F32, cuda), "dlogits": _Out((B, Cn), F32, cuda)}
                assert lib.hct_softmax_xent(xd.data_ptr(), yd.data_ptr(), B, Cn, gd.data_ptr(), outs["loss"].ptr, outs["dlogits"].ptr, _st()) == 0
                return outs
            old = _twice(theirs)
            ref = float(R.soft_xent_ref(x, y)[0])
            err = abs(float(mine["loss"][0]) - float(old["loss"][0]))
            units = float(((mine["dlogits"].double() - old["dlogits"].double()).abs() * B / R.DLOSS).max())
            worst = [max(worst[0], err / abs(ref) if abs(ref) >= TINY else 0.0), max(worst[1], units)]
            assert err <= R.FP32_BAR * abs(ref) + TINY, (B, Cn, float(mine["loss"][0]), float(old["loss"][0]), ref)
            assert units <= R.FP32_BAR, (B, Cn, units)
    print(f"mix_xent against softmax_xent: loss max difference {worst[0]:.2e} of the reference, gradient max difference {worst[1]:.2e}")


def test_mix_xent_refusals_touch_nothing(lib, cuda):
    x, y, lam = R.xent_inputs(3, 14)
    xd, yd, lamd = x.to(cuda), y.to(cuda), lam.to(cuda)
    outs = dict(loss=_Out((1,), F32, cuda), dlogits=_Out((3, 14), F32, cuda))
    lp, dp = outs["loss"].ptr, outs["dlogits"].ptr
    for eps, B, a, b in ((1.0, 3, lp, dp), (0.1, 0, lp, dp), (0.1, 3, None, None)):
        assert lib.hct_mix_xent(xd.data_ptr(), yd.data_ptr(), lamd.data_ptr(), eps, B, 14, None, a, b, _st()) == HCT_E_BADARG
        assert b"hct_mix_xent" in lib.hct_last_error_string()
    torch.cuda.synchronize()
    for o in outs.values():
        o.result()
        assert o.untouched()


# ---- 3. the autograd function ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_lam", [True, False])
def test_soft_cross_entropy_autograd(lib, cuda, use_lam):
    from headct_foundation_amd import soft_cross_entropy
    x, y, lam = R.xent_inputs(257, 14)
    xd, yd, lamd = x.to(cuda), y.to(cuda), (lam.to(cuda) if use_lam else None)
    kernel = _twice(lambda: _xent(lib, xd, yd, lamd, 0.1, None))
    leaf = xd.clone().requires_grad_(True)
    loss = soft_cross_entropy(leaf, yd, lamd, 0.1)
    loss.backward()
    assert loss.shape == () and torch.equal(_bits(loss.detach().cpu().view(1)), _bits(kernel["loss"]))
    assert torch.equal(_bits(leaf.grad.cpu()), _bits(kernel["dlogits"]))
    _check_xent({"loss": loss.detach().cpu().view(1), "dlogits": leaf.grad.cpu()}, x, y, lam if use_lam else None, 0.1, None, f"autograd lam={use_lam}")
    one = leaf.grad.clone()
    leaf.grad = None
    (3 * soft_cross_entropy(leaf, yd, lamd, 0.1)).backward()  # a scaled loss scales the gradient: within one ulp of 3 x
    ulp = torch.abs(torch.nextafter(3 * one, torch.full_like(one, float("inf"))) - 3 * one)
    assert bool(((leaf.grad - 3 * one).abs() <= ulp).all())
    with pytest.raises(ValueError, match="smoothing"):
        soft_cross_entropy(leaf, yd, lamd, 1.0)


# ---- 4. one step through MixedCriterion against a torch composition ---------------------------------------------------------------------
def _tiny(cuda, dtype, n_out, lock=False):
    from headct_foundation_amd import LinearClassifier
    from headct_foundation_amd.dino_model import ViTBackbone
    torch.manual_seed(5)
    vit = ViTBackbone(in_chans=3, img_size=24, patch_size=12, hidden_size=48, mlp_dim=96, num_layers=2, num_heads=3, num_register_tokens=0,
                      compute_dtype=dtype).to(cuda)
    cls = LinearClassifier(48, n_out, feature_grad=not lock).to(cuda).train()
    return vit, cls


@pytest.mark.parametrize("mode", ["batch", "elem"])
def test_mixed_step_against_torch_composition(lib, cuda, mode):
    from headct_foundation_amd import MixedCriterion, Mixup
    from headct_foundation_amd.data import SyntheticLabelled
    vit, cls = _tiny(cuda, "fp32", 3)
    vit.train()
    x, y, _ = next(iter(SyntheticLabelled(1, 4, 3, 24, 3, cuda, seed=3)))
    eps = 0.1
    for seed in (0, 1, 2, 3):  # four draws
        crit = MixedCriterion(Mixup(0.8, 1.0, mode=mode, seed=seed), eps)
        data, state = crit.mix(x.clone(), y)
        lam_x, box, lam_y = crit.mixup.last_draw
        assert torch.equal(state.cpu(), lam_y)
        # the composition: timm's, sample by sample against the flipped batch, in float64; the model is fed its fp32 cast
        x64 = x.double()
        flipped, want64 = x64.flip(0), x64.clone()
        bound = torch.zeros_like(x64)  # 0 where a box decides: a bit copy
        for b in range(4):
            if box is not None and R.has_box(box[b].tolist(), 24):
                l0, h0, l1, h1, l2, h2 = box[b].tolist()
                want64[b, :, l0:h0, l1:h1, l2:h2] = flipped[b, :, l0:h0, l1:h1, l2:h2]
            else:
                l = float(lam_x[b])
                want64[b] = x64[b] * l + flipped[b] * (1 - l)
                bound[b] = 4 * R.U * ((x64[b] * l).abs() + (flipped[b] * (1 - l)).abs())
        derr = (data.double() - want64).abs()
        assert bool((derr <= bound).all())  # the bar of test_mix_volumes_rounded
        want = want64.float()
        outs = []
        for batch in (data, want):
            for m in (vit, cls):
                m.zero_grad()
            logits = cls(vit(batch)[0])
            logits.retain_grad()
            if batch is data:
                loss = crit.train_loss(logits, y, state)
                loss.backward()
                outs.append((float(loss.detach()), logits.grad.double().cpu()))
            else:
                l = lam_y.double().view(-1, 1).to(cuda)
                onehot = lambda t: F.one_hot(t, 3).double()
                leaf = logits.detach().double().requires_grad_(True)
                loss = F.cross_entropy(leaf, l * onehot(y) + (1 - l) * onehot(y.flip(0)), label_smoothing=eps)
                loss.backward()
                outs.append((float(loss.detach()), leaf.grad.cpu()))
        (la, ga), (lb, gb) = outs
        units = float((ga - gb).abs().max()) * 4
        print(f"mixed step mode={mode} seed={seed}: boxes {None if box is None else box.tolist()}, data max err {float(derr.max()):.2e}, "
              f"loss {la:.7f} against {lb:.7f}, logit gradient max err {units:.2e} in units of the per-element derivative")
        assert abs(la - lb) <= R.FP32_BAR * abs(lb)
        assert units <= R.FP32_BAR


# ---- 5. training and inertness --------------------------------------------------------------------------------------------------------
EPOCHS = 30  # the steps of tests/test_multilabel_gpu.py's _train


def _train(cuda, mode, lock, multilabel=False):
    import config as cfgmod
    from engine_downstream import train_one_epoch
    from headct_foundation_amd import MixedCriterion, Mixup
    from headct_foundation_amd.data import SyntheticLabelled, SyntheticMultiLabelled
    from headct_foundation_amd.metrics import ClassificationMetrics, MultilabelMetrics
    from headct_foundation_amd.optim import HipAdamW
    names = ["a", "b", "c"] if multilabel else []
    cfg = cfgmod._C.clone()
    cfg.MODEL.NAME, cfg.TRAIN.LOCK, cfg.TRAIN.GRAD_CLIP, cfg.TRAIN.LABEL_NAMES, cfg.DATA.NUM_CLASSES = "vit", lock, 1.0, names, 2 if multilabel else 3
    vit, cls = _tiny(cuda, "bf16", 3, lock)
    if lock:
        for p in vit.parameters():
            p.requires_grad_(False)
    opts = [HipAdamW(cls, lr=1e-3, weight_decay=0.04)] + ([] if lock else [HipAdamW(vit, lr=1e-5, weight_decay=0.04)])
    train = (SyntheticMultiLabelled if multilabel else SyntheticLabelled)(2, 4, 3, 24, 3, cuda, seed=0)
    kept = [b[0].clone() for b in train]
    crit = MixedCriterion(Mixup(0.8, 0.0 if multilabel else 1.0, mode=mode, seed=0), 0.0 if multilabel else 0.1, multilabel=multilabel)
    before, head_before = vit._flat.clone(), cls._flat.clone()
    metrics = MultilabelMetrics(names) if multilabel else ClassificationMetrics(3)
    losses = [train_one_epoch(cfg, vit, cls, train, opts, [], crit, e, EPOCHS, metrics, device=cuda)["loss"] for e in range(EPOCHS)]
    assert all(torch.equal(a, b[0]) for a, b in zip(kept, train)), "the loader's own batches were mixed in place"
    third = EPOCHS // 3
    first, last = sum(losses[:third]) / third, sum(losses[-third:]) / third
    print(f"mixed training mode={mode} lock={lock} multilabel={multilabel}: loss {losses[0]:.4f} -> {losses[-1]:.4f}, mean of the first {third} epochs "
          f"{first:.4f}, of the last {third} {last:.4f}")
    assert all(l == l and abs(l) != float("inf") for l in losses), losses
    assert not torch.equal(head_before, cls._flat)
    return first, last, before, vit, cls, cfg, crit


@pytest.mark.parametrize("mode", ["batch", "elem"])
def test_mixed_training_loss_falls(lib, cuda, mode):
    """The loss of a mixed batch depends on its draw (a batch at lam 1/2 cannot go below log 2), so "falls" is read on the means of the
    first and the last third of the epochs, not on two single values."""
    first, last, before, vit, _, _, _ = _train(cuda, mode, False)
    assert last < first, (first, last)
    assert not torch.equal(before, vit._flat)


def test_mixed_training_lock_keeps_backbone_bit_unchanged(lib, cuda):
    first, last, before, vit, _, _, _ = _train(cuda, "batch", True)
    assert torch.equal(before, vit._flat)
    assert last < first, (first, last)


def test_mixed_training_multilabel_is_finite(lib, cuda):
    _train(cuda, "elem", False, multilabel=True)


def test_validation_sees_the_plain_loss_and_defaults_are_inert(lib, cuda):
    import config as cfgmod
    import main_downstream
    from engine_downstream import val_one_epoch
    from headct_foundation_amd import MixedCriterion, Mixup, cross_entropy
    from headct_foundation_amd.data import SyntheticLabelled
    from headct_foundation_amd.metrics import ClassificationMetrics
    cfg = cfgmod._C.clone()
    cfg.MODEL.NAME, cfg.DATA.NUM_CLASSES = "vit", 3
    vit, cls = _tiny(cuda, "bf16", 3)
    val = SyntheticLabelled(3, 4, 3, 24, 3, cuda, seed=1000)
    kept = [b[0].clone() for b in val]
    crit = MixedCriterion(Mixup(0.8, 1.0, seed=0), 0.1)
    mixed = val_one_epoch(cfg, vit, cls, val, 0, 1, ClassificationMetrics(3), crit, device=cuda)["loss"]
    plain = val_one_epoch(cfg, vit, cls, val, 0, 1, ClassificationMetrics(3), cross_entropy, device=cuda)["loss"]
    assert mixed == plain and crit.mixup.last_draw is None  # bit for bit, and nothing was drawn
    assert all(torch.equal(a, b[0]) for a, b in zip(kept, val))
    assert main_downstream.build_criterion(cfg) is cross_entropy  # every knob 0: exactly what the engine got before


# ---- 6. main_downstream.py end to end ---------------------------------------------------------------------------------------------------
def test_main_downstream_mixed_run(lib, cuda, tmp_path):
    from headct_foundation_amd.classifier import LinearClassifier
    from headct_foundation_amd.dino_model import ViTBackbone
    vit = ViTBackbone(in_chans=3, img_size=24, patch_size=12, hidden_size=48, mlp_dim=96, num_layers=2, num_heads=3, compute_dtype="fp32")
    torch.save({"state_dict": {"module." + k: v for k, v in vit.state_dict().items()}, "epoch": 3}, tmp_path / "pre.pt")
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("MODEL:\n  NAME: vit\n")
    opts = ["DATA.SYNTHETIC", "True", "DATA.SYNTHETIC_SAMPLES", "8", "VIT.INPUT_SIZE", "24", "VIT.PATCH_SIZE", "12",
            "VIT.HIDDEN_SIZE", "48", "VIT.MLP_DIM", "96", "VIT.NUM_LAYERS", "2", "VIT.NUM_HEADS", "3", "TRAIN.VAL_EVERY", "1",
            "MODEL.DIR", str(tmp_path / "out"), "MODEL.SAVE_NAME", "ft.pt", "LOG.OUTPUT_DIR", str(tmp_path / "log"),
            "PREDS_SAVE_NAME", "run"]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nproc-per-node", "1", "--master-port", "29641",
           os.path.join(ROOT, "main_downstream.py"), "--cfg", str(cfg), "--model_name", "vit", "--model_load_path", str(tmp_path / "pre.pt"),
           "--classifier", "linear", "--batch_size", "4", "--max_epochs", "2", "--grad_clip", "1.0", "--base_lr", "1e-4",
           "--mixup", "0.8", "--cutmix", "1.0", "--smoothing", "0.1", "--opts"] + opts
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-4000:]
    assert "Fine-tuning recipe: TRAIN.MIXUP 0.8, TRAIN.CUTMIX 1.0" in log and "TRAIN.LABEL_SMOOTHING 0.1" in log and "Final test loss" in log, log[-4000:]
    c = torch.load(tmp_path / "out" / "ft_classifier.pt", weights_only=True)
    LinearClassifier(48, 2).load_state_dict(c["state_dict"], strict=True)
    assert "state_dict" in torch.load(tmp_path / "out" / "ft.pt", weights_only=True)
