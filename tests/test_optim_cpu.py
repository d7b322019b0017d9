"""CPU: the Lion / SGD / Lamb optimizers and the poly / constant schedules.  The torch restatement (tests/optim_ref.py) against the
fixture made from the reference's own classes (tests/golden/optimizers.json); the host classes' dispatch, state-dict layout and
interchange with the torch-side optimizers; the loud failure without a GPU; the new C-ABI symbols."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

from oracle import mae_oracle as O
from tests import optim_ref as R
from tests.util import load_golden, sample_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("hct_lion_step", "hct_sgd_step", "hct_lamb_workspace_bytes", "hct_lamb_step")


def _config(optimizer="AdamW", scheduler="cosine"):
    train = types.SimpleNamespace(OPTIMIZER=optimizer, SCHEDULER=scheduler, WEIGHT_DECAY=5e-3, BETA1=0.9, BETA2=0.95, MOMENTUM=0.9)
    return types.SimpleNamespace(TRAIN=train)


def _micro():
    from headct_foundation_amd import MaskedAutoencoderViT
    cfg = O.CONFIGS["micro"]
    m = MaskedAutoencoderViT(**cfg.ctor_kwargs())
    m.load_state_dict(O.make_params(cfg, 0), strict=True)
    return cfg, m


@pytest.mark.parametrize("kind", R.KINDS)
def test_restatement_reproduces_reference_fixture(kind):
    """Pins tests/optim_ref.py to the reference where the reference itself is absent: parameters and state of every tensor case after
    each of the 5 steps.  The generator saw 0 (fp32, bit-equal) and <= 1.3e-7 (fp64 restatement against the fp32 reference); the fixture
    stores 9 significant digits, so samples are held to 1e-6 relative to the tensor's largest sample."""
    fx = load_golden("optimizers")["tensors"][kind]
    assert fx["hp"] == R.HP and fx["restatement_rel_dev"] <= 1e-6
    hist = R.run_cases(kind, torch.float32)
    assert len(hist) == len(fx["steps"]) == R.NSTEPS
    for (params, states), want in zip(hist, fx["steps"]):
        assert set(params) == set(want["params"])
        for n, entry in want["params"].items():
            got, ref, l2, l2w = sample_of(params[n], entry)
            assert abs(l2 - l2w) <= 1e-6 * l2w + 1e-30 and float((got - ref).abs().max()) <= 1e-6 * float(ref.abs().max()) + 1e-30, (kind, n)
        for n, st in want["state"].items():
            for k, entry in st.items():
                got, ref, l2, l2w = sample_of(states[n][k], entry)
                assert abs(l2 - l2w) <= 1e-6 * l2w + 1e-30 and float((got - ref).abs().max()) <= 1e-6 * float(ref.abs().max()) + 1e-30, (kind, n, k)
    # the special cases are really in there
    p0 = R.case_params()
    assert float(p0["big_norm"].norm()) > 10 and float(p0["param_zero"].abs().max()) == 0 and R.case_grads(2)["grad_none"] is None
    last = hist[-1][0]
    assert torch.equal(last["grad_none"], p0["grad_none"])
    if kind == "Lion":  # sign(0) = 0: only the weight decay moves a parameter whose gradient is zero
        keep = 1 - R.HP["lr"] * R.HP["weight_decay"]
        assert torch.allclose(last["grad_zero"], p0["grad_zero"] * keep ** R.NSTEPS, rtol=1e-6, atol=0)
    if kind == "SGD":
        assert torch.equal(last["grad_zero"], p0["grad_zero"])


def test_lamb_special_cases_of_the_restatement():
    """weight_norm clamps at 10, a zero parameter and a zero update both give trust ratio 1, a zero gradient leaves adam_norm =
    wd * ||p|| (the moments stay 0)."""
    hp = R.HP
    p = R.case_params()
    g = R.case_grads(0)
    st = {n: R.new_state("Lamb", p[n]) for n in p}
    out = {n: R.apply_("Lamb", p[n].clone(), g[n], st[n], hp["lr"], hp) for n in p if g[n] is not None}
    assert float(out["big_norm"][0]) == 10.0
    assert float(out["param_zero"][0]) == 0.0 and float(out["param_zero"][2]) == 1.0
    w, a, r = out["grad_zero"]
    assert abs(float(a) - hp["weight_decay"] * float(p["grad_zero"].norm())) <= 1e-6 * float(a)
    z = torch.zeros(8)
    assert float(R.lamb_step_(z.clone(), z.clone(), z.clone(), z.clone(), 1e-3, 0.9, 0.95, 1e-6, 0.0)[2]) == 1.0


@pytest.mark.parametrize("kind", ["poly", "constant"])
def test_schedules_match_reference_values(kind):
    from headct_foundation_amd.lr_sched import get_lr_scheduler
    fx = load_golden("optimizers")["schedules"]
    c = fx["case"]
    assert c == R.SCHEDULE_CASE
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=c["lr0"])
    sched = get_lr_scheduler(_config(scheduler=kind), opt, c["warmup"], c["total"], c["lr_end"])
    assert sched.state_dict()["lr_lambdas"] == [None]  # a closure, as in a reference checkpoint
    vals = []
    for _ in range(c["steps"]):
        vals.append(opt.param_groups[0]["lr"])
        opt.step()
        sched.step()
    assert np.allclose(vals, fx["lrs"][kind], rtol=1e-12, atol=0)
    assert np.allclose([c["lr0"] * R.factor(kind, s, c["warmup"], c["total"], c["lr0"], c["lr_end"]) for s in range(c["steps"])],
                       fx["lrs"][kind], rtol=1e-12, atol=0)
    if kind == "poly":
        assert vals[-1] == pytest.approx(c["lr_end"], rel=1e-12) and vals[c["total"]] == pytest.approx(c["lr_end"], rel=1e-12)
    else:
        assert vals[c["warmup"]:] == [c["lr0"]] * (c["steps"] - c["warmup"])


def test_scheduler_dispatch_and_errors():
    from headct_foundation_amd.lr_sched import get_constant_schedule_with_warmup, get_lr_scheduler, get_polynomial_decay_schedule_with_warmup
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=1e-3)
    for kind in ("cosine", "poly", "constant"):
        assert isinstance(get_lr_scheduler(_config(scheduler=kind), opt, 2, 10, 1e-6), torch.optim.lr_scheduler.LambdaLR)
    with pytest.raises(ValueError, match="Scheduler linear not supported"):
        get_lr_scheduler(_config(scheduler="linear"), opt, 2, 10, 1e-6)
    for bad in (1e-3, 1.0):  # lr_end >= lr0
        with pytest.raises(ValueError):
            get_polynomial_decay_schedule_with_warmup(opt, 2, 10, lr_end=bad, power=2.0)
        with pytest.raises(ValueError):
            get_lr_scheduler(_config(scheduler="poly"), opt, 2, 10, bad)
    get_constant_schedule_with_warmup(opt, 2)  # the function's own signature: no num_training_steps


def test_get_optimizer_dispatch(lib):
    from headct_foundation_amd import HipAdamW, HipLamb, HipLion, HipSGD
    from headct_foundation_amd.optim import get_optimizer
    _, m = _micro()
    want = {"AdamW": HipAdamW, "Lion": HipLion, "Lamb": HipLamb, "SGD": HipSGD}
    for kind, cls in want.items():
        opt = get_optimizer(_config(kind), 2e-3, [m])
        assert type(opt) is cls and opt.param_groups[0]["lr"] == 2e-3 and len(opt.param_groups) == 1
        g = opt.param_groups[0]
        if kind == "SGD":
            assert g["momentum"] == 0.9 and g["weight_decay"] == 0 and g["dampening"] == 0 and g["nesterov"] is False
        else:
            assert tuple(g["betas"]) == (0.9, 0.95) and g["weight_decay"] == 5e-3
        if kind == "Lamb":
            assert g["eps"] == 1e-6
        assert m._managed_updates
    for bad in ("Adam", "lion", "RMSprop"):
        with pytest.raises(NotImplementedError, match="Unknown optimizer: " + bad):
            get_optimizer(_config(bad), 1e-3, [m])
    # the defaults of the reference's classes / torch.optim.SGD
    assert HipLion(m).defaults == dict(lr=1e-4, betas=(0.9, 0.99), weight_decay=0.0)
    assert HipLamb(m).defaults == dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0)
    assert HipSGD(m).defaults["momentum"] == 0.0 and HipSGD(m).defaults["lr"] == 1e-3
    # invalid arguments: Lion asserts, as the reference's does; Lamb and SGD raise ValueError, as theirs do
    with pytest.raises(AssertionError):
        HipLion(m, lr=0.0)
    for bad in (dict(lr=-1.0), dict(eps=-1e-6), dict(betas=(1.0, 0.9)), dict(betas=(0.9, -0.1))):
        with pytest.raises(ValueError):
            HipLamb(m, **bad)
    with pytest.raises(ValueError):
        HipSGD(m, lr=-1.0)


@pytest.mark.parametrize("kind", R.KINDS)
def test_step_fails_loudly_without_gpu(lib, kind):
    from headct_foundation_amd import HctError
    from headct_foundation_amd.optim import get_optimizer
    _, m = _micro()
    opt = get_optimizer(_config(kind), 1e-3, [m])
    with pytest.raises(HctError, match="no CPU fallback"):
        opt.step()


@pytest.mark.parametrize("kind", R.KINDS)
def test_state_dict_interchange_with_the_torch_side_optimizer(lib, kind):
    """Key manifests equal the reference's (fixture), and a state dict written by the torch-side optimizer (the reference's layout:
    tests/optim_ref.py, torch.optim.SGD) loads into the Hip class on a CPU-resident model and comes back equal -- and the other way
    round."""
    from headct_foundation_amd.optim import get_optimizer
    fx = load_golden("optimizers")["manifests"]
    man = fx[kind]  # `Lamb`: the class get_optimizer names, whose layout the state dict keeps
    cfg, m = _micro()
    ref_params = [torch.nn.Parameter(p.detach().clone()) for p in m.parameters()]
    ref = R.torch_optimizer(kind, ref_params, 1e-3)
    for s in range(2):
        for k, p in enumerate(ref_params):
            p.grad = torch.from_numpy(O.hash_uniform(p.numel(), 50 + 7 * s + k)).reshape(p.shape) * 0.1
        ref.step()
    rsd = ref.state_dict()
    assert sorted(rsd["param_groups"][0]) == man["param_group_keys"]
    assert {tuple(sorted(v)) for v in rsd["state"].values()} == {tuple(v) for v in man["state_keys"].values()}
    opt = get_optimizer(_config(kind), 1e-3, [m])
    opt._ensure_state()
    sd0 = opt.state_dict()
    assert sorted(sd0["param_groups"][0]) == man["param_group_keys"] and man["n_groups"] == len(sd0["param_groups"]) == 1
    trainable = [i for i, p in enumerate(m.parameters()) if p.requires_grad]
    assert sorted(sd0["state"]) == trainable and sd0["param_groups"][0]["params"] == list(range(len(ref_params)))
    assert {tuple(sorted(v)) for v in sd0["state"].values()} == {tuple(v) for v in man["state_keys"].values()}
    opt.load_state_dict(rsd)
    sd = opt.state_dict()
    for i in trainable:
        for k, v in rsd["state"][i].items():
            got = sd["state"][i][k]
            if k == "step":
                assert got == v and isinstance(got, int)
            else:
                assert torch.equal(torch.as_tensor(got), torch.as_tensor(v).float()), (i, k)
    if kind == "Lamb":
        assert opt._step_count_fused == 2
    # the state lives in the flat buffers: per-parameter entries are views of them
    key = R.STATE_KEYS[kind][0]
    flat = opt._flat_buffer(key)
    named = dict(m.named_parameters())
    for name, off, numel, shape, rg, _ in m._layout:
        if named[name].requires_grad:
            assert opt.state[named[name]][key].data_ptr() == flat[off:off + numel].data_ptr()
    # ... and back into the torch-side class
    ref2 = R.torch_optimizer(kind, [torch.nn.Parameter(p.detach().clone()) for p in m.parameters()], 1e-3)
    ref2.load_state_dict(sd)
    back = ref2.state_dict()
    for i in trainable:
        for k, v in rsd["state"][i].items():
            assert torch.equal(torch.as_tensor(back["state"][i][k]).float(), torch.as_tensor(v).float()), (i, k)


def test_adamw_state_dict_keeps_each_parameters_own_step(lib):
    """torch.optim.AdamW counts steps per parameter (one with `grad is None` is passed over).  A torch state dict whose counts differ
    loads into HipAdamW with every count kept (it used to take the maximum for all), state_dict() writes them back, and a
    parameter torch has no state for yet comes back with step 0 and zero moments, which torch.optim.AdamW loads as a fresh one."""
    from headct_foundation_amd import HipAdamW
    _, m = _micro()
    ref_params = [torch.nn.Parameter(p.detach().clone()) for p in m.parameters()]
    ref = torch.optim.AdamW(ref_params, lr=1e-3, betas=(0.9, 0.999), weight_decay=5e-3)
    trainable = [i for i, p in enumerate(m.parameters()) if p.requires_grad]
    late, never = trainable[1], trainable[2]
    for s in range(4):
        for k, p in enumerate(ref_params):
            live = k in trainable and k != never and (k != late or s >= 3)
            p.grad = torch.from_numpy(O.hash_uniform(p.numel(), 70 + 11 * s + k)).reshape(p.shape) * 0.1 if live else None
        ref.step()
    rsd = ref.state_dict()
    assert int(rsd["state"][late]["step"]) == 1 and int(rsd["state"][trainable[0]]["step"]) == 4 and never not in rsd["state"]
    opt = HipAdamW(m, lr=1e-3, betas=(0.9, 0.999), weight_decay=5e-3)
    opt.load_state_dict(rsd)
    sd = opt.state_dict()
    assert sorted(sd["state"]) == trainable
    for i in trainable:
        want = rsd["state"].get(i)
        assert int(sd["state"][i]["step"]) == (int(want["step"]) if want else 0), i
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(sd["state"][i][k], want[k].float()) if want else not sd["state"][i][k].any(), (i, k)
    names = m.flat_segments()[0]
    by_name = {n: i for i, (n, _) in enumerate(m.named_parameters())}
    assert [int(c) for c in opt._seg_steps] == [int(rsd["state"][by_name[n]]["step"]) if by_name[n] in rsd["state"] else 0 for n in names]
    ref2 = torch.optim.AdamW([torch.nn.Parameter(p.detach().clone()) for p in m.parameters()], lr=1e-3)
    ref2.load_state_dict(sd)
    assert [int(ref2.state_dict()["state"][i]["step"]) for i in trainable] == [int(sd["state"][i]["step"]) for i in trainable]


def test_sgd_without_momentum_keeps_no_state(lib):
    from headct_foundation_amd import HipSGD
    _, m = _micro()
    opt = HipSGD(m, lr=1e-2, momentum=0.0)
    opt._ensure_state()
    assert opt.state_dict()["state"] == {} == torch.optim.SGD([torch.nn.Parameter(torch.zeros(2))], lr=1e-2).state_dict()["state"]


def test_dino_optimizer_kinds(lib):
    """DinoOptimizer builds two fused optimizers of the requested kind; the merged state dict has the kind's own keys and splits back."""
    from headct_foundation_amd import HipAdamW, HipLamb, HipLion, HipSGD
    from headct_foundation_amd.dino import DinoOptimizer
    from headct_foundation_amd.dino_model import DINOHead, MultiCropWrapper, ViTBackbone
    b = ViTBackbone(img_size=32, patch_size=16, in_chans=1, hidden_size=48, mlp_dim=96, num_layers=1, num_heads=2)
    h = DINOHead(in_dim=48, out_dim=64, hidden_dim=32, bottleneck_dim=16)
    model = MultiCropWrapper(b, h)
    nb, nh = len(list(b.parameters())), len(list(h.parameters()))
    for kind, cls in (("AdamW", HipAdamW), ("Lion", HipLion), ("Lamb", HipLamb), ("SGD", HipSGD)):
        opt = DinoOptimizer(model, lr=1e-3, betas=(0.9, 0.95), weight_decay=0.04, kind=kind, momentum=0.9)
        assert type(opt.primary) is cls and type(opt.secondary) is cls and opt.param_groups is opt.primary.param_groups
        opt.primary._ensure_state()
        opt.secondary._ensure_state()
        sd = opt.state_dict()
        assert sd["param_groups"][0]["params"] == list(range(nb + nh)) and len(sd["param_groups"]) == 1
        keys = {"AdamW": {"step", "exp_avg", "exp_avg_sq"}, "Lion": {"exp_avg"}, "SGD": {"momentum_buffer"},
                "Lamb": {"step", "exp_avg", "exp_avg_sq", "weight_norm", "adam_norm", "trust_ratio"}}[kind]
        assert all(set(v) == keys for v in sd["state"].values()) and max(sd["state"]) >= nb
        opt.load_state_dict(sd)
        sd2 = opt.state_dict()
        assert sorted(sd2["state"]) == sorted(sd["state"])
    assert DinoOptimizer(model, lr=1e-3).kind == "AdamW"  # the default stays AdamW
    with pytest.raises(NotImplementedError, match="Unknown optimizer: Adagrad"):
        DinoOptimizer(model, lr=1e-3, kind="Adagrad")


@pytest.mark.parametrize("kind,sched", R.curve_runs())
def test_mae_curve_of_the_restatement(kind, sched):
    """The restatement's 4-step `micro` loss curve and rates against the reference's own train_one_epoch (fixture): 6e-5 absolute on
    the loss the reference logs with 4 decimals (make_golden.run_case's bar), rates to 1e-12."""
    fx = next(c for c in load_golden("optimizers")["curves"] if c["optimizer"] == kind and c["scheduler"] == sched)
    cfg = O.CONFIGS[fx["config"]]
    hp = fx["hp"]
    assert hp == dict(R.CURVE_HP, base_lr=R.CURVE_LR[kind])
    st = R.TrainState(O.make_params(cfg, fx["seed"]))
    losses, lrs = [], []
    for i in range(fx["steps"]):
        l, lr, _ = R.train_step(cfg, st, O.make_volume(cfg, fx["batch"], fx["seed"] + 10 + i), O.make_noise(cfg, fx["batch"], fx["seed"] + 10 + i),
                                kind, sched, **hp)
        losses.append(l)
        lrs.append(lr)
    assert np.allclose(lrs, fx["lrs"], rtol=1e-12, atol=0) and np.allclose(losses, fx["logged_losses"], atol=6e-5)
    assert losses[-1] < losses[0]
    if fx["params_after"]:
        for k, entry in fx["params_after"].items():
            got, want, _, _ = sample_of(st.params[k], entry)
            assert torch.allclose(got, want, rtol=1e-4, atol=4 * hp["base_lr"] if k.endswith("qkv.bias") else 1e-5), k


def test_lion_sign_ties_on_micro_stay_under_the_cap():
    """The GPU test compares Lion element by element except where c = beta1*m + (1-beta1)*g cancels to rounding (|c| <= 1e-5 * (beta1*|m|
    + (1-beta1)*|g|) in the fp64 restatement at any step so far) and caps that set at 1e-4 of the model's elements.  Here, with oracle
    gradients on `micro` (batch 2, 4 steps): the set stays under the cap, and the fp32 and fp64 restatements fed the same gradients
    never disagree on a sign outside it."""
    cfg = O.CONFIGS["micro"]
    hp = dict(R.CURVE_HP, base_lr=R.CURVE_LR["Lion"])
    st = R.TrainState(O.make_params(cfg, 0))
    m64, excused, total = {}, {}, 0
    for i in range(4):
        before = {k: v["exp_avg"].clone() for k, v in st.state.items()}
        _, lr, grads = R.train_step(cfg, st, O.make_volume(cfg, 2, 10 + i), O.make_noise(cfg, 2, 10 + i), "Lion", "constant", **hp)
        for k, g in grads.items():
            m = m64.setdefault(k, torch.zeros_like(g, dtype=torch.float64))
            c64 = m * hp["beta1"] + g.double() * (1 - hp["beta1"])
            ex = R.lion_excused(c64, m, g.double(), hp["beta1"])
            excused[k] = excused.get(k, torch.zeros_like(ex)) | ex
            c32 = before.get(k, torch.zeros_like(g)) * hp["beta1"] + g * (1 - hp["beta1"])
            assert torch.equal(torch.sign(c32)[~excused[k]].double(), torch.sign(c64)[~excused[k]]), k
            m.mul_(hp["beta2"]).add_(g.double(), alpha=1 - hp["beta2"])
    total = sum(p.numel() for p in st.params.values())
    n_ex = sum(int(e.sum()) for e in excused.values())
    print(f"excused {n_ex} of {total} elements")
    assert total == 115424 and n_ex <= int(1e-4 * total)


def test_new_symbols_are_declared_bound_and_exported(lib):
    from headct_foundation_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "headct_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(hct_[a-z0-9_]+)\s*\(", hdr))
    raw = C.CDLL(_lib.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert s in declared and s in _lib.exported_symbols() and hasattr(raw, s), s
    # host arithmetic, no device call: two floats per 1024-element unit
    assert lib.hct_lamb_workspace_bytes(1024 * 10, 3) == 80 and lib.hct_lamb_workspace_bytes(1, 1) == 8
    # argument checks come back as error codes with a message, before any launch
    assert lib.hct_lion_step(None, None, None, None, None, None, 1, 1024, 1e-3, 0.9, 0.99, 0.0, None, None) != 0
    assert b"hct_lion_step" in lib.hct_last_error_string()
    assert lib.hct_sgd_step(None, None, None, None, None, None, 1, 1000, 1e-3, 0.9, None, None) != 0
    assert lib.hct_lamb_step(None, None, None, None, None, None, None, 1, 1024, 1e-3, 0.9, 0.95, 1e-6, 0.0, None, None, None, None, 0, None, None) != 0
