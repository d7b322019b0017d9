"""CPU: the yardstick of the optimizer kernel tests (tests/optim_kernel_ref.py) is itself checked here.
  * against torch: its AdamW (per-segment step count, skipped-then-live schedule included) and SGD are torch.optim's, its Lion and
    Lamb reproduce tests/golden/optimizers.json on a flat layout;
  * the bars pass what is right: the fp32 restatement (torch fp32, the reference's operation order) stays within MEASURED on every
    case, the bars are 4 x that (floor 2) and none passes 16; Lion's excused share of every case is printed and stays <= 1e-5;
  * the bars bite: each deliberately wrong restatement (fp64, so that only the mistake shows) fails its bar on at least one case.
"""
import functools
import math

import numpy as np
import pytest
import torch

from tests import optim_kernel_ref as KR
from tests import optim_ref as R
from tests.util import load_golden, sample_of


@functools.lru_cache(maxsize=None)
def _case(case_name, kind):
    case = next(c for c in KR.all_cases(kind) if c.name == case_name)
    pre = KR.inputs(case)
    hp = KR.abi_hp(kind, case.hp)
    return case, pre, hp, KR.one_step(kind, pre, hp)


def _cases(kind):
    return [_case(c.name, kind) for c in KR.all_cases(kind)]


def _count_pres(betas):
    """Case F as one-step problems: the pre-step state of torch.optim.AdamW (fp64 -> fp32) at every step of the schedule."""
    ci = KR.count_inputs(betas)
    hp = KR.abi_hp("AdamW", ci["hp"])
    seg = ci["seg"]
    p = ci["p"].clone()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    counts = [0] * (len(seg) - 1)
    for step in range(KR.COUNT_STEPS):
        live = KR.count_schedule(step)
        counts = [c + int(l) for c, l in zip(counts, live)]
        pre = {"seg": seg, "p": p, "g": ci["grads"][step], "state": {"exp_avg": m, "exp_avg_sq": v},
               "skip": torch.tensor([0 if l else 1 for l in live], dtype=torch.uint8), "steps": torch.tensor(counts, dtype=torch.int32)}
        ref = KR.one_step("AdamW", pre, hp)
        yield step, pre, hp, ref
        p, m, v = ref["p"].float(), ref["state"]["exp_avg"].float(), ref["state"]["exp_avg_sq"].float()


# ---- against torch and the fixture ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.9, 0.95)])
def test_adamw_counts_per_segment_like_torch(betas):
    """The restatement chained over case F (one segment live throughout, one without a gradient for the first 5 of 8 steps, one never
    live) against torch.optim.AdamW in fp64: 1e-12 of the largest parameter at every step, and the step counts torch ends with."""
    ci = KR.count_inputs(betas)
    hp = KR.abi_hp("AdamW", ci["hp"])
    seg = ci["seg"]
    hist, opt = KR.torch_adamw_run(ci)
    pre = {"seg": seg, "p": ci["p"].double(), "state": {"exp_avg": torch.zeros(seg[-1], dtype=torch.float64), "exp_avg_sq": torch.zeros(seg[-1], dtype=torch.float64)}}
    counts = [0, 0, 0]
    for step in range(KR.COUNT_STEPS):
        live = KR.count_schedule(step)
        counts = [c + int(l) for c, l in zip(counts, live)]
        pre.update(g=ci["grads"][step].double(), skip=[0 if l else 1 for l in live], steps=counts)
        out = KR.one_step("AdamW", pre, hp)
        for s, (a, b) in enumerate(zip(seg, seg[1:])):
            assert float((out["p"][a:b] - hist[step][s]).abs().max()) <= 1e-12, (step, s)
        pre.update(p=out["p"], state=out["state"])
    assert counts == [KR.COUNT_STEPS, KR.COUNT_STEPS - KR.COUNT_LATE, 0]
    steps = [int(opt.state[q]["step"]) if opt.state[q] else 0 for q in opt.param_groups[0]["params"]]
    assert steps == counts
    assert torch.equal(out["p"][seg[2]:], ci["p"][seg[2]:].double())


def test_a_late_segment_starts_its_bias_correction_at_one():
    """What the count per segment is for: the first live update of a segment that sat out 5 steps is lr * sign(g) (eps aside), as
    torch's is, not the 0.52 lr that the count of the other segments would give (betas 0.9 / 0.999)."""
    _, pre, hp, ref = next(x for x in _count_pres((0.9, 0.999)) if x[0] == KR.COUNT_LATE)
    a, b = pre["seg"][1], pre["seg"][2]
    g = pre["g"][a:b].double()
    keep = 1.0 - hp["lr"] * hp["weight_decay"]
    upd = (ref["p"][a:b] - pre["p"][a:b].double() * keep) / hp["lr"]
    big = g.abs() > 1e-3
    assert int(big.sum()) > 100 and float((upd[big] + torch.sign(g[big])).abs().max()) < 1e-4
    wrong = dict(pre, steps=torch.full((3,), KR.COUNT_LATE + 1, dtype=torch.int32))
    upd_wrong = (KR.one_step("AdamW", wrong, hp)["p"][a:b] - pre["p"][a:b].double() * keep) / hp["lr"]
    assert abs(float(upd_wrong[big].abs().mean()) - 0.52) < 0.01


@pytest.mark.parametrize("momentum", [0.0, 0.9])
def test_sgd_is_torch_sgd(momentum):
    units = KR.LAYOUTS["trips"][4:]
    seg = KR.offsets(units)
    rng = np.random.default_rng(5)
    p0 = torch.from_numpy(rng.uniform(-1, 1, seg[-1]))
    ps = [torch.nn.Parameter(p0[a:b].clone()) for a, b in zip(seg, seg[1:])]
    opt = torch.optim.SGD(ps, lr=1e-2, momentum=momentum, foreach=False)
    pre = {"seg": seg, "p": p0.clone(), "state": {} if momentum == 0 else {"momentum_buffer": torch.zeros_like(p0)}}
    hp = dict(lr=1e-2, momentum=momentum, weight_decay=0.0)
    for step in range(3):
        g = torch.from_numpy(rng.normal(size=seg[-1]))
        live = [True, step != 1, True]
        for s, (q, (a, b)) in enumerate(zip(ps, zip(seg, seg[1:]))):
            q.grad = g[a:b].clone() if live[s] else None
        opt.step()
        pre.update(g=g, skip=[0 if l else 1 for l in live])
        out = KR.one_step("SGD", pre, hp)
        for q, (a, b) in zip(ps, zip(seg, seg[1:])):
            assert float((out["p"][a:b] - q.detach()).abs().max()) <= 1e-14
        pre.update(p=out["p"], state=out["state"])


@pytest.mark.parametrize("kind", ["Lion", "Lamb"])
def test_lion_and_lamb_reproduce_the_fixture_on_a_flat_layout(kind):
    """tests/golden/optimizers.json (the reference's own classes, fp32) through one_step: the tensor cases laid end to end as the
    segments of one flat buffer, the gradient-less one skipped; same samples and tolerance as tests/test_optim_cpu.py."""
    fx = load_golden("optimizers")["tensors"][kind]
    hp = dict(R.HP, eps=R.LAMB_EPS)
    params = R.case_params()
    names = list(params)
    seg = [0]
    for n in names:
        seg.append(seg[-1] + params[n].numel())
    pre = {"seg": seg, "p": torch.cat([params[n].reshape(-1) for n in names]),
           "state": {k: torch.zeros(seg[-1]) for k in KR.STATE_KEYS[kind]}}
    for step, want in enumerate(fx["steps"]):
        grads = R.case_grads(step)
        pre.update(g=torch.cat([(grads[n] if grads[n] is not None else torch.zeros_like(params[n])).reshape(-1) for n in names]),
                   skip=[1 if grads[n] is None else 0 for n in names])
        out = KR.one_step(kind, pre, hp, torch.float32)
        for s, n in enumerate(names):
            got, ref, l2, l2w = sample_of(out["p"][seg[s]:seg[s + 1]].reshape(params[n].shape), want["params"][n])
            assert abs(l2 - l2w) <= 1e-6 * l2w + 1e-30 and float((got - ref).abs().max()) <= 1e-6 * float(ref.abs().max()) + 1e-30, (step, n)
        pre.update(p=out["p"], state=out["state"])


# ---- the bars pass what is right -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KR.KINDS)
def test_fp32_restatement_within_measured(kind):
    """The fp32 restatement against fp64 on every case, in units of 2^-24 * S per quantity: within MEASURED (the values the bars
    are 4 x of), hence within every bar; Lion's excused share per case printed, <= 1e-5 of each tensor."""
    worst = {}
    runs = [(c.name, pre, hp, ref) for c, pre, hp, ref in _cases(kind)]
    if kind == "AdamW":
        runs += [(f"count-{betas[1]}-step{step}", pre, hp, ref) for betas in ((0.9, 0.999), (0.9, 0.95)) for step, pre, hp, ref in _count_pres(betas)]
    for name, pre, hp, ref in runs:
        got = KR.one_step(kind, pre, hp, torch.float32)
        w = KR.check(kind, pre, got, hp, ref=ref)
        if kind == "Lion":
            print(f"{name}: excused share {w['excused']:.2e}")
            assert w.pop("excused") <= KR.LION_TOL_SHARE, name
        for q, x in w.items():
            worst[q] = max(worst.get(q, 0.0), x)
    print(kind, {q: round(x, 3) for q, x in worst.items()})
    for q, x in KR.MEASURED[kind].items():
        assert worst[q] <= x, (q, worst[q], x)
        assert KR.K[kind][q] == max(2.0, 4.0 * x) and KR.K[kind][q] <= 16.0, (q, KR.K[kind][q])


def test_fold_bound_counts_the_chain():
    """1 unit: 1 + 2 + 6 + 2 roundings to the unit's sum, 8 more in the block tree, halved by the root, + 1; each trip past the first
    adds one addition."""
    assert KR.fold_k(1) == KR.fold_k(256) == 10.5 and KR.fold_k(257) == 11.0 and KR.fold_k(513) == 11.5
    assert max(KR.diag_k(513).values()) == 11.5 + 11.5 + KR.K["Lamb"]["adam_norm"] + 2


def test_cases_hold_the_regimes():
    """What the issue lists is really in the inputs: the two trips past 256 units, a zero-gradient and a zero-parameter segment,
    ||p|| on both sides of 10, every (lr scale, wd scale) pair next to a different one, energy in the hot units, eps-sized gradients."""
    _, pre, hp, ref = _case("lamb-wd0.01-s1-trips", "Lamb")
    seg, units = pre["seg"], pre["units"]
    assert units == [1, 257, 1, 513, 2, 256, 1] and KR.hot_units(257) == [256] and KR.hot_units(513) == [256, 512] and KR.hot_units(256) == []
    w = ref["diag"]["weight_norm"]
    assert float(w[0]) < 10 and float(w[1]) == 10 and float(w[2]) == 0 and float(ref["diag"]["trust_ratio"][2]) == 1
    for s in (1, 3):
        a = seg[s]
        hot = torch.zeros(units[s] * KR.UNIT, dtype=torch.bool)
        for u in KR.hot_units(units[s]):
            hot[u * KR.UNIT:(u + 1) * KR.UNIT] = True
        for x in (pre["p"][a:seg[s + 1]].double(), ):
            assert float((x[hot] ** 2).sum()) > 0.9 * float((x ** 2).sum()), s
        g = _case("adamw-trips", "AdamW")[1]["g"][a:seg[s + 1]].double()
        assert float((g[hot] ** 2).sum()) > 0.9 * float((g ** 2).sum()), s
    _, pre0, _, ref0 = _case("lamb-wd0.0-s0-many", "Lamb")
    z = pre0["zero_g"]
    assert not pre0["g"][pre0["seg"][z]:pre0["seg"][z + 1]].any() and float(ref0["diag"]["adam_norm"][z]) == 0 and float(ref0["diag"]["trust_ratio"][z]) == 1
    _, pa, _, _ = _case("adamw-scaled-s1", "AdamW")
    pairs = {(float(a), float(b)) for a, b in zip(pa["lr_scale"], pa["wd_scale"])}
    assert len(pairs) == 12 and int(pa["skip"].sum()) > 10 and int((pa["coef"] == 1).sum()) > 40
    assert float((pa["g"].abs() < 1e-8).double().mean()) > 0.1  # eps decides these


# ---- the bars bite -------------------------------------------------------------------------------------------------------------------
def _seg_consts(pre, hp, s, nb=0):
    n = len(pre["seg"]) - 1
    j = (s + nb) % n
    ls = float(pre["lr_scale"][j]) if pre.get("lr_scale") is not None else 1.0
    ws = float(pre["wd_scale"][j]) if pre.get("wd_scale") is not None else 1.0
    return hp["lr"] * ls, hp["weight_decay"] * ws


def _wrong_adamw(pre, hp, wrong=None):
    """AdamW written out in fp64 with one switchable mistake; wrong=None is right (and must pass every bar)."""
    seg = pre["seg"]
    n = len(seg) - 1
    p, g, m, v = (x.double().clone() for x in (pre["p"], pre["g"], pre["state"]["exp_avg"], pre["state"]["exp_avg_sq"]))
    b1, b2, eps = hp["beta1"], hp["beta2"], hp["eps"]
    for s, (a, b) in enumerate(zip(seg, seg[1:])):
        if pre.get("skip") is not None and int(pre["skip"][s]):
            continue
        c = float(pre["coef"][(s + 1) % n if wrong == "neighbour_coef" else s]) if pre.get("coef") is not None else 1.0
        raw = g[a:b].clone()
        gc = raw * c
        if wrong != "no_write_back":
            g[a:b] = gc
        lr_s, wd_s = _seg_consts(pre, hp, s, 1 if wrong == "neighbour_scales" else 0)
        t = int(pre["steps"][s])
        t = {"step_plus": t + 1, "step_minus": t - 1, "global_step": int(max(pre["steps"]))}.get(wrong, t)
        m[a:b] = b1 * m[a:b] + (1 - b1) * gc
        sq = raw * raw if wrong == "square_before_clip" else gc * gc
        v[a:b] = b2 * v[a:b] + (b2 if wrong == "beta2_twice" else 1 - b2) * sq
        bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
        den = (v[a:b] / bc2 + eps).sqrt() if wrong == "eps_in_root" else v[a:b].sqrt() / math.sqrt(bc2) + eps
        keep = 1.0 if wrong == "no_decay" else 1 - lr_s * wd_s
        p[a:b] = p[a:b] * keep - lr_s / bc1 * m[a:b] / den
    return {"p": p, "g": g, "state": {"exp_avg": m, "exp_avg_sq": v}, "diag": {}}


def _wrong_lamb(pre, hp, wrong=None):
    seg = pre["seg"]
    p, g, m, v = (x.double().clone() for x in (pre["p"], pre["g"], pre["state"]["exp_avg"], pre["state"]["exp_avg_sq"]))
    diag = {k: torch.full((len(seg) - 1,), float("nan"), dtype=torch.float64) for k in KR.DIAG}
    b1, b2, eps = hp["beta1"], hp["beta2"], hp["eps"]
    for s, (a, b) in enumerate(zip(seg, seg[1:])):
        if pre.get("skip") is not None and int(pre["skip"][s]):
            continue
        g[a:b] *= float(pre["coef"][s])
        lr_s, wd_s = _seg_consts(pre, hp, s)
        m[a:b] = b1 * m[a:b] + (1 - b1) * g[a:b]
        v[a:b] = b2 * v[a:b] + (1 - b2) * g[a:b] ** 2
        u = m[a:b] / (v[a:b].sqrt() + eps) + wd_s * p[a:b]
        w, an = p[a:b].norm().clamp(0, 10), u.norm()
        r = 1.0 if float(w) == 0 or float(an) == 0 else float(w / (an + eps))
        if wrong == "other_wd_in_update":
            u = m[a:b] / (v[a:b].sqrt() + eps) + hp["weight_decay"] * p[a:b]  # the launch scalar, not the segment's
        p[a:b] = p[a:b] - lr_s * r * u
        diag["weight_norm"][s], diag["adam_norm"][s], diag["trust_ratio"][s] = w, an, r
    return {"p": p, "g": g, "state": {"exp_avg": m, "exp_avg_sq": v}, "diag": diag}


def _fails_somewhere(kind, fn, wrong, quantity):
    """True if `fn(pre, hp, wrong)` misses the bar of `quantity` on at least one case; the right version passes all of them."""
    failed = 0
    runs = [(pre, hp, ref) for _, pre, hp, ref in _cases(kind)]
    if kind == "AdamW":
        runs += [(pre, hp, ref) for _, pre, hp, ref in _count_pres((0.9, 0.999))]
    for pre, hp, ref in runs:
        KR.check(kind, pre, fn(pre, hp, None), hp, ref=ref)
        try:
            KR.check(kind, pre, fn(pre, hp, wrong), hp, ref=ref)
        except AssertionError as e:
            assert f" {quantity} segment" in str(e), (wrong, str(e))
            failed += 1
    return failed


@pytest.mark.parametrize("wrong,quantity", [("eps_in_root", "p"), ("global_step", "p"), ("step_plus", "p"), ("step_minus", "p"), ("no_decay", "p"),
                                            ("beta2_twice", "exp_avg_sq"), ("square_before_clip", "exp_avg_sq"), ("neighbour_coef", "g"),
                                            ("neighbour_scales", "p"), ("no_write_back", "g")])
def test_wrong_adamw_fails_its_bar(wrong, quantity):
    """eps inside the root, the bias correction at the count of the other segments, step +- 1, no decay, beta2 where 1 - beta2
    belongs, g^2 before the clip coefficient, the neighbour's coefficient / scales, the clipped gradient not written back."""
    runs = _fails_somewhere("AdamW", _wrong_adamw, wrong, quantity) if wrong != "step_minus" else None
    if wrong == "step_minus":  # a count of 0 divides by zero: only the cases past the first step
        runs = 0
        for case, pre, hp, ref in _cases("AdamW"):
            if case.step > 1:
                try:
                    KR.check("AdamW", pre, _wrong_adamw(pre, hp, wrong), hp, ref=ref)
                except AssertionError:
                    runs += 1
    print(wrong, "fails on", runs, "cases")
    assert runs >= 1


def test_wrong_lamb_fails_its_bar():
    """u recomputed in the update with another decay than the one whose norm went into the trust ratio."""
    assert _fails_somewhere("Lamb", _wrong_lamb, "other_wd_in_update", "p") >= 1


def test_wrong_lion_without_decay_fails_its_bar():
    failed = 0
    for case, pre, hp, ref in _cases("Lion"):
        got = KR.one_step("Lion", pre, dict(hp, weight_decay=0.0))
        try:
            KR.check("Lion", pre, got, hp, ref=ref)
        except AssertionError:
            failed += 1
        else:
            assert hp["weight_decay"] == 0 or hp["lr"] == 0, case.name
    assert failed >= 1


@pytest.mark.parametrize("wrong", ["last_unit", "second_trip"])
def test_wrong_norm_fold_fails_its_bar(wrong):
    """The last unit of a segment, or the units of the loop trips past the first, left out of the fold: off by a large factor on the
    257- and 513-unit segments, whose energy sits there."""
    _, pre, _, _ = _case("adamw-trips", "AdamW")
    seg, g = pre["seg"], pre["g"]
    right = KR.seg_norms(g.double(), seg)
    KR.check_norms(g, seg, 3.0, right.float(), KR.clip_coef(right, 3.0).float())
    bad = right.clone()
    for s, (a, b) in enumerate(zip(seg, seg[1:])):
        cut = b - KR.UNIT if wrong == "last_unit" else min(b, a + 256 * KR.UNIT)
        bad[s] = g[a:cut].double().norm()
    assert float(bad[1]) < 0.1 * float(right[1]) and float(bad[3]) < 0.9 * float(right[3])  # one of one, one or two of three hot units
    with pytest.raises(AssertionError, match="norm of segment"):
        KR.check_norms(g, seg, 3.0, bad.float(), KR.clip_coef(bad, 3.0).float())


def test_truncated_shadow_fails():
    """bf16 by truncation where rounding to nearest even belongs."""
    _, pre, hp, ref = _case("adamw-one", "AdamW")
    p = ref["p"].float()
    before = torch.zeros(p.numel(), dtype=torch.bfloat16)
    KR.check_shadow(p, p.to(torch.bfloat16), before, pre)
    trunc = (p.view(torch.int32) & ~0xFFFF).view(torch.float32).to(torch.bfloat16)
    with pytest.raises(AssertionError, match="shadow of segment"):
        KR.check_shadow(p, trunc, before, pre)


def test_counts_entry_point_is_declared(lib):
    """hct_adamw_step_counts: in the header, in _lib's prototypes, exported, and loud about bad arguments."""
    import os
    from headct_foundation_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "headct_hip.h")).read()
    assert "int hct_adamw_step_counts(" in header and "hct_adamw_step_counts" in _lib._PROTOS and hasattr(lib, "hct_adamw_step_counts")
    assert lib.hct_adamw_step_counts(None, None, None, None, None, None, None, 1, 1024, 1e-3, 0.9, 0.95, 1e-8, 0.0, None, None, None, None, None) != 0
    assert b"hct_adamw_step_counts" in lib.hct_last_error_string()
