"""The yardstick of tests/test_optim_kernels_gpu.py and tests/test_optim_kernel_ref_cpu.py: ONE step of the per-tensor clip and of
AdamW / Lion / SGD / Lamb over a flat buffer cut into segments, in the dtype asked for (fp64 = the yardstick, fp32 = the reference's
own arithmetic, whose distance from fp64 sets the bars), the inputs of the cases both files run, and the per-element bounds.

The update formulas are not restated here: they are oracle.mae_oracle.adamw_step_ and tests/optim_ref.py through
tests/param_scales_ref.apply_scaled_, pinned to the reference by tests/golden/optimizers.json.  What this file adds is the flat
layout (seg_off, deferred clip coefficient, skip mask, per-segment scales) and AdamW's step count PER SEGMENT, which is what
torch.optim.AdamW keeps (src/utils/optimizers.py:354-360): a parameter with `grad is None` is passed over and its count starts
with its first gradient.

Comparisons are one step deep: the kernel's own pre-step fp32 p, g, m, v go into the fp64 restatement and the post-step values are
compared, so nothing accumulates.  A bound is k * 2^-24 * S per element, S the magnitude of what enters the quantity's last
operation (`scales`), k a count of roundings (`K`).
"""
import contextlib
import math
import zlib
from typing import Dict, List, NamedTuple, Optional

import numpy as np
import torch

from tests import optim_ref as R
from tests import param_scales_ref as PS

UNIT = 1024
U24 = 2.0 ** -24
KINDS = PS.KINDS
STATE_KEYS = PS.STATE_KEYS
DIAG = ("weight_norm", "adam_norm", "trust_ratio")
LION_TOL_SHARE = 1e-5  # a tenth of the cap tests/test_optim_gpu.py allows (optim_ref.lion_excused)
LION_CAP = 1e-4

# units of 1024 elements per segment
LAYOUTS = {
    "one": [1],
    "few": [1, 2, 1],                      # the skip sequences
    "many": [1] * 131,                     # no power of two: the binary search of find_segment ends at every index
    "trips": [1, 257, 1, 513, 2, 256, 1],  # 257 / 513 units: a second and a third trip of the 256-thread folds
}


def offsets(units: List[int]) -> List[int]:
    seg = [0]
    for u in units:
        seg.append(seg[-1] + u * UNIT)
    return seg


def f32(x) -> float:
    """What a `float` argument of the C ABI holds: hct_adamw_step* take lr, the betas, eps and the decay as floats, and the
    yardstick is given those values, not the doubles they were rounded from (0.999f = 0.99900001287, whose 1 - beta2 differs
    from 1e-3 by 1.3e-5 of it: a property of the call's signature, not an error of the arithmetic)."""
    return float(np.float32(x))


def abi_hp(kind: str, hp: dict) -> dict:
    if kind != "AdamW":
        return dict(hp)  # Lion / SGD / Lamb take doubles
    return {k: (f32(v) if k in ("lr", "weight_decay", "beta1", "beta2", "eps") else v) for k, v in hp.items()}


# ---- the clip (src/utils/misc.py:374-383) ------------------------------------------------------------------------------------------
def seg_norms(g: torch.Tensor, seg: List[int]) -> torch.Tensor:
    return torch.stack([g[a:b].norm(2) for a, b in zip(seg, seg[1:])])


def clip_coef(norms: torch.Tensor, clip: float) -> torch.Tensor:
    """coef = clip / (norm + 1e-6), applied iff < 1: an infinite norm gives 0, a NaN norm compares false and stays unclipped."""
    one = torch.ones_like(norms)
    if not clip > 0:
        return one
    c = clip / (norms + 1e-6)
    return torch.where(c < 1, c, one)


def scaled_grad(g: torch.Tensor, seg: List[int], coef: torch.Tensor) -> torch.Tensor:
    """g * coef per segment, one product per element; a coefficient of exactly 1 leaves the bits."""
    out = g.clone()
    for s, (a, b) in enumerate(zip(seg, seg[1:])):
        if float(coef[s]) != 1.0:
            out[a:b] *= float(coef[s])
    return out


@contextlib.contextmanager
def _norms_in_double():
    """The fp32 restatement measures the element-wise arithmetic; its two norms are not torch's fp32 accumulation over up to 525K
    squares (hundreds of ulps, and torch's own business) but the correctly rounded ones.  The kernels' folds are bounded by
    `fold_k`, derived, not measured."""
    norm = torch.Tensor.norm
    torch.Tensor.norm = lambda self, p=2: norm(self.double(), p=p).to(self.dtype)
    try:
        yield
    finally:
        torch.Tensor.norm = norm


# ---- one step ------------------------------------------------------------------------------------------------------------------------
def one_step(kind: str, pre: dict, hp: dict, dtype=torch.float64) -> dict:
    """`pre`: seg, p, g, state {key: tensor}, and optionally coef [nseg], skip [nseg], steps [nseg] (AdamW: the 1-based number of the
    update this step makes to each segment), lr_scale, wd_scale [nseg].  Returns p, g, state, diag {name: [nseg]} after the step, in
    `dtype`; a skipped segment keeps everything (its diagnostics are NaN here: the kernel must not write them, compare with what was there)."""
    seg = pre["seg"]
    nseg = len(seg) - 1
    p, g = pre["p"].to(dtype).clone(), pre["g"].to(dtype).clone()
    state = {k: v.to(dtype).clone() for k, v in pre["state"].items()}
    diag = {k: torch.full((nseg,), float("nan"), dtype=dtype) for k in DIAG} if kind == "Lamb" else {}
    lion_c = torch.zeros_like(p) if kind == "Lion" else None
    for s, (a, b) in enumerate(zip(seg, seg[1:])):
        if pre.get("skip") is not None and int(pre["skip"][s]):
            continue
        if pre.get("coef") is not None and float(pre["coef"][s]) != 1.0:
            g[a:b] *= float(pre["coef"][s])
        st = {k: v[a:b] for k, v in state.items()}
        step = int(pre["steps"][s]) if pre.get("steps") is not None else 1
        ls = float(pre["lr_scale"][s]) if pre.get("lr_scale") is not None else 1.0
        ws = float(pre["wd_scale"][s]) if pre.get("wd_scale") is not None else 1.0
        with _norms_in_double():
            out = PS.apply_scaled_(kind, p[a:b], g[a:b], st, hp["lr"], hp, step, ls, ws)
        if kind == "Lamb":
            for k, x in zip(DIAG, out):
                diag[k][s] = x
        if kind == "Lion":
            lion_c[a:b] = out
    return {"p": p, "g": g, "state": state, "diag": diag, "lion_c": lion_c}


def seg_lr(pre: dict, hp: dict, s: int) -> float:
    return hp["lr"] * (float(pre["lr_scale"][s]) if pre.get("lr_scale") is not None else 1.0)


# ---- bounds --------------------------------------------------------------------------------------------------------------------------
def scales(kind: str, pre: dict, ref: dict, hp: dict) -> Dict[str, torch.Tensor]:
    """S per element for the written-back gradient, every state buffer and the parameter; `ref` = one_step(..., float64).
      g            |g c|
      m, buffer    |m_old| + |g c|
      v            v_new + (1 - beta2) (g c)^2: the product g c is rounded before it is squared, so the g^2 term carries that rounding
                   twice (with S = v_new alone the fp32 restatement is 5.2 away, which times 4 passes 16)
      p            |p_old| + |update| + the update with S_m in the place of m.  The last term is what m's bar implies: the update is linear
                   in m, and where beta1 m_old and (1 - beta1) g cancel, k 2^-24 S_m is many ulps of m_new and comes through the
                   division unchanged (with S = |p_old| + |update| the fp32 restatement is thousands away on the zero-parameter
                   segment).  |update| carries the roundings of the update's own operations (the root, the denominator, the quotient,
                   the product); with the last term alone the fp32 restatement is 5.2 away on AdamW, which times 4 passes 16.
                   Lion's update is lr sign(c): S = |p_old| + |update| (a sign that may flip is excused, not bounded)."""
    seg = pre["seg"]
    gc = ref["g"].abs()
    p_old = pre["p"].double().abs()
    out = {"g": gc}
    for k in pre["state"]:
        out[k] = ref["state"][k] + (1.0 - hp["beta2"]) * gc * gc if k == "exp_avg_sq" else pre["state"][k].double().abs() + gc
    if kind == "Lion":
        out["p"] = p_old + (ref["p"] - pre["p"].double()).abs()
        return out
    sp = p_old + (ref["p"] - pre["p"].double()).abs()
    for s, (a, b) in enumerate(zip(seg, seg[1:])):
        if pre.get("skip") is not None and int(pre["skip"][s]):
            continue
        lr_s = seg_lr(pre, hp, s)
        wd_s = hp["weight_decay"] * (float(pre["wd_scale"][s]) if pre.get("wd_scale") is not None else 1.0)
        if kind == "AdamW":
            t = int(pre["steps"][s])
            den = ref["state"]["exp_avg_sq"][a:b].sqrt() / math.sqrt(1.0 - hp["beta2"] ** t) + hp["eps"]
            sp[a:b] += lr_s / (1.0 - hp["beta1"] ** t) * out["exp_avg"][a:b] / den
        elif kind == "SGD":
            sp[a:b] += lr_s * (out["momentum_buffer"][a:b] if "momentum_buffer" in out else gc[a:b])
        else:
            r = ref["diag"]["trust_ratio"][s]
            if not bool(torch.isnan(r)):  # a skipped segment has none
                den = ref["state"]["exp_avg_sq"][a:b].sqrt() + hp["eps"]
                sp[a:b] += lr_s * float(r) * (out["exp_avg"][a:b] / den + wd_s * p_old[a:b])
    out["p"] = sp
    return out


def err_units(got: torch.Tensor, ref: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """|got - ref| in units of 2^-24 * scale, per element; where the scale is 0 the value must be exact."""
    err = (got.double() - ref).abs()
    out = err / (U24 * scale)
    out = torch.where(scale == 0, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))), out)
    return out


def fold_k(units: int) -> float:
    """Roundings in the kernels' fixed-order L2 norm of a segment of `units` units, in units of 2^-24 of the norm.  Every addend is a
    square, so each addition of the chain adds at most 2^-24 of the running sum (first order).  The longest chain an element goes
    through: its square (1), the thread's float4 tree (2), the 64-lane butterfly (6), the four wave partials (2) -> the unit's sum;
    then the serial trips of the thread that owns the unit in the per-segment fold (ceil(units / 256) - 1 additions: the first lands
    on an exact 0), and the same block tree again (6 + 2).  The square root halves the relative error and rounds once."""
    trips = -(-units // 256)
    return (1 + 2 + 6 + 2 + (trips - 1) + 6 + 2) / 2 + 1


# k per quantity: 4 x the worst distance of the fp32 restatement (torch fp32, the reference's operation order) from fp64 over every
# case of `value_cases` / `scaled_cases` and the steps of `count_inputs`, floor 2.  The kernel regroups legitimately (it multiplies by 1/sqrt(bc2)
# where torch divides, rounds its constants once from double, forms AdamW's first moment as a lerp), hence the margin.  MEASURED is
# asserted by tests/test_optim_kernel_ref_cpu.py::test_fp32_restatement_within_measured (it prints the values), and no k may pass 16.
# "adam_norm" is the element-wise part of Lamb's ||u|| only: the fp32 restatement's norm against the fp64 one; the kernel's fold is
# bounded by fold_k on top of it, as are `norms` and weight_norm, which have no element-wise part.
MEASURED = {
    "AdamW": {"g": 1.00, "exp_avg": 1.76, "exp_avg_sq": 1.99, "p": 2.79},
    "Lion": {"g": 1.00, "exp_avg": 2.22, "p": 2.18},
    "SGD": {"g": 1.00, "momentum_buffer": 2.15, "p": 1.51},
    "Lamb": {"g": 1.00, "exp_avg": 2.16, "exp_avg_sq": 2.62, "p": 2.19, "adam_norm": 2.54},
}


def _k(x: float) -> float:
    return max(2.0, 4.0 * x)


K = {kind: {q: _k(x) for q, x in d.items()} for kind, d in MEASURED.items()}


def diag_k(units: int) -> Dict[str, float]:
    """Lamb's three per-segment values.  trust_ratio = w / (a + eps): both errors, the sum and the quotient."""
    w, a = fold_k(units), fold_k(units) + K["Lamb"]["adam_norm"]
    return {"weight_norm": w, "adam_norm": a, "trust_ratio": w + a + 2}


def p_k(kind: str, units: int) -> float:
    """The parameter's k: Lamb's step is scaled by the trust ratio, whose error is the folds'."""
    return K[kind]["p"] + (diag_k(units)["trust_ratio"] if kind == "Lamb" else 0.0)


def lion_excused(pre: dict, ref: dict, hp: dict) -> torch.Tensor:
    """optim_ref.lion_excused on the one step: the elements whose sign argument cancels to rounding."""
    return R.lion_excused(ref["lion_c"], pre["state"]["exp_avg"].double(), ref["g"], hp["beta1"])


def check(kind: str, pre: dict, got: dict, hp: dict, ref: Optional[dict] = None, bars: Optional[dict] = None,
          enforce: bool = True) -> Dict[str, float]:
    """Every per-element bar of one step; `got` = p, g, state, diag (and optionally shadow) in any float dtype.  Returns the worst
    distance per quantity in units of 2^-24 * S, after asserting each against its k (`enforce=False`: measure only).  Skipped segments are the caller's to compare
    bit for bit."""
    seg = pre["seg"]
    ref = ref or one_step(kind, pre, hp)
    sc = scales(kind, pre, ref, hp)
    bars = bars or K[kind]
    live = [s for s in range(len(seg) - 1) if not (pre.get("skip") is not None and int(pre["skip"][s]))]
    excused = lion_excused(pre, ref, hp) if kind == "Lion" else None
    worst = {}

    def bar(q, s, units_err, k):
        w = float(units_err.max()) if units_err.numel() else 0.0
        worst[q] = max(worst.get(q, 0.0), w)
        assert not enforce or w <= k, f"{kind} {q} segment {s}: {w:.2f} x 2^-24 x S > k = {k}"

    for s in live:
        a, b = seg[s], seg[s + 1]
        units = (b - a) // UNIT
        bar("g", s, err_units(got["g"][a:b], ref["g"][a:b], sc["g"][a:b]), bars["g"])
        for k in pre["state"]:
            bar(k, s, err_units(got["state"][k][a:b], ref["state"][k][a:b], sc[k][a:b]), bars[k])
        e = err_units(got["p"][a:b], ref["p"][a:b], sc["p"][a:b])
        pk = bars["p"] + (diag_k(units)["trust_ratio"] if kind == "Lamb" else 0.0)
        if kind == "Lion":
            ex = excused[a:b]
            share = float(ex.double().mean())
            worst["excused"] = max(worst.get("excused", 0.0), share)
            assert share <= LION_CAP, f"Lion segment {s}: {share:.2e} of the elements excused"
            # an excused element may have stepped the other way: off by 2 * lr_s, within the same bar
            two = 2.0 * seg_lr(pre, hp, s)
            d = (got["p"][a:b].double() - ref["p"][a:b]).abs()[ex]
            off = torch.minimum(d, (d - two).abs()) / (U24 * sc["p"][a:b][ex])
            bar("p", s, off, pk)
            e = e[~ex]
        bar("p", s, e, pk)
        if kind == "Lamb":
            for q, k in diag_k(units).items():
                r = ref["diag"][q][s]
                bar(q, s, err_units(got["diag"][q][s:s + 1], r.reshape(1), r.abs().reshape(1)), k)
    return worst


def check_norms(g: torch.Tensor, seg: List[int], clip: float, norms: torch.Tensor, coef: torch.Tensor, enforce: bool = True) -> float:
    """hct_grad_norms' two outputs against fp64 on finite gradients: norms within fold_k of the value; coef = clip / (norm + 1e-6)
    within fold_k + 2 (the sum and the quotient) where that is below 1 by more than the bound, exactly 1 where it is above 1 by more
    than the bound (in between either is right: the cases stay clear of it, the threshold has a test of its own), all ones at
    clip = 0, and norm 0 -> exactly (0, 1).  Returns the worst norm distance in units of 2^-24 of the norm."""
    want = seg_norms(g.double(), seg)
    worst = 0.0
    for s, (a, b) in enumerate(zip(seg, seg[1:])):
        k = fold_k((b - a) // UNIT)
        n, c, w = float(norms[s]), float(coef[s]), float(want[s])
        if w == 0.0:
            assert n == 0.0 and c == 1.0, (s, n, c)
            continue
        d = abs(n - w) / (U24 * w)
        worst = max(worst, d)
        assert not enforce or d <= k, f"norm of segment {s}: {d:.2f} x 2^-24 x norm > k = {k}"
        cw = clip / (w + 1e-6) if clip > 0 else 2.0
        tol = (k + 2) * U24 * cw
        if cw - tol > 1.0:
            assert not enforce or c == 1.0, (s, c, cw)
        elif cw + tol < 1.0:
            assert not enforce or abs(c - cw) <= tol, (s, c, cw)
    return worst


def check_shadow(p: torch.Tensor, shadow: torch.Tensor, shadow_before: torch.Tensor, pre: dict) -> None:
    """The bf16 shadow is the updated parameter ROUNDED to bf16 on every live segment and untouched on a skipped one, bit for bit."""
    seg = pre["seg"]
    for s, (a, b) in enumerate(zip(seg, seg[1:])):
        skipped = pre.get("skip") is not None and int(pre["skip"][s])
        want = shadow_before[a:b] if skipped else p[a:b].to(torch.bfloat16)
        assert torch.equal(shadow[a:b].view(torch.int16), want.view(torch.int16)), f"shadow of segment {s} (skipped: {bool(skipped)})"


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
class Case(NamedTuple):
    name: str
    kind: str
    layout: str
    hp: dict           # lr, weight_decay, beta1, beta2, momentum, eps as the caller writes them
    step: int = 1      # AdamW: the count every live segment is at
    seeded: bool = False
    scaled: bool = False


def _rng(name: str) -> np.random.Generator:
    return np.random.default_rng(zlib.crc32(name.encode()))


def hot_units(units: int) -> List[int]:
    """Within a segment longer than one trip: the first unit of the second and third trips and the last unit."""
    return sorted({u for u in (256, 512, units - 1) if 0 < u < units}) if units > 256 else []


def inputs(case: Case) -> dict:
    """fp32 CPU tensors of one case.  Gradients log-uniform in magnitude over 1e-12 .. 1e3 with random signs, times a power of two
    per segment; parameters uniform(-1, 1) times a per-segment scale (segment 0: 0.1, so that ||p|| < 10; segment 2: zero); one
    zero-gradient segment; a deferred clip coefficient, a skip bit and (scaled cases) an lr / wd scale that differ between
    neighbouring segments.  In the 257- and 513-unit segments the units of `hot_units` keep their magnitude and the rest are scaled
    down by 2^-10 (g), 2^-8 (p) and, in the seeded state, given a huge second moment: the folds' energy sits in the hot units."""
    units = LAYOUTS[case.layout]
    seg = offsets(units)
    nseg, total = len(units), seg[-1]
    rng = _rng(case.name)
    g = rng.choice([-1.0, 1.0], total) * 10.0 ** rng.uniform(-12.0, 3.0, total)
    p = rng.uniform(-1.0, 1.0, total)
    m = rng.uniform(-1.0, 1.0, total) * 10.0 ** rng.uniform(-6.0, 1.0, total)
    v = 10.0 ** rng.uniform(-12.0, 2.0, total)
    v[rng.uniform(size=total) < 0.01] = 0.0
    coef = np.ones(nseg, dtype=np.float32)
    skip = np.zeros(nseg, dtype=np.uint8)
    zero_g = nseg - 1 if nseg > 2 else -1
    for s, (a, b) in enumerate(zip(seg, seg[1:])):
        g[a:b] *= 2.0 ** ((5 * s) % 9 - 4)
        p[a:b] *= (0.1, 1.0, 0.0, 1.0, 0.5)[s % 5] if nseg > 1 else 1.0
        p[a:b] += 0.0  # the zero-parameter segment holds +0: at lr 0 a -0 may leave as +0, which is no error of the step
        if s % 3:
            coef[s] = np.float32(rng.uniform(0.05, 0.95))
        if nseg > 2 and s % 7 == 5:
            skip[s] = 1
        hot = hot_units(units[s])
        if hot:
            cold = np.ones(units[s], dtype=bool)
            cold[hot] = False
            cold = np.repeat(cold, UNIT)
            g[a:b][cold] *= 2.0 ** -10
            p[a:b][cold] *= 2.0 ** -8
            m[a:b][cold] *= 1e-3
            v[a:b][cold] += 1e10
        if s == zero_g:
            g[a:b] = 0.0
    t = lambda x: torch.from_numpy(np.asarray(x, dtype=np.float32).copy())
    keys = () if (case.kind == "SGD" and case.hp["momentum"] == 0) else STATE_KEYS[case.kind]
    seeds = {"exp_avg": m, "momentum_buffer": m, "exp_avg_sq": v}
    state = {k: (t(seeds[k]) if case.seeded else torch.zeros(total)) for k in keys}
    pre = {"seg": seg, "units": units, "p": t(p), "g": t(g), "state": state, "coef": t(coef), "skip": torch.from_numpy(skip),
           "steps": torch.full((nseg,), case.step, dtype=torch.int32), "zero_g": zero_g}
    if case.scaled:
        pre["lr_scale"] = t([(0.0, 0.5, 1.0, 2.0)[s % 4] for s in range(nseg)])
        pre["wd_scale"] = t([(0.0, 1.0, 3.0)[s % 3] for s in range(nseg)])
    return pre


_BASE = dict(lr=1e-3, weight_decay=0.05, beta1=0.9, beta2=0.999, momentum=0.9, eps=1e-8)


def value_cases(kind: str) -> List[Case]:
    """The regimes of each optimizer: the full product on the 131-segment layout (131K elements), and the two seeded extremes on the
    layout with the long segments (1M elements)."""
    out = []
    if kind == "AdamW":
        for b1, b2 in ((0.9, 0.999), (0.9, 0.95)):
            for step in (1, 2, 1000, 100000):
                for wd in (0.0, 0.05):
                    hp = dict(_BASE, beta1=b1, beta2=b2, weight_decay=wd)
                    out.append(Case(f"adamw-b2{b2}-t{step}-wd{wd}", kind, "many", hp, step, seeded=step > 1))
        out.append(Case("adamw-lr0", kind, "many", dict(_BASE, lr=0.0), 3, seeded=True))
        out.append(Case("adamw-one", kind, "one", dict(_BASE), 1))
        out.append(Case("adamw-trips", kind, "trips", dict(_BASE), 1000, seeded=True))
    elif kind == "Lion":
        for b1, b2 in ((0.9, 0.99), (0.95, 0.98)):
            for wd in (0.0, 0.1):
                for seeded in (False, True):
                    out.append(Case(f"lion-b1{b1}-wd{wd}-s{int(seeded)}", kind, "many", dict(_BASE, lr=1e-4, beta1=b1, beta2=b2, weight_decay=wd), seeded=seeded))
        out.append(Case("lion-lr0", kind, "many", dict(_BASE, lr=0.0, beta2=0.99), seeded=True))
        out.append(Case("lion-one", kind, "one", dict(_BASE, lr=1e-4, beta2=0.99)))
        out.append(Case("lion-trips", kind, "trips", dict(_BASE, lr=1e-4, beta2=0.99), seeded=True))
    elif kind == "SGD":
        for mom in (0.0, 0.9):
            for seeded in (False, True):
                out.append(Case(f"sgd-m{mom}-s{int(seeded)}", kind, "many", dict(_BASE, lr=1e-2, momentum=mom), seeded=seeded))
            out.append(Case(f"sgd-m{mom}-lr0", kind, "many", dict(_BASE, lr=0.0, momentum=mom), seeded=True))
        out.append(Case("sgd-one", kind, "one", dict(_BASE, lr=1e-2)))
        out.append(Case("sgd-trips", kind, "trips", dict(_BASE, lr=1e-2), seeded=True))
    elif kind == "Lamb":
        for wd in (0.0, 0.01):
            for seeded in (False, True):
                hp = dict(_BASE, eps=1e-6, weight_decay=wd)
                out.append(Case(f"lamb-wd{wd}-s{int(seeded)}-many", kind, "many", hp, seeded=seeded))
                out.append(Case(f"lamb-wd{wd}-s{int(seeded)}-trips", kind, "trips", hp, seeded=seeded))
        out.append(Case("lamb-lr0", kind, "trips", dict(_BASE, lr=0.0, eps=1e-6, weight_decay=0.01), seeded=True))
        out.append(Case("lamb-one", kind, "one", dict(_BASE, eps=1e-6, weight_decay=0.01)))
    return out


def scaled_cases(kind: str) -> List[Case]:
    """The `_scaled` entry points over the 131 segments: lr scales {0, 0.5, 1, 2} and wd scales {0, 1, 3} by segment index."""
    hp = {"AdamW": dict(_BASE), "Lion": dict(_BASE, lr=1e-4, beta2=0.99), "SGD": dict(_BASE, lr=1e-2),
          "Lamb": dict(_BASE, eps=1e-6, weight_decay=0.01)}[kind]
    return [Case(f"{kind.lower()}-scaled-s{int(seeded)}", kind, "many", hp, step=7, seeded=seeded, scaled=True) for seeded in (False, True)]


def all_cases(kind: str) -> List[Case]:
    return value_cases(kind) + scaled_cases(kind)


# ---- AdamW's count per segment (case F) ----------------------------------------------------------------------------------------------
COUNT_UNITS = [2, 1, 1]           # live throughout | no gradient for the first 5 of 8 steps | skipped throughout
COUNT_STEPS, COUNT_LATE = 8, 5


def count_schedule(step: int) -> List[bool]:
    """live[s] at 0-based step `step`."""
    return [True, step >= COUNT_LATE, False]


def count_inputs(betas) -> dict:
    seg = offsets(COUNT_UNITS)
    rng = _rng(f"count-{betas}")
    p = torch.from_numpy(rng.uniform(-1.0, 1.0, seg[-1]).astype(np.float32))
    grads = [torch.from_numpy((rng.choice([-1.0, 1.0], seg[-1]) * 10.0 ** rng.uniform(-6.0, 1.0, seg[-1])).astype(np.float32))
             for _ in range(COUNT_STEPS)]
    return {"seg": seg, "p": p, "grads": grads, "hp": dict(_BASE, beta1=betas[0], beta2=betas[1])}


def torch_adamw_run(ci: dict, dtype=torch.float64) -> List[List[torch.Tensor]]:
    """torch.optim.AdamW (foreach=False) over the three tensors, given the gradients of the schedule (None where not live) and
    the hyper-parameters as the C ABI holds them.  Returns the parameters after every step."""
    seg, hp = ci["seg"], abi_hp("AdamW", ci["hp"])
    ps = [torch.nn.Parameter(ci["p"][a:b].to(dtype).clone()) for a, b in zip(seg, seg[1:])]
    opt = torch.optim.AdamW(ps, lr=hp["lr"], betas=(hp["beta1"], hp["beta2"]), eps=hp["eps"], weight_decay=hp["weight_decay"], foreach=False)
    hist = []
    for step in range(COUNT_STEPS):
        for s, (q, (a, b)) in enumerate(zip(ps, zip(seg, seg[1:]))):
            q.grad = ci["grads"][step][a:b].to(dtype).clone() if count_schedule(step)[s] else None
        opt.step()
        hist.append([q.detach().clone() for q in ps])
    return hist, opt
