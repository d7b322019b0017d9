"""GPU: the optimizer kernels of csrc/optim.hip one by one through the C ABI, per element against tests/optim_kernel_ref.py (fp64, one
step deep: the kernel's own pre-step p, g, m, v go into the yardstick, so nothing accumulates), and AdamW's step count per segment
at kernel and at class level against torch.optim.AdamW.  Bars: k * 2^-24 * S per element, k and S from optim_kernel_ref (whose CPU
tests show that the bars pass the fp32 restatement and fail a dozen wrong ones); folds by the derived chain length.

Every device buffer a kernel may write (p, g, the state, the bf16 shadow, both workspaces, norms / coef / Lamb's diagnostics) sits
between two guard units of NaN, and after every call the guards must have kept their bits: a stray write is a failed assertion."""
import copy

import numpy as np
import pytest
import torch

from headct_foundation_amd import _lib
from tests import optim_kernel_ref as KR
from tests.util import rel_err

pytestmark = pytest.mark.gpu
G = KR.UNIT
CLIP_MANY = 4000.0  # between the norms of the 131 segments (240 .. 61000): about half are clipped


def _st():
    return torch.cuda.current_stream().cuda_stream


class Guarded:
    """`src` on the device between two guard units of NaN."""

    def __init__(self, src, dev, dtype=None):
        src = torch.as_tensor(src)
        dtype = dtype or src.dtype
        n = src.numel()
        self.full = torch.full((n + 2 * G,), float("nan"), dtype=dtype, device=dev)
        self.t = self.full[G:G + n]
        self.t.copy_(src.to(dtype))
        self._bits = self._guards()

    def _guards(self):
        v = self.full.view(torch.int16 if self.full.element_size() == 2 else torch.int32)
        return torch.cat([v[:G], v[-G:]]).clone()

    def intact(self):
        return torch.equal(self._guards(), self._bits)

    def ptr(self):
        return self.t.data_ptr()

    def cpu(self):
        return self.t.detach().cpu().clone()


class Problem:
    """One flat problem of optim_kernel_ref.inputs on the device, driven through the C ABI."""

    def __init__(self, lib, dev, kind, pre, hp):
        self.lib, self.dev, self.kind, self.hp = lib, dev, kind, hp
        seg = self.seg = pre["seg"]
        self.nseg, self.total = len(seg) - 1, seg[-1]
        n, t = self.nseg, self.total
        self.p, self.g = Guarded(pre["p"], dev), Guarded(pre["g"], dev)
        self.state = {k: Guarded(v, dev) for k, v in pre["state"].items()}
        self.shadow = Guarded(torch.full((t,), 7.0), dev, torch.bfloat16)  # 7: no parameter here comes near it
        self.diag = {k: Guarded(torch.full((n,), -7.0), dev) for k in KR.DIAG}
        self.norms = Guarded(torch.full((n,), -7.0), dev)
        self.coef = Guarded(pre["coef"] if pre.get("coef") is not None else torch.ones(n), dev)
        self.ws_bytes, self.lws_bytes = lib.hct_grad_norms_workspace_bytes(t), lib.hct_lamb_workspace_bytes(t, n)
        self.ws = Guarded(torch.full((self.ws_bytes // 4,), float("nan")), dev)
        self.lws = Guarded(torch.full((self.lws_bytes // 4,), float("nan")), dev)
        self.seg_t = torch.tensor(seg, dtype=torch.int64, device=dev)
        self.skip_t = torch.as_tensor(pre["skip"] if pre.get("skip") is not None else [0] * n, dtype=torch.uint8).to(dev)
        self.steps = [int(x) for x in pre["steps"]] if pre.get("steps") is not None else [1] * n
        self.steps_t = torch.tensor(self.steps, dtype=torch.int32, device=dev)
        self.lr_scale = pre["lr_scale"].to(dev) if pre.get("lr_scale") is not None else None
        self.wd_scale = pre["wd_scale"].to(dev) if pre.get("wd_scale") is not None else None

    def buffers(self):
        return [self.p, self.g, self.shadow, self.norms, self.coef, self.ws, self.lws] + list(self.state.values()) + list(self.diag.values())

    def assert_guards(self):
        torch.cuda.synchronize()
        assert all(b.intact() for b in self.buffers()), "a guard unit was written"

    def set(self, g=None, skip=None, steps=None):
        if g is not None:
            self.g.t.copy_(g)
        if skip is not None:
            self.skip_t.copy_(torch.as_tensor(skip, dtype=torch.uint8))
        if steps is not None:
            self.steps = [int(x) for x in steps]
            self.steps_t.copy_(torch.tensor(self.steps, dtype=torch.int32))

    def grad_norms(self, clip, in_place):
        _lib.check(self.lib.hct_grad_norms(self.g.ptr(), self.seg_t.data_ptr(), self.nseg, self.total, float(clip), int(in_place), self.norms.ptr(),
                                           self.coef.ptr(), self.ws.ptr(), self.ws_bytes, _st()), "hct_grad_norms")

    def step(self, entry=None, coef=True, skip=True, shadow=True):
        """entry: None = the plain entry point (`_scaled` when the problem has scales), "counts" = hct_adamw_step_counts."""
        lib, hp, k = self.lib, self.hp, self.kind
        common = (self.seg_t.data_ptr(), self.coef.ptr() if coef else None, self.skip_t.data_ptr() if skip else None, self.nseg, self.total)
        sh = self.shadow.ptr() if shadow else None
        ls, ws = _lib.ptr(self.lr_scale), _lib.ptr(self.wd_scale)
        scaled = self.lr_scale is not None or self.wd_scale is not None
        S = lambda name: self.state[name].ptr()
        if k == "AdamW":
            head = (self.p.ptr(), self.g.ptr(), S("exp_avg"), S("exp_avg_sq"), *common, hp["lr"], hp["beta1"], hp["beta2"], hp["eps"], hp["weight_decay"])
            if entry == "counts":
                rc = lib.hct_adamw_step_counts(*head, self.steps_t.data_ptr(), sh, ls, ws, _st())
            else:
                live = {t for t, s in zip(self.steps, self.skip_t.tolist()) if not (skip and s)}
                assert len(live) == 1, "one count for all live segments, or the counts entry point"
                rc = lib.hct_adamw_step_scaled(*head, live.pop(), sh, ls, ws, _st()) if scaled else lib.hct_adamw_step(*head, live.pop(), sh, _st())
        elif k == "Lion":
            args = (self.p.ptr(), self.g.ptr(), S("exp_avg"), *common, hp["lr"], hp["beta1"], hp["beta2"], hp["weight_decay"], sh)
            rc = lib.hct_lion_step_scaled(*args, ls, ws, _st()) if scaled else lib.hct_lion_step(*args, _st())
        elif k == "SGD":
            buf = S("momentum_buffer") if self.state else None
            args = (self.p.ptr(), self.g.ptr(), buf, *common, hp["lr"], hp["momentum"], sh)
            rc = lib.hct_sgd_step_scaled(*args, ls, _st()) if scaled else lib.hct_sgd_step(*args, _st())
        else:
            d = self.diag
            args = (self.p.ptr(), self.g.ptr(), S("exp_avg"), S("exp_avg_sq"), *common, hp["lr"], hp["beta1"], hp["beta2"], hp["eps"], hp["weight_decay"],
                    d["weight_norm"].ptr(), d["adam_norm"].ptr(), d["trust_ratio"].ptr(), self.lws.ptr(), self.lws_bytes, sh)
            rc = lib.hct_lamb_step_scaled(*args, ls, ws, _st()) if scaled else lib.hct_lamb_step(*args, _st())
        _lib.check(rc, k)

    def got(self):
        return {"p": self.p.cpu(), "g": self.g.cpu(), "state": {k: v.cpu() for k, v in self.state.items()},
                "diag": {k: v.cpu() for k, v in self.diag.items()}, "shadow": self.shadow.cpu()}


def _bits(a, b):
    return a.dtype == b.dtype and torch.equal(a.view(torch.int16 if a.element_size() == 2 else torch.int32), b.view(torch.int16 if b.element_size() == 2 else torch.int32))


def _assert_skipped_kept(pre, before, got):
    """A skipped segment keeps every bit: parameter, gradient, state, shadow, Lamb's diagnostics."""
    seg = pre["seg"]
    for s, (a, b) in enumerate(zip(seg, seg[1:])):
        if pre.get("skip") is None or not int(pre["skip"][s]):
            continue
        for q in ("p", "g", "shadow"):
            assert _bits(got[q][a:b], before[q][a:b]), (s, q)
        for k in got["state"]:
            assert _bits(got["state"][k][a:b], before["state"][k][a:b]), (s, k)
        for k in got["diag"]:
            assert _bits(got["diag"][k][s:s + 1], before["diag"][k][s:s + 1]), (s, k)


def _assert_unclipped_gradient_kept(pre, got):
    seg = pre["seg"]
    for s, (a, b) in enumerate(zip(seg, seg[1:])):
        if pre.get("coef") is None or float(pre["coef"][s]) == 1.0:
            assert _bits(got["g"][a:b], pre["g"][a:b]), s


def _one_step_checked(pb, pre, hp_abi, entry=None, **kw):
    """Run one step of `pb`, whose pre-step content is `pre`, and hold it to every bar; returns the worst distances."""
    before = pb.got()
    pb.step(entry, **kw)
    pb.assert_guards()
    got = pb.got()
    worst = KR.check(pb.kind, pre, got, hp_abi)
    _assert_skipped_kept(pre, before, got)
    _assert_unclipped_gradient_kept(pre, got)
    KR.check_shadow(got["p"], got["shadow"], before["shadow"], pre)
    return got, worst


# ---- C. value regimes, the three layouts, the scaled entry points ----------------------------------------------------------------------
def _case_params():
    out = []
    for kind in KR.KINDS:
        for c in KR.all_cases(kind):
            out.append(pytest.param(kind, c, None, id=c.name))
            if kind == "AdamW":  # the same problem through the per-segment-count entry point, every count equal
                out.append(pytest.param(kind, c, "counts", id=c.name + "-counts"))
    return out


@pytest.mark.parametrize("kind,case,entry", _case_params())
def test_one_step_per_element(lib, cuda, kind, case, entry):
    """Every regime of optim_kernel_ref.value_cases / scaled_cases: gradients log-uniform over 1e-12 .. 1e3, seeded and zero moments,
    131 one-unit segments that each have their own gradient scale, clip coefficient, skip bit (and lr / wd scale), the layout with
    257- and 513-unit segments, lr 0, large steps, both beta pairs.  Per element within k * 2^-24 * S; skipped segments and unclipped
    gradients keep their bits; the shadow is the rounded parameter; at lr 0 the parameter keeps its bits while the moments move."""
    pre = KR.inputs(case)
    pb = Problem(lib, cuda, kind, pre, case.hp)
    got, worst = _one_step_checked(pb, pre, KR.abi_hp(kind, case.hp), entry)
    print(case.name, entry or "", {q: round(x, 3) for q, x in worst.items()})
    if case.hp["lr"] == 0:
        seg = pre["seg"]
        for s, (a, b) in enumerate(zip(seg, seg[1:])):
            if int(pre["skip"][s]):
                continue
            assert _bits(got["p"][a:b], pre["p"][a:b]), s
            assert _bits(got["shadow"][a:b], pre["p"][a:b].to(torch.bfloat16)), s
            if s != pre["zero_g"]:
                assert all(not torch.equal(got["state"][k][a:b], pre["state"][k][a:b]) for k in got["state"]), s


def test_adamw_counts_entry_agrees_with_the_uniform_launch(lib, cuda):
    """With one count for every segment hct_adamw_step_counts computes what hct_adamw_step[_scaled] does: the same constants formed in
    double on the device instead of on the host, so the same bits wherever pow() agrees to the last place of a double, and never more
    than one unit of the step's last place apart."""
    for name in ("adamw-b20.999-t1000-wd0.05", "adamw-scaled-s1"):
        case = next(c for c in KR.all_cases("AdamW") if c.name == name)
        pre = KR.inputs(case)
        a, b = Problem(lib, cuda, "AdamW", pre, case.hp), Problem(lib, cuda, "AdamW", pre, case.hp)
        a.step()
        b.step("counts")
        ga, gb = a.got(), b.got()
        assert _bits(ga["g"], gb["g"]) and all(_bits(ga["state"][k], gb["state"][k]) for k in ga["state"])
        d = (ga["p"].double() - gb["p"].double()).abs()
        upd = (ga["p"].double() - pre["p"].double()).abs()
        assert float((d - 2.0 ** -23 * (upd + pre["p"].double().abs())).max()) <= 0, name


# ---- exact cases -------------------------------------------------------------------------------------------------------------------------
def _exact_pre(kind, rng):
    seg = KR.offsets(KR.LAYOUTS["few"])
    ints = lambda lo, hi: torch.from_numpy(rng.integers(lo, hi + 1, seg[-1]).astype(np.float32))
    p = ints(-8, 8) if kind == "SGD" else ints(-2048, 2048) / 1024.0
    key = "momentum_buffer" if kind == "SGD" else "exp_avg"
    return {"seg": seg, "p": p, "g": ints(-16, 16), "state": {key: ints(-16, 16)}}


@pytest.mark.parametrize("kind", ["SGD", "Lion"])
def test_exact_integer_steps(lib, cuda, kind):
    """SGD with integer p, g, lr 0.5 and momentum 0.5; Lion with wd 0, lr 2^-10, betas 0.5 / 0.5 and integer m, g: every product and
    sum of three steps is exact in fp32, so the kernel equals the fp64 restatement bit for bit."""
    rng = np.random.default_rng(11)
    hp = dict(lr=0.5, momentum=0.5, weight_decay=0.0) if kind == "SGD" else dict(lr=2.0 ** -10, beta1=0.5, beta2=0.5, weight_decay=0.0)
    pre = _exact_pre(kind, rng)
    pb = Problem(lib, cuda, kind, pre, hp)
    for step in range(3):
        ref = KR.one_step(kind, pre, hp)
        pb.step()
        pb.assert_guards()
        got = pb.got()
        assert torch.equal(got["p"].double(), ref["p"]), step
        for k in got["state"]:
            assert torch.equal(got["state"][k].double(), ref["state"][k]), (step, k)
        assert torch.equal(got["shadow"], got["p"].to(torch.bfloat16))
        g = _exact_pre(kind, rng)["g"]
        pb.set(g=g)
        pre = {"seg": pre["seg"], "p": got["p"], "g": g, "state": got["state"]}
    assert not torch.equal(got["p"], _exact_pre(kind, np.random.default_rng(11))["p"])


# ---- B. hct_grad_norms -------------------------------------------------------------------------------------------------------------------
def _norms_call(lib, dev, g, seg, clip, in_place):
    pre = {"seg": seg, "p": torch.zeros(seg[-1]), "g": g, "state": {}}
    pb = Problem(lib, dev, "SGD", pre, {})
    pb.grad_norms(clip, in_place)
    pb.assert_guards()
    return pb.norms.cpu(), pb.coef.cpu(), pb.g.cpu()


@pytest.mark.parametrize("layout,clip", [("one", 1000.0), ("many", CLIP_MANY), ("trips", 3.0), ("trips", 1e9)])
def test_grad_norms_and_coefficients(lib, cuda, layout, clip):
    """`norms` and `coef` per segment against fp64, the fold's k from the length of its chain (a fold that drops the last unit or a
    later trip of the 257- / 513-unit segments is off by a large factor: their energy sits there); a zero gradient gives exactly
    (0, 1); the deferred route leaves the gradient alone; scale_in_place writes exactly g * coef, one product."""
    case = next(c for c in KR.all_cases("AdamW") if c.layout == layout)
    pre = KR.inputs(case)
    seg, g = pre["seg"], pre["g"]
    norms, coef, g0 = _norms_call(lib, cuda, g, seg, clip, 0)
    worst = KR.check_norms(g, seg, clip, norms, coef)
    print(layout, clip, "worst norm distance", round(worst, 3), "x 2^-24; clipped", int((coef < 1).sum()), "of", len(coef))
    assert _bits(g0, g)
    if pre["zero_g"] >= 0:
        assert float(norms[pre["zero_g"]]) == 0.0 and float(coef[pre["zero_g"]]) == 1.0
    if layout == "many":
        assert 30 < int((coef < 1).sum()) < 100
    norms1, coef1, g1 = _norms_call(lib, cuda, g, seg, clip, 1)
    assert _bits(norms1, norms) and _bits(coef1, coef)
    assert _bits(g1, KR.scaled_grad(g, seg, coef))


@pytest.mark.parametrize("in_place", [0, 1])
def test_grad_norms_without_clip(lib, cuda, in_place):
    """clip = 0 (the route clip_grad_norm_ takes): norms as ever, every coefficient exactly 1, the gradient bits untouched."""
    pre = KR.inputs(next(c for c in KR.all_cases("AdamW") if c.layout == "many"))
    norms, coef, g = _norms_call(lib, cuda, pre["g"], pre["seg"], 0.0, in_place)
    KR.check_norms(pre["g"], pre["seg"], 0.0, norms, coef)
    assert bool((coef == 1.0).all()) and _bits(g, pre["g"])


def test_grad_norms_on_either_side_of_the_threshold(lib, cuda):
    """Two segments whose fp32 norms are exact: 1024 x 2^-5 (norm 1), and the same plus 2^-5 and 2^-11 in a second unit (sum of
    squares 1 + 2^-10 + 2^-22 = (1 + 2^-11)^2).  With clip = 1 + 2^-12 the first lies under clip - 1e-6 (coef exactly 1, gradient
    untouched), the second over it (scaled by clip / (norm + 1e-6) in fp32)."""
    seg = KR.offsets([1, 2])
    g = torch.zeros(seg[-1])
    g[:1024] = 2.0 ** -5
    g[1024:2048] = 2.0 ** -5
    g[2048], g[3071] = 2.0 ** -5, 2.0 ** -11
    clip = 1.0 + 2.0 ** -12
    norms, coef, g1 = _norms_call(lib, cuda, g, seg, clip, 1)
    assert float(norms[0]) == 1.0 and float(norms[1]) == 1.0 + 2.0 ** -11
    c = torch.tensor(clip, dtype=torch.float32) / (norms[1] + torch.tensor(1e-6, dtype=torch.float32))
    assert float(coef[0]) == 1.0 and float(coef[1]) == float(c) < 1.0
    assert _bits(g1[:1024], g[:1024]) and _bits(g1[1024:], g[1024:] * c)


@pytest.mark.parametrize("poison", [float("inf"), float("nan")])
def test_a_non_finite_gradient_stays_in_its_segment(lib, cuda, poison):
    """One inf (or NaN) in segment 64 of 131.  Its own norm, coefficient and gradient are the restatement's, NaN positions included
    (an infinite norm scales by 0: the inf becomes NaN, the rest 0; a NaN norm compares false and is left unclipped); every other
    segment's outputs are the bits of the run without the poison."""
    pre = KR.inputs(next(c for c in KR.all_cases("AdamW") if c.layout == "many"))
    seg, g = pre["seg"], pre["g"]
    bad = g.clone()
    a, b = seg[64], seg[65]
    bad[a + 100] = poison
    clean = _norms_call(lib, cuda, g, seg, CLIP_MANY, 1)
    norms, coef, g1 = _norms_call(lib, cuda, bad, seg, CLIP_MANY, 1)
    other = torch.ones(len(seg) - 1, dtype=torch.bool)
    other[64] = False
    assert _bits(norms[other], clean[0][other]) and _bits(coef[other], clean[1][other])
    assert _bits(g1[:a], clean[2][:a]) and _bits(g1[b:], clean[2][b:])
    want_n = KR.seg_norms(bad.double(), seg)
    want_c = KR.clip_coef(want_n, CLIP_MANY)
    want_g = KR.scaled_grad(bad.double(), seg, want_c)[a:b]
    if poison != poison:
        assert norms[64] != norms[64] and float(coef[64]) == 1.0 and _bits(g1[a:b], bad[a:b])
    else:
        assert float(norms[64]) == float("inf") and float(coef[64]) == 0.0
    assert torch.equal(torch.isnan(g1[a:b]), torch.isnan(want_g)) and int(torch.isnan(want_g).sum()) == 1
    keep = ~torch.isnan(want_g)
    assert torch.equal(g1[a:b][keep].double(), want_g[keep])


def _seeded(kind, layout):
    return next(c for c in KR.value_cases(kind) if c.seeded and c.layout == layout and c.hp["lr"] > 0)


@pytest.mark.parametrize("layout", ["many", "trips"])
@pytest.mark.parametrize("kind", KR.KINDS)
def test_in_place_scaling_equals_the_deferred_write_back(lib, cuda, kind, layout):
    """scale_in_place = 1 leaves, bit for bit, the gradient each optimizer kernel writes back when the coefficient is deferred to it:
    one product g * c either way."""
    case = _seeded(kind, layout)
    pre = KR.inputs(case)
    pre["skip"] = torch.zeros_like(pre["skip"])
    clip = CLIP_MANY if layout == "many" else 3000.0
    _, coef, g1 = _norms_call(lib, cuda, pre["g"], pre["seg"], clip, 1)
    pb = Problem(lib, cuda, kind, pre, case.hp)
    pb.grad_norms(clip, 0)
    pb.step()
    pb.assert_guards()
    assert _bits(pb.coef.cpu(), coef) and 0 < int((coef < 1).sum()) < len(coef)
    assert _bits(pb.g.cpu(), g1)


# ---- D. null forms -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,entry", [(k, None) for k in KR.KINDS] + [("AdamW", "counts")])
def test_null_pointer_forms(lib, cuda, kind, entry):
    """coef = NULL is a coefficient array of ones, skip = NULL a mask of zeros, params_bf16 = NULL changes nothing else: same bits."""
    case = _seeded(kind, "many")
    pre = KR.inputs(case)
    n = len(pre["seg"]) - 1
    runs = {}
    for name, kw in (("arrays", {}), ("no_coef", dict(coef=False)), ("no_skip", dict(skip=False)), ("no_shadow", dict(shadow=False))):
        pb = Problem(lib, cuda, kind, dict(pre, coef=torch.ones(n), skip=torch.zeros(n, dtype=torch.uint8)), case.hp)
        pb.step(entry, **kw)
        pb.assert_guards()
        runs[name] = pb.got()
    base = runs["arrays"]
    assert not _bits(base["p"], pre["p"])
    for name in ("no_coef", "no_skip", "no_shadow"):
        r = runs[name]
        assert _bits(r["p"], base["p"]) and _bits(r["g"], base["g"]) and all(_bits(r["state"][k], base["state"][k]) for k in base["state"]), name
        assert all(_bits(r["diag"][k], base["diag"][k]) for k in base["diag"]), name
        if name != "no_shadow":
            assert _bits(r["shadow"], base["shadow"]), name
    assert bool((runs["no_shadow"]["shadow"] == 7.0).all()) and _bits(base["shadow"], base["p"].to(torch.bfloat16))


# ---- E. skip sequences ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KR.KINDS)
def test_skip_sequence(lib, cuda, kind):
    """Six steps; the 2-unit middle segment is live, skipped, skipped, live, skipped, live.  Skipped: parameter, moments, shadow,
    diagnostics and gradient keep their bits.  Live: the yardstick's bars (AdamW with the segment's own count: 1, 2, 3)."""
    hp0 = next(c.hp for c in KR.value_cases(kind) if c.hp["lr"] > 0 and c.hp["weight_decay"] > 0 and c.hp["momentum"] > 0)
    case = KR.Case(f"skipseq-{kind}", kind, "few", hp0, seeded=True)
    pre = KR.inputs(case)
    hp = KR.abi_hp(kind, case.hp)
    pb = Problem(lib, cuda, kind, pre, case.hp)
    counts = [0, 0, 0]
    for step, live in enumerate([1, 0, 0, 1, 0, 1]):
        skip = [0, 1 - live, 0]
        counts = [c + 1 - s for c, s in zip(counts, skip)]
        g = KR.inputs(case._replace(name=f"{case.name}-{step}"))["g"]
        pb.set(g=g, skip=skip, steps=counts)
        cur = pb.got()
        now = dict(pre, p=cur["p"], g=g, state=cur["state"], skip=torch.tensor(skip, dtype=torch.uint8), steps=torch.tensor(counts, dtype=torch.int32))
        _, worst = _one_step_checked(pb, now, hp, "counts" if kind == "AdamW" else None)
        print(kind, "step", step, "live" if live else "skipped", {q: round(x, 3) for q, x in worst.items()})
    assert counts == [6, 3, 6]


# ---- F. AdamW's count per segment ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.9, 0.95)])
def test_adamw_counts_per_segment_vs_torch(lib, cuda, betas):
    """Three segments: live throughout, no gradient for the first 5 of 8 steps, never live.  torch.optim.AdamW (fp64, CPU, fed the
    same gradients, None where not live) keeps its own step per parameter; before every step its parameters and moments are set to
    the kernel's, so the comparison is one step deep and per element under AdamW's bars.  The late segment's first update is
    corrected with step 1, as torch's is."""
    ci = KR.count_inputs(betas)
    hp = KR.abi_hp("AdamW", ci["hp"])
    seg = ci["seg"]
    n = seg[-1]
    pre0 = {"seg": seg, "p": ci["p"], "g": ci["grads"][0], "state": {"exp_avg": torch.zeros(n), "exp_avg_sq": torch.zeros(n)}}
    pb = Problem(lib, cuda, "AdamW", pre0, ci["hp"])
    ps = [torch.nn.Parameter(ci["p"][a:b].double().clone()) for a, b in zip(seg, seg[1:])]
    opt = torch.optim.AdamW(ps, lr=hp["lr"], betas=(hp["beta1"], hp["beta2"]), eps=hp["eps"], weight_decay=hp["weight_decay"], foreach=False)
    counts = [0, 0, 0]
    for step in range(KR.COUNT_STEPS):
        live = KR.count_schedule(step)
        skip = [0 if l else 1 for l in live]
        counts = [c + int(l) for c, l in zip(counts, live)]
        g = ci["grads"][step]
        pb.set(g=g, skip=skip, steps=counts)
        cur = pb.got()
        with torch.no_grad():  # re-seed torch from the kernel's state; its step counts stay its own
            for s, (q, (a, b)) in enumerate(zip(ps, zip(seg, seg[1:]))):
                q.copy_(cur["p"][a:b].double())
                if opt.state[q]:
                    opt.state[q]["exp_avg"].copy_(cur["state"]["exp_avg"][a:b].double())
                    opt.state[q]["exp_avg_sq"].copy_(cur["state"]["exp_avg_sq"][a:b].double())
                q.grad = g[a:b].double().clone() if live[s] else None
        opt.step()
        ref = {"p": torch.cat([q.detach() for q in ps]), "g": g.double(), "diag": {}, "lion_c": None,
               "state": {k: torch.cat([opt.state[q][k] if opt.state[q] else torch.zeros(b - a, dtype=torch.float64) for q, (a, b) in zip(ps, zip(seg, seg[1:]))])
                         for k in ("exp_avg", "exp_avg_sq")}}
        now = {"seg": seg, "p": cur["p"], "g": g, "state": cur["state"], "skip": torch.tensor(skip, dtype=torch.uint8),
               "steps": torch.tensor(counts, dtype=torch.int32)}
        before = cur
        pb.step("counts")
        pb.assert_guards()
        got = pb.got()
        worst = KR.check("AdamW", now, got, hp, ref=ref)
        _assert_skipped_kept(now, before, got)
        print(betas, "step", step, "counts", counts, {q: round(x, 3) for q, x in worst.items()})
        assert [int(opt.state[q]["step"]) if opt.state[q] else 0 for q in ps] == counts
    assert counts == [8, 3, 0]


def _dino_student(cuda):
    from headct_foundation_amd.dino_model import DINOHead, MultiCropWrapper, ViTBackbone
    b = ViTBackbone(img_size=24, patch_size=12, in_chans=3, hidden_size=48, mlp_dim=96, num_layers=2, num_heads=3)  # the tiny plumbing yaml
    return MultiCropWrapper(b, DINOHead(48, 512, hidden_dim=64, bottleneck_dim=32)).to(cuda)


class _DinoRun:
    """test_dino_iteration_and_merged_state_dict's tiny student under DinoOptimizer(kind="AdamW"), five iterations on fixed crops, the
    prototype layer's gradients cancelled for the first two (engine_pretrain_dino.cancel_gradients_last_layer at epoch 0 of
    DINO.FREEZE_LAST_LAYER = 1)."""
    ITERS, FROZEN = 5, 2

    def __init__(self, cuda, betas):
        from headct_foundation_amd.dino import DINOLoss
        torch.manual_seed(6)
        self.cuda, self.betas = cuda, betas
        self.init = _dino_student(cuda).state_dict()
        self.crops = [[torch.rand(2, 3, 24, 24, 24, device=cuda) for _ in range(4)] for _ in range(self.ITERS)]
        self.crit = DINOLoss(512, 4, 0.04, 0.04, 30, 200).to(cuda)
        teacher = self.student()
        with torch.no_grad():
            self.t_out = [teacher(c[:2])['dino_output'].float() for c in self.crops]

    def student(self, state=None):
        m = _dino_student(self.cuda)
        m.load_state_dict(state or self.init)
        return m

    def optimizer(self, model):
        from headct_foundation_amd.dino import DinoOptimizer
        return DinoOptimizer(model, lr=1e-3, betas=self.betas, weight_decay=0.04, kind="AdamW")

    def iteration(self, it, model, opt, sync_is_error=False):
        from engine_pretrain_dino import cancel_gradients_last_layer
        opt.zero_grad()
        self.crit.center.zero_()
        loss = self.crit(model(self.crops[it])['dino_output'].float(), self.t_out[it], 0)
        loss.backward()
        cancel_gradients_last_layer(0 if it < self.FROZEN else 1, model, 1)
        if sync_is_error:
            torch.cuda.set_sync_debug_mode("error")
        try:
            opt.step()
        finally:
            torch.cuda.set_sync_debug_mode("default")


def _spy_on_adamw(monkeypatch, lib):
    calls = []
    for name in ("hct_adamw_step", "hct_adamw_step_scaled", "hct_adamw_step_counts"):
        monkeypatch.setattr(lib, name, lambda *a, _fn=getattr(lib, name), _name=name: (calls.append((_name, a[14])), _fn(*a))[1])
    return calls


def test_uniform_counts_keep_the_uniform_launch(lib, cuda, monkeypatch):
    """While every live segment has had the same number of updates HipAdamW launches what it always did: hct_adamw_step with that
    count (the MAE step, DINO before the thaw) and one CPU scalar shared by every state entry.  Once the prototype layer thaws the
    head goes through hct_adamw_step_counts, the backbone does not; and a step whose skip key has not changed does not synchronise
    with the device (torch's sync debug mode set to raise around it)."""
    from headct_foundation_amd import HipAdamW
    from oracle import mae_oracle as O
    from tests.util import build_hip_model
    calls = _spy_on_adamw(monkeypatch, lib)
    cfg = O.CONFIGS["micro"]
    model = build_hip_model(cfg, O.make_params(cfg, 0), cuda, "fp32", full_pred=False)
    opt = HipAdamW(model, lr=1e-3, betas=(0.9, 0.95), weight_decay=5e-3)
    for step in range(3):
        opt.zero_grad()
        loss, _, _ = model(O.make_volume(cfg, 2, 10 + step).to(cuda), noise=O.make_noise(cfg, 2, 10 + step).to(cuda))
        loss.backward()
        opt.step()
    assert calls == [("hct_adamw_step", 1), ("hct_adamw_step", 2), ("hct_adamw_step", 3)]
    assert len({id(s["step"]) for s in opt.state.values()}) == 1 and all(float(s["step"]) == 3.0 for s in opt.state.values())
    del calls[:]
    run = _DinoRun(cuda, (0.9, 0.999))
    student = run.student()
    dopt = run.optimizer(student)
    for it in range(run.ITERS):
        run.iteration(it, student, dopt, sync_is_error=it in (1, 3, 4))  # the skip key changes at 0 (first upload) and at 2 (the thaw)
    names = [n for n, _ in calls]
    assert names[:2 * run.FROZEN] == ["hct_adamw_step"] * (2 * run.FROZEN)
    assert names[2 * run.FROZEN:] == ["hct_adamw_step", "hct_adamw_step_counts"] * (run.ITERS - run.FROZEN)
    assert [a for n, a in calls if n == "hct_adamw_step"] == [1, 1, 2, 2, 3, 4, 5]


@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.9, 0.95)])
def test_dino_thaw_matches_torch_adamw_fed_the_hip_gradients(lib, cuda, betas):
    """The HIP path's own gradients go to a torch.optim.AdamW twin (fp32, the hyper-parameters as the C ABI holds them), None where
    the engine cancelled them.  Every parameter and moment agrees at test_mae_update_vs_restatement_fed_the_hip_gradients's
    tolerance (1e-6 relative per tensor, times the steps so far) at every iteration -- the thawed prototype layer too, whose first
    update torch corrects with step 1 -- and state_dict()'s `step` of every parameter torch has state for is torch's."""
    run = _DinoRun(cuda, betas)
    model = run.student()
    opt = run.optimizer(model)
    twin = [torch.nn.Parameter(p.detach().clone()) for p in model.parameters()]
    names = [n for n, _ in model.named_parameters()]
    topt = torch.optim.AdamW(twin, lr=KR.f32(1e-3), betas=(KR.f32(betas[0]), KR.f32(betas[1])), eps=KR.f32(1e-8), weight_decay=KR.f32(0.04), foreach=False)
    last = [i for i, (n, p) in enumerate(model.named_parameters()) if "last_layer" in n and p.requires_grad]
    for it in range(run.ITERS):
        run.iteration(it, model, opt)
        for q, p in zip(twin, model.parameters()):
            q.grad = None if p.grad is None else p.grad.detach().clone()
        assert all((twin[i].grad is None) == (it < run.FROZEN) for i in last) and last
        topt.step()
        sd, tsd = opt.state_dict(), topt.state_dict()
        worst = 0.0
        for i, (n, q, p) in enumerate(zip(names, twin, model.parameters())):
            e = rel_err(p.detach(), q.detach()) if float(q.detach().abs().max()) > 0 else float(p.detach().abs().max())
            worst = max(worst, e)
            assert e < 1e-6 * (it + 1), (it, n, e)
            if i in tsd["state"]:
                assert int(sd["state"][i]["step"]) == int(tsd["state"][i]["step"]), (it, n, sd["state"][i]["step"], tsd["state"][i]["step"])
                for k in ("exp_avg", "exp_avg_sq"):
                    ref = tsd["state"][i][k]
                    assert rel_err(sd["state"][i][k], ref) < 1e-6 * (it + 1) or float(ref.abs().max()) == 0.0 and not sd["state"][i][k].any(), (it, n, k)
        print(betas, "iteration", it, "worst per-tensor relative error", f"{worst:.2e}", "last layer step",
              [int(sd["state"][i]["step"]) for i in last])
    assert [int(sd["state"][i]["step"]) for i in last] == [run.ITERS - run.FROZEN] * len(last)


def test_dino_thaw_resume_is_bit_equal(lib, cuda):
    """state_dict() after the first iteration (mid-freeze) and after the third (the thawed layer one update old) -> a fresh student
    and optimizer -> load_state_dict -> continue: the bits of the uninterrupted run, which needs every parameter's own count back."""
    run = _DinoRun(cuda, (0.9, 0.999))
    model = run.student()
    opt = run.optimizer(model)
    for it in range(run.ITERS):
        run.iteration(it, model, opt)
    m2 = run.student()
    o2 = run.optimizer(m2)
    for it in range(run.ITERS):
        run.iteration(it, m2, o2)
        if it in (0, 2):
            sd, weights = copy.deepcopy(o2.state_dict()), copy.deepcopy(m2.state_dict())
            m2 = run.student(weights)
            o2 = run.optimizer(m2)
            o2.load_state_dict(sd)
    for (n, a), (_, b) in zip(model.named_parameters(), m2.named_parameters()):
        assert torch.equal(a, b), n
    sa, sb = opt.state_dict()["state"], o2.state_dict()["state"]
    assert sorted(sa) == sorted(sb)
    for i in sa:
        assert int(sa[i]["step"]) == int(sb[i]["step"]) and torch.equal(sa[i]["exp_avg"], sb[i]["exp_avg"]) and torch.equal(sa[i]["exp_avg_sq"], sb[i]["exp_avg_sq"]), i
    assert len({int(v["step"]) for v in sa.values()}) == 2  # the thawed layer's count is its own
