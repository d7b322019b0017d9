"""CPU: tests/lora_kernel_ref.py pinned down before tests/test_lora_kernels_gpu.py relies on it.

 - exact() against tests/lora_ref.lora_update and against torch autograd on test_lora_gpu._kernel_ref's formulation, in float64;
 - every `integers` case is exact in bf16 and in fp32 in any summation order, and its U and dx1 increment are mostly non-zero;
 - the table holds what it claims, asserted from instance(...), the restatement of lora.hip::rmw_launch;
 - the bound is worth having: eight planted defects are flagged per element on `gaussian` (a result that sits at the defective
   value and carries a whole bound of rounding noise of its own is still outside: |bad - exact| > 2 bound somewhere) and break bit
   equality on `integers`, at every case that reaches an MFMA instance and that the defect applies to."""
import pytest
import torch

from tests import lora_kernel_ref as K
from tests import lora_ref as R
from tests.test_lora_gpu import _kernel_ref

MFMA = K.mfma_cases()


def test_positions_and_placement():
    for N, H in ((1, 1), (5, 1), (1, 3), (2, 3), (7, 3), (16, 8), (9, 8)):
        head, tok = K.positions(N, H)
        h2, t2 = R.lora_positions(N, H)
        assert torch.equal(head, h2) and torch.equal(tok, t2)
        assert len({(int(a), int(b)) for a, b in zip(head.flatten(), tok.flatten())}) == N * H  # a bijection onto heads x tokens
    case = K.Case("p", 2, 7, 3, 8, 32)
    V = torch.arange(2 * 7 * 2 * 24, dtype=torch.float64).view(2, 7, 2, 24) + 1
    P = K.place(case, V)
    assert torch.equal(K.gather(case, P), V) and not P[:, :, 1].any()


@pytest.mark.parametrize("name", ["fp32-r32-3x9x3x16", "fp32-r96-1x17x2x32", "fp32-r64-2x37x2x64"])
def test_exact_is_the_restatement_and_its_autograd(name):
    case = next(c for c in K.CASES if c.name == name)
    d = dict(K.make_data(case, "gaussian"))
    d["T"] = K.exact(case, d)["T"]  # the float64 chain: T unrounded, as lora_update and autograd have it
    ex = K.exact(case, d)
    t = {k: d[k] for k in ("x1", "qkv", "dqkv", "dx0", "Aq", "Av", "Bq", "Bv")}
    want = _kernel_ref(t, case.H, "fp32")
    close = lambda a, b: float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))
    assert close(ex["qkv"], want[0]) and close(ex["T"].view(case.B, case.N, -1), want[1])
    for i, k in enumerate(("dAq", "dAv", "dBq", "dBv")):
        assert close(ex[k], want[2 + i]), k
    assert close(ex["inc"].view(case.B, case.N, case.D), want[6])
    assert close(ex["dx1"], d["dx0"].double().view(case.M, case.D) + want[6].reshape(case.M, case.D))
    for z, (a, b) in enumerate((("Aq", "Bq"), ("Av", "Bv"))):
        upd = R.lora_update(d["x1"].double(), d[a].double(), d[b].double(), case.H)   # [B, H, N, dh]
        assert close(ex["U"][:, :, 2 * z].permute(0, 2, 1, 3), upd)
    assert not ex["U"][:, :, 1].any()


def test_integer_cases_are_exact_and_not_trivial():
    """Every stored value is an integer of magnitude <= 256 (exact in bf16), |T| <= 8, |U| <= 64 and |dT| <= 4 by construction, every
    partial sum in any order is below 2^24 (the sums of absolute terms are), U and the dx1 increment are non-zero on >= 90 % of their
    elements, and the old qkv values of neighbouring dh blocks of a volume differ (a mis-sent block cannot land on an equal one)."""
    top = dict(U=0.0, qkv=0.0, inc=0.0, dx1=0.0)
    for case in K.CASES:
        d = K.make_data(case, "integers")
        ex = K.exact(case, d)
        M, D, r = case.M, case.D, case.r
        for k in ("x1", "qkv", "dqkv", "dx0", "Aq", "Av", "Bq", "Bv", "T"):
            assert torch.equal(d[k], d[k].round()) and float(d[k].abs().max()) <= 64, (case.name, k)
        assert torch.equal(d["T"].double(), ex["T"]), case.name
        for k in K.OUTPUTS + ("inc", "dT", "U"):
            assert torch.equal(ex[k], ex[k].round()), (case.name, k)
        assert float(ex["T"].abs().max()) <= 8 and float(ex["dT"].abs().max()) <= 4 and float(ex["U"].abs().max()) <= 64, case.name
        for k in top:
            top[k] = max(top[k], float(ex[k].abs().max()))
            assert float(ex[k].abs().max()) <= 256, (case.name, k)
        # sums of absolute terms: no partial sum of any product, in any order, reaches 2^24
        x1, dU = d["x1"].double().view(M, D).abs(), K.gather(case, d["dqkv"].double()).view(M, 2, D).abs()
        for z, (a, b) in enumerate((("Aq", "Bq"), ("Av", "Bv"))):
            dT = ex["dT"][:, z * r:(z + 1) * r].abs()
            sums = (dU[:, z].t() @ ex["T"][:, z * r:(z + 1) * r].abs(), dT.t() @ x1, dU[:, z] @ d[b].double().abs(), dT @ d[a].double().abs() * 2 + 64)
            assert max(float(s.max()) for s in sums) < 2 ** 24, case.name
        U = K.gather(case, ex["U"])
        assert float((U != 0).double().mean()) >= 0.90, (case.name, "U", float((U != 0).double().mean()))
        assert float((ex["inc"] != 0).double().mean()) >= 0.90, (case.name, "inc", float((ex["inc"] != 0).double().mean()))
        if case.N * case.H > 1:
            for z in range(2):
                blocks = K.gather(case, d["qkv"].double())[:, :, z].reshape(case.B, case.N * case.H, case.dh)
                assert bool((blocks[:, 1:] != blocks[:, :-1]).any(dim=2).all()), case.name
    print("integers: largest |U| {U:.0f}, |old + U| {qkv:.0f}, |dT A| {inc:.0f}, |dx0 + dT A| {dx1:.0f}".format(**top))


def test_table_holds_what_it_claims():
    assert len({c.name for c in K.CASES}) == len(K.CASES)
    fwd = {c.fwd_instance for c in K.CASES}
    bwd = {c.bwd_instance for c in K.CASES}
    assert {("mfma", ks, 1) for ks in (1, 2, 4)} <= fwd and {("mfma", ks, 2) for ks in (1, 2, 4)} <= bwd
    assert ("generic",) in fwd and ("generic",) in bwd
    for inst, which in [(("mfma", ks, p), p) for ks in (1, 2, 4) for p in (1, 2)]:
        Ms = [c.M for c in K.CASES if (c.fwd_instance if which == 1 else c.bwd_instance) == inst]
        assert set(K.M_EDGES) <= set(Ms), inst
        assert any(m % 16 for m in Ms) and any(m > K.KROWS_WAVE for m in Ms) and any(m > K.KROWS_WG for m in Ms), inst
        Bs = {c.B > 1 for c in K.CASES if (c.fwd_instance if which == 1 else c.bwd_instance) == inst}
        assert Bs == {True, False}, inst
    # every reason for the generic kernel, alone
    why_f = {K.generic_reasons(c.dtype, c.D, c.dh, c.r, True, c.qkv_off % 8 == 0, True) for c in K.CASES}
    why_b = {K.generic_reasons(c.dtype, c.D, c.dh, c.r, c.at, True, False) for c in K.CASES}
    assert {("fp32",), ("D % 64",), ("rank",), ("alignment",), ("dh % 8",)} <= why_f, why_f
    assert {("fp32",), ("D % 64",), ("rank",), ("no transposed copy",)} <= why_b, why_b
    assert {c.r for c in K.CASES if c.dtype == "fp32"} == {32, 64, 96, 128}
    assert any(c.dtype == "bf16" and c.r == 96 for c in K.CASES) and any(c.dtype == "bf16" and c.D == 48 for c in K.CASES)
    assert {(c.at, c.bt) for c in K.CASES if c.dtype == "bf16"} == {(True, True), (True, False), (False, True), (False, False)}
    # the geometry of the permutation on the MFMA path
    geo = {(c.H, c.dh) for c in MFMA if c.fwd_instance[0] == "mfma"}
    assert {(8, 8), (4, 16), (4, 48), (2, 64), (1, 64), (1, 128), (3, 64), (12, 64)} <= geo
    for H in (8, 4, 3):
        Ns = {c.N for c in MFMA if c.H == H}
        assert 1 in Ns and any(1 < n < H for n in Ns) and any(n > H and n % H == 0 for n in Ns)
        assert any(n > H and all(n % p or H % p for p in range(2, H + 1)) for n in Ns)  # coprime
        assert any(n > H and n % H and not all(n % p or H % p for p in range(2, H + 1)) for n in Ns) or H == 3
    assert any(c.B > 1 and c.N > 1 and c.H > 1 for c in MFMA) and any(c.B == 1 for c in MFMA)
    assert max(c.D for c in K.CASES if "vitb" not in c.name) <= 192 and max(c.M * c.D for c in K.CASES) == 2 * 513 * 768


def test_instance_restates_the_launch():
    """Hand-read from lora.hip::rmw_launch, lora_scatter, lora_dx_accum and hct_lora_qv_bwd's `tr`."""
    assert K.instance("bf16", 768, 64, 128, True, True) == ("mfma", 4, 1)
    assert K.instance("bf16", 64, 8, 32, False, True) == ("mfma", 1, 1)            # the scatter's B is [D, r] row-major as passed
    assert K.instance("bf16", 128, 64, 64, True, True, scatter=False) == ("mfma", 2, 2)
    assert K.instance("bf16", 128, 64, 64, False, True, scatter=False) == ("generic",)
    assert K.instance("bf16", 64, 4, 32, True, True) == ("generic",) and K.instance("bf16", 64, 4, 32, True, True, scatter=False) == ("mfma", 1, 2)
    assert K.instance("bf16", 64, 8, 32, True, False) == ("generic",)
    assert K.instance("bf16", 128, 64, 96, True, True) == ("generic",) and K.instance("bf16", 48, 16, 32, True, True) == ("generic",)
    assert K.instance("fp32", 128, 64, 64, True, True) == ("generic",)


GRADS = ("dAq", "dAv", "dBq", "dBv", "dx1")


def _flagged(bad, ex, b):
    return (bad - ex).abs() > 2.0 * b


def _asked(case, defect):
    """The groups of outputs that must show `defect` at this case: qkv where the scatter is an MFMA instance, dx1 where the dx1
    product is; the gather feeds every gradient, and one of them must show it wherever either product is an MFMA instance."""
    outs = K.DEFECTS[defect][1]
    f, b = case.fwd_instance[0] == "mfma", case.bwd_instance[0] == "mfma"
    if "grads" in outs:
        return [GRADS] if f or b else []
    return [(o,) for o in outs if (f if o == "qkv" else b)]


def _bits(case, k, v):
    return K.stored(v, 1 if case.dtype == "bf16" and k in ("qkv", "dx1") else 0)


@pytest.mark.parametrize("defect", list(K.DEFECTS))
def test_bound_separates_planted_defects(defect):
    reach = [c for c in MFMA if _asked(c, defect)]
    cases = [c for c in reach if K.applies(c, defect)]
    assert len(cases) >= 0.75 * len(reach), (defect, len(cases), len(reach))
    low = (1.0, "")
    for case in cases:
        for gen in ("gaussian", "integers"):
            d = K.make_data(case, gen)
            ex, bad = K.exact(case, d), K.exact(case, d, defect)
            b = K.bound(case, d, ex) if gen == "gaussian" else None
            for group in _asked(case, defect):
                if gen == "gaussian":
                    n = sum(int(_flagged(bad[k], ex[k], b[k]).sum()) for k in group)
                    moved = sum(int((bad[k] != ex[k]).sum()) for k in group)
                    assert n > 0, (case.name, defect, group)
                    low = min(low, (n / moved, f"{case.name}/{group[0]}"))
                else:
                    assert any(not torch.equal(_bits(case, k, bad[k]), _bits(case, k, ex[k])) for k in group), (case.name, defect, group)
    print(f"{defect}: {len(cases)} of {len(reach)} cases; lowest share of the moved elements flagged at 2 x bound: {low[0]:.3f} ({low[1]})")
