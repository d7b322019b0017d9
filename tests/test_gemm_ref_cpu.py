"""CPU: tests/gemm_ref.py pinned down before tests/test_gemm_kernels_gpu.py relies on it.

 - exact() against F.linear, F.gelu and their autograd in float64 (1e-12);
 - every `integers` case keeps every partial sum, in any order, below 2^24 (so bit equality is a fair demand);
 - every table entry plans, on 256 CUs, the kernel, epilogue instance, tile height, split and stream-K sharing that its comment
   claims (hct_gemm_describe: host arithmetic, no device);
 - the erff allowance is 4 x what torch's fp32 gelu / gelu' miss float64 by on the tables' pre-activations;
 - the bound is worth having: four planted defects are flagged in >= 95 % of the elements they touch, in every `gaussian` case with
   K <= 320, and break bit equality in every `integers` case."""
import pytest
import torch
import torch.nn.functional as F

from tests import gemm_ref as R

ALL = R.all_hct_gemm_cases()
FAMILIES = {"nt256": [c for c in ALL if c.kernel == R.NT256], "nt128": [c for c in ALL if c.kernel == R.NT128],
            "tn": [c for c in ALL if c.kernel in (R.TN128, R.TN256)], "generic": [c for c in ALL if c.kernel == R.GENERIC]}


def test_tables_have_the_cases_the_kernels_need():
    assert len({c.name for c in ALL}) == len(ALL)
    assert all(len(v) > 100 for v in FAMILIES.values())
    nt = FAMILIES["nt256"]
    assert {c.mode for c in nt} == {0, 1, 2, 3, 4} and any(c.fuse for c in nt) and any(c.sk for c in nt) and any(c.rows == 192 for c in nt)
    assert any(c.c2_dtype >= 0 for c in nt) and any(c.alpha != 1 for c in nt) and any(c.lda == 2 * c.K for c in nt)
    tn = FAMILIES["tn"]
    assert any(c.kernel == R.TN128 and c.split and c.c2_dtype >= 0 for c in tn), "gemm_fold_kernel never gets a real epilogue"
    assert any(c.kernel == R.TN128 and c.c_dtype == R.BF16 for c in tn) and any(c.kernel == R.TN128 and c.hook == 128 for c in tn)
    gen = FAMILIES["generic"]
    assert {(c.a_dtype, c.b_dtype) for c in gen} == set(R.GEN_DTYPES) and {(c.transA, c.transB) for c in gen} == set(R.GEN_LAYOUTS)
    assert {c.act for c in gen} == {R.NONE, R.GELU, R.GELU_D, R.DGELU, R.MULAUX} and any(c.K % 16 for c in gen)


@pytest.mark.parametrize("act", [R.NONE, R.GELU, R.GELU_D, R.DGELU, R.MULAUX])
@pytest.mark.parametrize("layout", R.GEN_LAYOUTS)
def test_exact_is_the_headers_formula(act, layout):
    """act(alpha op(A) op(B) + bias) (+ residual) with F.linear / F.gelu / autograd in float64."""
    tA, tB = layout
    case = R.Case(name="pin", M=13, N=12, K=21, transA=tA, transB=tB, a_dtype=R.F32, b_dtype=R.BF16, c_dtype=R.BF16, bias=True, residual=True,
                  act=act, aux_dtype=R.BF16 if act else -1, c2_dtype=R.F32, alpha=-0.75, colsum=True)
    d = R.make_data(case, "gaussian")
    A = d["A"].double().t() if tA else d["A"].double()
    W = d["B"].double() if tB else d["B"].double().t()
    lin = F.linear(A, case.alpha * W, d["bias"].double()).requires_grad_(True)
    u = d["aux"].double().requires_grad_(True)
    F.gelu(lin).sum().backward()
    F.gelu(u).sum().backward()
    want = {R.NONE: lin, R.GELU: F.gelu(lin), R.GELU_D: F.gelu(lin), R.DGELU: lin * u.grad, R.MULAUX: lin * u}[act].detach() + d["res"].double()
    ex = R.exact(case, d)
    assert float((ex["C"] - want).abs().max()) < 1e-12 and ex["C2"] is ex["C"]
    if act == R.GELU:
        assert float((ex["aux"] - lin.detach()).abs().max()) < 1e-12
    if act == R.GELU_D:
        assert float((ex["aux"] - lin.grad).abs().max()) < 1e-12
    # column sums of the separate pass: of C as stored; of the fused form: of the unrounded value
    assert float((ex["colsum"] - want.float().bfloat16().double().sum(0)).abs().max()) < 1e-12
    fused = R.exact(R.dataclasses.replace(case, fuse=True), d)
    assert float((fused["colsum"] - want.sum(0)).abs().max()) < 1e-12


@pytest.mark.parametrize("family", list(FAMILIES))
def test_integer_cases_are_exact_in_fp32(family):
    """Every partial sum in any order stays below 2^24 in magnitude (and is a multiple of 1/2): fp32 arithmetic on them is exact,
    whatever the order of an MFMA, a split-K fold or a stream-K slab; fp32 CPU matmul agrees with float64 bit for bit."""
    n = 0
    for case in FAMILIES[family]:
        if "integers" not in case.gens:
            continue
        d = R.make_data(case, "integers")
        assert R.max_partial_sum(case, d) < 2 ** 24, case.name
        A32 = d["A64"].float()
        assert torch.equal((A32 @ d["B64"].float().t()).double(), d["P"]), case.name
        ex = R.exact(case, d)
        assert torch.equal(ex["C"] * 2, (ex["C"] * 2).round()), case.name
        n += 1
    assert n > 40


@pytest.mark.parametrize("family", list(FAMILIES))
def test_every_case_plans_what_its_comment_claims(lib, family):
    for case in FAMILIES[family]:
        assert R.check_plan(lib, case, 256) is None, (case.name, R.check_plan(lib, case, 256))
    if family == "nt256":  # the stream-K shape is the first of the older test's candidates that the plan shares out
        first = next(s for s in R.SK_CANDIDATES if R.check_plan(lib, R.nt_cases(R.NT256, *s, 0, "strided", sk=True)[0], 256) is None)
        assert first == R.SK_SHAPE_256_CUS
        # M = 449 on 192-row tiles is three row tiles with 65 rows in the last
        assert (449 + 191) // 192 == 3 and 449 - 2 * 192 == 65


def test_erf_gelu_allowance_is_four_times_the_measured_error():
    """torch's fp32 F.gelu and its autograd derivative against float64 over the pre-activations (GELU, GELU_D) and saved
    pre-activations (DGELU) of every gaussian case that takes an erff epilogue, per unit of max(1, |x|)."""
    worst_g = worst_d = 0.0
    seen = set()
    for case in ALL:
        if case.act not in (R.GELU, R.GELU_D, R.DGELU) or case.fast_gelu:
            continue
        key = (case.M, case.N, case.K, case.transA, case.transB, case.a_dtype, case.b_dtype, case.act == R.DGELU, case.alpha)
        if key in seen:
            continue
        seen.add(key)
        d = R.make_data(case, "gaussian")
        x = (d["aux"].double() if case.act == R.DGELU else case.alpha * d["P"] + d["bias"].double())
        x32 = x.float().requires_grad_(True)
        g32 = F.gelu(x32)
        g32.sum().backward()
        x = x32.detach().double()
        scale = x.abs().clamp(min=1.0)
        worst_g = max(worst_g, float(((g32.detach().double() - R.gelu64(x)).abs() / scale).max()))
        worst_d = max(worst_d, float(((x32.grad.double() - R.dgelu64(x)).abs() / scale).max()))
    print(f"measured fp32 erf gelu error {worst_g:.3e}, gelu' error {worst_d:.3e} per max(1, |x|); allowances {R.ERF_GELU_ALLOW:.1e}, {R.ERF_DGELU_ALLOW:.1e}")
    assert 0.9 <= R.ERF_GELU_ALLOW / (4 * worst_g) <= 1.1
    assert 0.9 <= R.ERF_DGELU_ALLOW / (4 * worst_d) <= 1.1


DEFECTS = ("kslice", "row", "quad", "alpha")          # integers: one row / one quad at a seeded place
DEFECTS_EVERYWHERE = ("kslice", "rows", "zero", "alpha")  # gaussian: the row and the quad defect at every place, nothing selected


def _applies(case, defect):
    return not ((defect in ("row", "rows") and case.M < 2) or (defect == "quad" and case.N < 4) or (defect == "alpha" and case.alpha == 1.0))


@pytest.mark.parametrize("family", list(FAMILIES))
def test_bound_flags_planted_defects(family):
    """One 32-deep K slice dropped, a row taken from its neighbour, a quad zeroed, alpha ignored.  For the Gaussian share the row and
    the quad defect are planted at every place at once (every row from its neighbour, every element zeroed): the share is over
    all rows and quads, none picked.  For the integer cases one row / one quad at a place seeded by the case's name."""
    low = (1.0, "")
    for case in FAMILIES[family]:
        if "gaussian" in case.gens and case.K <= 320:  # (the 95 % is asked of K <= 320 only; bit inequality below of every case)
            d = R.make_data(case, "gaussian")
            ex = R.exact(case, d)
            b = R.bound(case, d, ex)
            for defect in DEFECTS_EVERYWHERE:
                if not _applies(case, defect):
                    continue
                region = R.defect_region(case, d, defect)
                bad = R.exact(case, d, defect)
                flagged = ((bad["C"] - ex["C"]).abs() > b["C"])[region]
                if ex["aux"] is not None and defect in ("kslice", "alpha"):  # (an element is flagged if any output at its place is:
                    flagged = flagged | ((bad["aux"] - ex["aux"]).abs() > b["aux"])[region]  # gelu is flat where the written aux is not)
                frac = float(flagged.double().mean())
                low = min(low, (frac, f"{case.name}/{defect}"))
                assert frac >= 0.95, (case.name, defect, frac)
        if "integers" in case.gens:
            d = R.make_data(case, "integers")
            want = R.stored(R.exact(case, d)["C"], case.c_dtype)
            for defect in DEFECTS:
                if _applies(case, defect):
                    assert not torch.equal(R.stored(R.exact(case, d, defect)["C"], case.c_dtype), want), (case.name, defect)
    print(f"{family}: lowest flagged share {low[0]:.4f} ({low[1]})")


def test_locate_names_the_wave_the_kernels_use():
    """Hand-computed from csrc/gemm.hip: NT256 / TN256 have 8 waves = 4 (M) x 2 (N), wm = wave >> 1, wn = wave & 1, each
    16 * MT rows (64, or 48 on 192-row tiles) x 128 columns; NT128 / TN128 4 waves = 2 x 2 of 64 x 64; the generic kernel's wave
    w holds rows 16 w .. 16 w + 15 of its 64 x 64 tile."""
    c = lambda kernel, rows=256: R.Case(name="where", M=600, N=600, K=128, kernel=kernel, rows=rows)
    assert R.locate(c(R.NT256), 70, 200) == ((0, 0), (1, 1))          # row 70 is in the second 64-row wave, column 200 in the second 128
    assert R.locate(c(R.NT256), 256 + 255, 256 + 127) == ((1, 1), (3, 0))
    assert R.locate(c(R.NT256, 192), 70, 200) == ((0, 0), (1, 1))     # 48-row waves: rows 48 .. 95
    assert R.locate(c(R.NT256, 192), 192 + 47, 128) == ((1, 0), (0, 1))
    assert R.locate(c(R.NT256, 192), 192 + 144, 127) == ((1, 0), (3, 0))
    assert R.locate(c(R.TN256), 300, 511) == ((1, 1), (0, 1))         # row 44 of tile row 1
    assert R.locate(c(R.TN256), 255, 0) == ((0, 0), (3, 0))
    for k in (R.NT128, R.TN128):
        assert R.locate(c(k), 70, 200) == ((0, 1), (1, 1))            # column 200 = 72 of tile column 1: second 64
        assert R.locate(c(k), 128 + 63, 63) == ((1, 0), (0, 0))
    assert R.locate(c(R.GENERIC), 70, 200) == ((1, 3), (0, 0))        # row 6 of tile row 1: ty = 1, wave 0
    assert R.locate(c(R.GENERIC), 63, 5) == ((0, 0), (3, 0))


def test_guarded_layout():
    fill = torch.arange(15.0).reshape(3, 5)
    g = R.guarded((3, 5), 9, torch.float32, fill=fill, off=4)
    assert g.start % 128 == 4 and g.start >= 2 * 9 and g.flat.numel() >= g.start + (3 + 2) * 9
    assert torch.equal(g.view, fill) and int(torch.isnan(g.flat).sum()) == g.flat.numel() - 15 and g.outside_is_nan()
    g.flat[g.start + 5] = 1.0  # a gap column
    assert not g.outside_is_nan()
    out = R.guarded((3, 5), 9, torch.bfloat16)
    assert bool(torch.isnan(out.flat).all()) and out.ptr == out.flat.data_ptr() + 2 * out.start
