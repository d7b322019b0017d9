"""Every GEMM kernel of csrc/gemm.hip (generic, NT128, persistent NT256 with its 192-row and stream-K forms, TN128, TN256, the grouped
wgrad and gemm_fold_kernel) and every epilogue instance, through the C ABI, against tests/gemm_ref.py: the float64 value of the
header's formula, a derived per-element bound, and integer inputs for which the outputs must be bit-equal.

Every operand and output is a strided view inside a larger NaN-filled allocation (gemm_ref.guarded): outputs must leave every
element outside the view NaN, inputs carry NaN in the gap columns, the guard rows and the rows after the last reduction row, so a
lost column mask, a store past M or N, or a reduction that reads past its end shows.  Every call runs twice into fresh buffers and
must give the same bits.  The plan (kernel, epilogue instance, tile height, split, stream-K) is asserted first on the device's CU
count; tests/test_gemm_ref_cpu.py asserts the same claims for 256 CUs without a device."""
import ctypes as C
import json
import time

import pytest
import torch

from headct_foundation_amd import _lib
from headct_foundation_amd._lib import GemmArgs
from tests import gemm_ref as R

pytestmark = pytest.mark.gpu

STATS = {}  # (kernel, output dtype) -> [worst |err| / bound, integer outputs bit-equal, integer outputs checked]
NAN = float("nan")


def _st():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def ws(lib, cuda):
    """4 MiB for column-sum partials / split-K slabs, then the stream-K region at the end."""
    return torch.zeros((4 << 20) + lib.hct_gemm_nt_stream_k_bytes() + 4096, dtype=torch.uint8, device=cuda)


@pytest.fixture(scope="module", autouse=True)
def summary():
    t0 = time.time()
    yield
    rows = {f"{k[0]}/{k[1]}": dict(worst_ratio=round(v[0], 4), int_equal=v[1], int_checked=v[2]) for k, v in sorted(STATS.items())}
    print("\nGEMM_REF_SUMMARY " + json.dumps(dict(seconds=round(time.time() - t0, 1), rows=rows)))


def _note(case, name, dtype, ratio=None, equal=None):
    kernel = "tn_group" if case.name.startswith("tn_group") else R.KERNEL_NAMES[case.kernel]
    key = (kernel + " colsum", "fp32") if name == "colsum" else (kernel, "bf16" if dtype == R.BF16 else "fp32")
    s = STATS.setdefault(key, [0.0, 0, 0])
    if ratio is not None:
        s[0] = max(s[0], ratio)
    if equal is not None:
        s[1] += int(equal)
        s[2] += 1


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


class Buffers:
    """The guarded device buffers of one call and the hct_gemm_args that point into them."""

    def __init__(self, case, d, dev, after_reduction=2):
        td = R.torch_dtype
        ra = after_reduction if case.transA else 2   # rows after the last reduction row (TN: A and B are [R, .])
        rb = after_reduction if not case.transB else 2
        self.inp = dict(A=R.guarded(case.a_shape, case.lda, td(case.a_dtype), fill=d["A"], off=case.a_off, after=ra).to(dev),
                        B=R.guarded(case.b_shape, case.ldb, td(case.b_dtype), fill=d["B"], off=case.b_off, after=rb).to(dev))
        if case.bias:
            self.inp["bias"] = R.guarded((1, case.N), case.N + 8, torch.float32, fill=d["bias"][None]).to(dev)
        if case.residual:
            self.inp["res"] = R.guarded((case.M, case.N), case.ldr, torch.float32, fill=d["res"]).to(dev)
        if case.aux_dtype >= 0 and not case.aux_written:
            self.inp["aux"] = R.guarded((case.M, case.N), case.ldaux, td(case.aux_dtype), fill=d["aux"]).to(dev)
        self.case, self.dev = case, dev
        self.proto = dict(C=R.guarded((case.M, case.N), case.ldc, td(case.c_dtype), off=case.c_off))
        if case.c2_dtype >= 0:
            self.proto["C2"] = R.guarded((case.M, case.N), case.ldc2, td(case.c2_dtype))
        if case.aux_written:
            self.proto["aux"] = R.guarded((case.M, case.N), case.ldaux, td(case.aux_dtype))
        if case.colsum:
            self.proto["colsum"] = R.guarded((1, case.N), case.N + 8, torch.float32)

    def fresh_outputs(self):
        return {k: g.to(self.dev) for k, g in self.proto.items()}

    def args(self, out):
        c, a = self.case, GemmArgs()
        a.M, a.N, a.K = c.M, c.N, c.K
        a.A, a.a_dtype, a.lda, a.transA = self.inp["A"].ptr, c.a_dtype, c.lda, c.transA
        a.B, a.b_dtype, a.ldb, a.transB = self.inp["B"].ptr, c.b_dtype, c.ldb, c.transB
        a.C, a.c_dtype, a.ldc = out["C"].ptr, c.c_dtype, c.ldc
        a.bias = self.inp["bias"].ptr if c.bias else None
        a.residual, a.ldr = (self.inp["res"].ptr if c.residual else None), c.ldr
        a.act, a.alpha, a.force_generic = c.act, c.alpha, c.force_generic
        if c.aux_dtype >= 0:
            a.aux, a.aux_dtype, a.ldaux = (out["aux"].ptr if c.aux_written else self.inp["aux"].ptr), c.aux_dtype, c.ldaux
        if c.c2_dtype >= 0:
            a.C2, a.c2_dtype, a.ldc2 = out["C2"].ptr, c.c2_dtype, c.ldc2
        a.colsum_out = out["colsum"].ptr if c.colsum else None
        return a


def _dtype_of(case, name):
    return dict(C=case.c_dtype, C2=case.c2_dtype, aux=case.aux_dtype, colsum=R.F32)[name]


def check_outputs(case, d, outs, fails):
    """Guards intact, outputs finite, bit equality (integers) or the per-element bound (gaussian).  Appends texts to `fails`."""
    ex = R.exact(case, d)
    allow = R.bound(case, d, ex) if d["gen"] == "gaussian" else None
    for name, g in outs.items():
        g = g.to("cpu")
        if not g.outside_is_nan():
            fails.append(f"{case.name}/{d['gen']}: {name}: an element outside the [{g.rows}, {g.width}] view (ld {g.ld}) was written")
        got, dt = g.view, _dtype_of(case, name)
        want64 = ex[name] if name != "colsum" else ex[name][None]
        if not bool(torch.isfinite(got).all()):
            bad = (~torch.isfinite(got)).nonzero()[0].tolist()
            fails.append(f"{case.name}/{d['gen']}: {name}: not finite at {bad} (tile, wave {R.locate(case, *bad)})")
            continue
        if d["gen"] == "integers":
            equal = torch.equal(got, R.stored(want64, dt))
            _note(case, name, dt, equal=equal)
            if not equal:
                row, col = (got != R.stored(want64, dt)).nonzero()[0].tolist()
                fails.append(f"{case.name}/integers: {name} differs in {int((got != R.stored(want64, dt)).sum())} elements, first at ({row}, {col}) "
                             f"(tile, wave {R.locate(case, row, col)}): got {float(got[row, col])}, exact {float(want64[row, col])}")
        else:
            b = allow[name] if name != "colsum" else allow[name][None]
            ratio, row, col = R.worst(got.double(), want64, b)
            _note(case, name, dt, ratio=ratio)
            if not ratio <= 1.0:
                fails.append(f"{case.name}/gaussian: {name} |err| / bound = {ratio:.3f} at ({row}, {col}) (tile, wave {R.locate(case, row, col)}): "
                             f"got {float(got[row, col])!r}, exact {float(want64[row, col])!r}")


def assert_plan(lib, case, cuda, args, ws):
    """The plan of the call itself (its own pointers, leading dimensions and workspace size) on the device's own CU count; only the
    stream-K and 192-row claims may be out of reach on another count (the stream-K test skips then; a 192-row case runs on the
    tiles it gets: every check holds for whatever tile height the plan takes)."""
    diff = R.check_plan(lib, case, 0, args, ws.numel())
    if diff is None:
        return
    cus = torch.cuda.get_device_properties(cuda).multi_processor_count
    if diff.startswith("cu-dependent") and cus != 256:
        print(f"{case.name}: {diff} on {cus} CUs")
        return
    pytest.fail(f"{case.name}: {diff}")


def run_cases(lib, cuda, ws, cases, after_reduction=2):
    fails = []
    try:
        for case in cases:
            for gen in case.gens:
                d = R.make_data(case, gen)
                buf = Buffers(case, d, cuda, after_reduction)
                runs = []
                for rep in range(2):
                    out = buf.fresh_outputs()
                    a = buf.args(out)
                    if rep == 0:
                        assert_plan(lib, case, cuda, a, ws)
                    lib.hct_debug_set_gemm_variant(case.hook)
                    _lib.check(lib.hct_gemm(C.byref(a), ws.data_ptr(), ws.numel(), _st()), case.name)
                    runs.append(out)
                lib.hct_debug_set_gemm_variant(0)
                torch.cuda.synchronize()
                for name in runs[0]:
                    if not torch.equal(_bits(runs[0][name].flat), _bits(runs[1][name].flat)):
                        fails.append(f"{case.name}/{gen}: {name}: two launches differ")
                check_outputs(case, d, runs[0], fails)
    finally:
        lib.hct_debug_set_gemm_variant(0)
        lib.hct_set_cu_reserve(0)
    assert not fails, f"{len(fails)} failures:\n" + "\n".join(fails[:40])


@pytest.mark.parametrize("shape", R.nt_shapes(R.NT256), ids=lambda s: "{}x{}x{}-{}".format(s[0], s[1], s[2], s[4]))
def test_nt256(lib, cuda, ws, shape):
    run_cases(lib, cuda, ws, R.nt_cases(R.NT256, *shape))


@pytest.mark.parametrize("shape", R.nt_shapes(R.NT128), ids=lambda s: "{}x{}x{}-{}".format(s[0], s[1], s[2], s[4]))
def test_nt128(lib, cuda, ws, shape):
    run_cases(lib, cuda, ws, R.nt_cases(R.NT128, *shape))


def test_nt256_stream_k_strided(lib, cuda, ws):
    """The smallest of test_stream_k_follower_and_owner_items's candidates whose remainder round this device shares out by K range:
    follower and owner items with strided operands and guarded outputs, every epilogue instance."""
    pick = next((s for s in R.SK_CANDIDATES if R.check_plan(lib, R.nt_cases(R.NT256, *s, 0, "strided", sk=True)[0], 0, None, ws.numel()) is None), None)
    if pick is None:
        cus = torch.cuda.get_device_properties(cuda).multi_processor_count
        assert cus != 256, "no candidate shape splits on 256 CUs"
        pytest.skip(f"no candidate shape's remainder round is shared out on {cus} CUs")
    off = lib.hct_gemm_nt_flags_offset(ws.numel())
    flags = ws[off:off + 4096].view(torch.int32)
    flags.zero_()
    run_cases(lib, cuda, ws, R.nt_cases(R.NT256, *pick, 0, "strided", sk=True))
    assert int((flags[:256] != 0).sum()) > 0, "stream-K did not engage"
    assert int(flags[512]) == 0, "a partial never arrived"


@pytest.mark.parametrize("R_", R.TN_R)
@pytest.mark.parametrize("MN", R.TN_MN, ids=lambda s: f"{s[0]}x{s[1]}")
def test_tn(lib, cuda, ws, MN, R_):
    """64 NaN rows follow the last reduction row of A and of B: the zero-fill past `rend` has to be a zero-fill."""
    run_cases(lib, cuda, ws, R.tn_cases(*MN, R_), after_reduction=64)


@pytest.mark.parametrize("layout", R.GEN_LAYOUTS, ids=lambda s: "nt"[s[0]] + "nt"[s[1]])
@pytest.mark.parametrize("shape", R.GEN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_generic(lib, cuda, ws, shape, layout):
    run_cases(lib, cuda, ws, R.generic_cases(*shape, *layout), after_reduction=4)


def test_generic_takes_what_the_tuned_path_refuses(lib, cuda, ws):
    run_cases(lib, cuda, ws, R.fallback_cases())


def test_tn_group(lib, cuda):
    """One grouped launch of four wgrads with strided operands: jobs 0 and 1 read their A from the two column parts of ONE buffer
    (job 1's part is NaN below its 33 rows), every C is guarded, 64 NaN rows follow every reduction."""
    jobs = (GemmArgs * len(R.TN_GROUP_JOBS))()
    fails = []
    for gen in ("integers", "gaussian"):
        cases, datas, keep = [], [], []
        for i, (Rr, M, N) in enumerate(R.TN_GROUP_JOBS):
            cases.append(R.Case(name=f"tn_group-{Rr}x{M}x{N}", M=M, N=N, K=Rr, transA=1, transB=0, c_dtype=R.F32, alpha=(1.0, 0.5)[i % 2],
                                lda=M + 8, ldb=N + 24, ldc=N + 4, kernel=R.TN256))
            datas.append(R.make_data(cases[-1], gen))
        (R0, M0, _), (R1, M1, _) = R.TN_GROUP_JOBS[0], R.TN_GROUP_JOBS[1]
        shared = torch.full((R0, M0 + M1), NAN, dtype=torch.bfloat16)
        shared[:, :M0] = datas[0]["A"]
        shared[:R1, M0:] = datas[1]["A"]
        shared = R.guarded((R0, M0 + M1), M0 + M1 + 8, torch.bfloat16, fill=shared, after=64).to(cuda)
        runs = []
        for rep in range(2):
            outs = []
            for i, (case, d) in enumerate(zip(cases, datas)):
                a = jobs[i]
                a.M, a.N, a.K = case.M, case.N, case.K
                if i < 2:
                    a.A, a.lda = shared.ptr + (0 if i == 0 else 2 * M0), shared.ld
                else:
                    A = R.guarded(case.a_shape, case.lda, torch.bfloat16, fill=d["A"], after=64).to(cuda)
                    keep.append(A)
                    a.A, a.lda = A.ptr, case.lda
                B = R.guarded(case.b_shape, case.ldb, torch.bfloat16, fill=d["B"], after=64).to(cuda)
                keep.append(B)
                out = R.guarded((case.M, case.N), case.ldc, torch.float32).to(cuda)
                outs.append(out)
                a.a_dtype, a.transA, a.B, a.b_dtype, a.ldb, a.transB = R.BF16, 1, B.ptr, R.BF16, case.ldb, 0
                a.C, a.c_dtype, a.ldc, a.alpha = out.ptr, R.F32, case.ldc, case.alpha
            n = len(cases)
            nbytes = lib.hct_gemm_tn_group_workspace_bytes(n)
            gws = torch.empty(nbytes, dtype=torch.uint8, device=cuda)
            _lib.check(lib.hct_gemm_tn_group_prepare(C.cast(jobs, C.c_void_p), n, gws.data_ptr(), nbytes, _st()), "tn_group_prepare")
            _lib.check(lib.hct_gemm_tn_group_run(C.cast(jobs, C.c_void_p), n, gws.data_ptr(), nbytes, _st()), "tn_group_run")
            torch.cuda.synchronize()
            runs.append(outs)
        for case, d, o0, o1 in zip(cases, datas, *runs):
            if not torch.equal(_bits(o0.flat), _bits(o1.flat)):
                fails.append(f"{case.name}/{gen}: two launches differ")
            check_outputs(case, d, dict(C=o0), fails)
    assert not fails, "\n".join(fails[:40])


def test_refusals_touch_nothing(lib, cuda, ws):
    """Each must return non-zero and leave the NaN-filled outputs as they were."""
    nt = R.nt_cases(R.NT256, 65, 16, 128, 0, "strided")
    by = {c.name.rsplit("-", 1)[1]: c for c in nt}
    tn = R.tn_cases(48, 272, 1000)[0]
    rep = R.dataclasses.replace
    refusals = [
        ("DGELU without aux", rep(by["dgelu"], aux_dtype=-1), True),
        ("GELU_D without aux", rep(by["gelu_d"], aux_dtype=-1), True),
        ("MULAUX without aux", rep(by["mulaux_cs"], aux_dtype=-1, colsum=False), True),
        ("HCT_ACT_TANH", rep(by["plain_bf16"], act=R.TANH), True),
        ("unknown activation code", rep(by["plain_bf16"], act=17), True),
        ("colsum_out on a TN product", rep(tn, colsum=True), True),
        ("colsum_out with no workspace", by["mulaux_cs"], False),
        ("a split TN product with no workspace", tn, False),
        # the column-sum pass behind the generic kernel reads C four columns at a time; the call used to launch the product and fail after it
        ("colsum_out with N % 4 != 0", R.gen_case(77, 53, 45, 0, 1, R.F32, R.F32, "plain_f32", colsum=True), True),
        ("colsum_out with ldc % 4 != 0", R.gen_case(64, 64, 16, 0, 1, R.F32, R.F32, "scalar_ldc", colsum=True), True),
        ("colsum_out with C off its alignment", R.gen_case(64, 64, 16, 0, 1, R.F32, R.F32, "scalar_c_off", colsum=True), True),
    ]
    for what, case, with_ws in refusals:
        d = R.make_data(case, "integers")
        buf = Buffers(case, d, cuda)
        out = buf.fresh_outputs()
        a = buf.args(out)
        rc = lib.hct_gemm(C.byref(a), ws.data_ptr() if with_ws else None, ws.numel() if with_ws else 0, _st())
        torch.cuda.synchronize()
        assert rc != 0, what
        for name, g in out.items():
            assert bool(torch.isnan(g.flat).all()), f"{what}: {name} was written"
