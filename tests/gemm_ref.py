"""CPU-only reference, error bound, generators, guarded buffers and case tables for the GEMM tests (csrc/gemm.hip through
hct_gemm / hct_gemm_tn_group_*).  Imported by tests/test_gemm_ref_cpu.py (which pins this file to torch and to the plan) and
tests/test_gemm_kernels_gpu.py (which runs the kernels against it).  Nothing here touches a device.

exact(case, data)  the operation of include/headct_hip.h, act(alpha op(A) op(B) + bias) (+ residual), in float64 on the operands as
                   stored (bf16- or fp32-rounded), with C2, the written aux and colsum_out.
bound(case, data)  a per-element allowance |got - exact| <= bound, derived term by term (below), never tuned to a kernel.
make_data          two seeded generators: `integers` (every partial sum in any order is exact in fp32: the outputs must be
                   BIT-equal to exact) and `gaussian` (checked element by element against bound).
guarded            a [rows, width] view with row stride ld > width inside a larger NaN-filled allocation.

The bound, with u = 2^-24 (fp32 unit round-off), |A||B|^T the product of the absolute operands, mag = |alpha| |A||B|^T + |bias|:
  accumulation   bf16 products are exact in fp32; K of them summed in ANY order err <= gamma_K |A||B|^T, gamma_K ~ K u; doubled,
                 because the order inside an MFMA and across split-K / stream-K partials is unspecified:  |alpha| K 2^-23 |A||B|^T
                 (fp32 operands, generic kernel: each product is rounded once more: K + 1 in place of K)
  epilogue op    each fp32 multiply / add of the epilogue (alpha, bias, residual, the aux factor): 2^-23 |value|, value <= mag (+ |res|)
  store          bf16: 2^-8 |value| (8 significant bits, round to nearest: half a spacing of 2^-7 2^e on a value >= 2^e); fp32: nothing more
  GELU family    specialised NT256 epilogues (clamped-polynomial CDF): the project's bar of test_epilogue_gelu_accuracy_on_a_grid,
                 2e-4 absolute on gelu and on the stored gelu', |acc| 2e-4 on x gelu'(aux); runtime-flag epilogues (erff):
                 ERF_GELU_ALLOW / ERF_DGELU_ALLOW (4 x what torch's fp32 gelu / gelu' miss float64 by, measured in
                 tests/test_gemm_ref_cpu.py, per unit of max(1, |x|)); plus the Lipschitz constant times the pre-activation's bound
  column sums    sum over the rows of the elements' bounds + M 2^-23 sum |C| (fp32 sums in any order)
"""
import dataclasses
import functools
import math
import zlib

import torch

F32, BF16 = 0, 1                                              # HCT_F32, HCT_BF16
NONE, GELU, DGELU, TANH, GELU_D, MULAUX = 0, 1, 2, 3, 4, 5    # HCT_ACT_*
GENERIC, NT128, NT256, TN128, TN256 = 0, 1, 2, 3, 4           # HCT_GEMM_*
KERNEL_NAMES = {GENERIC: "generic", NT128: "nt128", NT256: "nt256", TN128: "tn128", TN256: "tn256"}

U23, U8 = 2.0 ** -23, 2.0 ** -8
FAST_GELU_ABS = 2e-4        # test_epilogue_gelu_accuracy_on_a_grid's bar for the polynomial CDF (gelu, gelu', and per unit of |acc|)
LIP_GELU, LIP_DGELU = 1.13, 0.80  # max |gelu'| = 1.1290 (x = sqrt 2), max |gelu''| = 2 phi(0) = 0.7979
# torch's fp32 F.gelu / its derivative against float64 over the pre-activations of the tables below, per unit of max(1, |x|): measured
# 3.5e-7 and 3.0e-7 (test_gemm_ref_cpu.py::test_erf_gelu_allowance_is_four_times_the_measured_error asserts that the constants are
# 4 x the figure it measures, to 10 %); the factor 4 covers a different erff / expf on the device.
ERF_GELU_ALLOW, ERF_DGELU_ALLOW = 1.4e-6, 1.2e-6


def torch_dtype(code):
    return torch.bfloat16 if code == BF16 else torch.float32


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    M: int
    N: int
    K: int
    transA: int = 0
    transB: int = 1
    a_dtype: int = BF16
    b_dtype: int = BF16
    c_dtype: int = BF16
    bias: bool = False
    residual: bool = False
    act: int = NONE
    aux_dtype: int = -1      # -1: no aux
    c2_dtype: int = -1       # -1: no C2
    alpha: float = 1.0
    colsum: bool = False
    lda: int = 0             # row strides in elements (0 = dense)
    ldb: int = 0
    ldc: int = 0
    ldr: int = 0
    ldaux: int = 0
    ldc2: int = 0
    a_off: int = 0           # first element of A / B / C past a 256-byte boundary, in elements
    b_off: int = 0
    c_off: int = 0
    hook: int = 0            # hct_debug_set_gemm_variant value for the call (0 auto, 128: the 128 x 128 kernels)
    force_generic: int = 0
    gens: tuple = ("integers", "gaussian")
    # what the plan must be on 256 CUs
    kernel: int = GENERIC
    mode: int = 0            # NT256 epilogue instance
    rows: int = 256          # NT256 tile height
    fuse: bool = False       # column sums from the epilogue
    split: object = None     # TN: True = splits > 1, False = splits == 1, None = not claimed
    sk: bool = False         # NT256: the remainder round is shared out by K range

    @property
    def a_shape(self):       # as stored
        return (self.K, self.M) if self.transA else (self.M, self.K)

    @property
    def b_shape(self):
        return (self.N, self.K) if self.transB else (self.K, self.N)

    @property
    def fast_gelu(self):     # the polynomial-CDF epilogues
        return self.kernel == NT256 and self.mode in (3, 4)

    @property
    def aux_written(self):
        return self.act in (GELU, GELU_D) and self.aux_dtype >= 0


# ---- generators ----------------------------------------------------------------------------------------------------------------------
def int_range(K):
    return 8 if K <= 320 else 4


# The 95 % of test_gemm_ref_cpu.py::test_bound_flags_planted_defects is a condition on the inputs: an output of 16 elements meets it
# only if ALL of them show the defect, and a dropped K slice cannot show through a gelu'(aux) factor that lies at its zero
# crossing, nor a zeroed element where gelu(x) is itself below its allowance (x < -4).  The one shape whose first draw holds such
# an element is drawn again with the salt given here; every other shape keeps its first draw.
SEED_SALT = {("gaussian", 1, 16, 320): 2}


@functools.lru_cache(maxsize=4)
def _shape_data(gen, M, N, K, transA, transB, a_dtype, b_dtype):
    key = (gen, M, N, K, transA, transB, a_dtype, b_dtype)
    g = torch.Generator(device="cpu").manual_seed(zlib.crc32(repr(key + ((SEED_SALT[key[:4]],) if key[:4] in SEED_SALT else ())).encode()))
    a_shape = (K, M) if transA else (M, K)
    b_shape = (N, K) if transB else (K, N)
    if gen == "integers":
        r = int_range(K)
        ri = lambda shape: torch.randint(-r, r + 1, shape, generator=g).float()
        nz = lambda shape: torch.randint(1, r + 1, shape, generator=g).float() * (2 * torch.randint(0, 2, shape, generator=g) - 1).float()
        A, B, bias, res, aux = nz(a_shape), nz(b_shape), ri((N,)), ri((M, N)), nz((M, N))  # (no zero factor: a K = 1 product must show)
    else:
        A, B = torch.randn(a_shape, generator=g), torch.randn(b_shape, generator=g) * 0.05
        bias, res, aux = torch.randn(N, generator=g), torch.randn(M, N, generator=g), torch.randn(M, N, generator=g)
    A, B = A.to(torch_dtype(a_dtype)), B.to(torch_dtype(b_dtype))
    aux = aux.bfloat16()  # (bf16-representable, so the same values serve an fp32 aux)
    A64 = (A.double().t() if transA else A.double())      # op(A) [M, K]
    B64 = (B.double() if transB else B.double().t())      # op(B)^T [N, K]
    d = dict(gen=gen, A=A, B=B, bias=bias, res=res, aux=aux, A64=A64, B64=B64)
    d["P"] = A64 @ B64.t()
    d["absP"] = A64.abs() @ B64.abs().t()
    return d


def make_data(case, gen):
    """Seeded by the shape, layout and operand dtypes only: the epilogue instances of one shape share operands and product."""
    return _shape_data(gen, case.M, case.N, case.K, case.transA, case.transB, case.a_dtype, case.b_dtype)


# ---- exact ---------------------------------------------------------------------------------------------------------------------------
def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x * math.sqrt(0.5)))


def dgelu64(x):
    return 0.5 * (1.0 + torch.erf(x * math.sqrt(0.5))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def stored(x64, dtype):
    """float64 -> the bits the kernel must store for an exactly representable-in-fp32 value (the integers generator)."""
    x = x64.float()
    return x.bfloat16() if dtype == BF16 else x


def _pick_row(case, v):
    """(row, neighbour) of the planted "row" defect: a position seeded by the case's name, moved on to the first row that differs
    from its neighbour (the next row; the last row's is the one before it) -- a row copied from an identical one is no defect.
    The place is drawn, not chosen where the defect shows best."""
    M = v.shape[0]
    nb = torch.arange(1, M + 1)
    nb[-1] = M - 2
    differs = (v != v[nb]).any(dim=1)
    r0 = zlib.crc32(("row" + case.name).encode()) % M
    r = next((r0 + k) % M for k in range(M) if differs[(r0 + k) % M])
    return r, int(nb[r])


def _pick_quad(case, v):
    """(row, first column) of the planted "quad" defect: an aligned quad at a position seeded by the case's name, moved on to the
    first quad that is not zero already (integer cases: a zeroed zero is no defect)."""
    nq = v.shape[1] // 4
    live = (v[:, :nq * 4].reshape(v.shape[0], nq, 4) != 0).any(dim=2).flatten()
    q0 = zlib.crc32(("quad" + case.name).encode()) % live.numel()
    q = next((q0 + k) % live.numel() for k in range(live.numel()) if live[(q0 + k) % live.numel()])
    return q // nq, 4 * (q % nq)


def exact(case, d, defect=None):
    """dict(C, C2, aux, colsum) in float64 (None where the case has none).  `defect` plants a wrong result for the tests of the
    bound: "kslice" drops one 32-deep slice of the reduction, "alpha" ignores alpha, "row" takes one row from its neighbour,
    "quad" zeroes four consecutive elements (both at a place seeded by the case's name, _pick_row / _pick_quad); "rows" and "zero"
    plant those two at every place at once, so that the share of flagged elements is taken over all rows and quads."""
    P, alpha = d["P"], case.alpha
    if defect == "kslice":
        k0 = (case.K // 2) // 32 * 32
        P = P - d["A64"][:, k0:k0 + 32] @ d["B64"][:, k0:k0 + 32].t()
    if defect == "alpha":
        alpha = 1.0
    pre = alpha * P
    if case.bias:
        pre = pre + d["bias"].double()
    aux_out = None
    if case.act == NONE:
        v = pre
    elif case.act in (GELU, GELU_D):
        v = gelu64(pre)
        if case.aux_dtype >= 0:
            aux_out = pre if case.act == GELU else dgelu64(pre)
    elif case.act == DGELU:
        v = pre * dgelu64(d["aux"].double())
    elif case.act == MULAUX:
        v = pre * d["aux"].double()
    else:
        raise ValueError(case.act)
    if case.residual:
        v = v + d["res"].double()
    if defect == "row":
        r, nb = _pick_row(case, v)
        v = v.clone()
        v[r] = v[nb]
    if defect == "quad":
        r, c = _pick_quad(case, v)
        v = v.clone()
        v[r, c:c + 4] = 0.0
    if defect == "rows":  # every row from its neighbour, "zero": every quad zeroed -- the share of flagged elements over ALL places
        nb = torch.arange(1, case.M + 1)
        nb[-1] = case.M - 2
        v = v[nb]
    if defect == "zero":
        v = torch.zeros_like(v)
    colsum = None
    if case.colsum:  # fused: of the unrounded values; separate pass: of C as stored
        colsum = (v if case.fuse else stored(v, case.c_dtype).double()).sum(0)
    return dict(C=v, C2=v if case.c2_dtype >= 0 else None, aux=aux_out, colsum=colsum)


def defect_region(case, d, defect):
    """Boolean [M, N] mask of the elements of C that the planted defect touches."""
    ex = exact(case, d)["C"]
    m = torch.zeros(case.M, case.N, dtype=torch.bool)
    if defect in ("kslice", "alpha", "rows", "zero"):
        m[:] = True
    elif defect == "row":
        m[_pick_row(case, ex)[0]] = True
    else:
        r, c = _pick_quad(case, ex)
        m[r, c:c + 4] = True
    return m


# ---- bound ---------------------------------------------------------------------------------------------------------------------------
def bound(case, d, ex=None):
    """Per-element allowance for |got - exact| of C, C2, the written aux and colsum_out (see the module docstring)."""
    ex = ex if ex is not None else exact(case, d)
    fp32_ops = case.a_dtype == F32 or case.b_dtype == F32
    a = abs(case.alpha)
    acc_err = a * (case.K + (1 if fp32_ops else 0)) * U23 * d["absP"]
    mag = a * d["absP"] + (d["bias"].double().abs() if case.bias else 0.0)
    pre_err = acc_err + U23 * mag * (1 + (1 if case.bias else 0))  # alpha, bias
    pre = case.alpha * d["P"] + (d["bias"].double() if case.bias else 0.0)
    gelu_abs = lambda x, erf_allow: FAST_GELU_ABS if case.fast_gelu else erf_allow * x.abs().clamp(min=1.0)
    aux_err = None
    if case.act == NONE:
        err, val = pre_err, mag
    elif case.act in (GELU, GELU_D):
        err = gelu_abs(pre, ERF_GELU_ALLOW) + LIP_GELU * pre_err
        val = gelu64(pre).abs() + err
        if case.aux_dtype >= 0:
            aux_err = pre_err if case.act == GELU else gelu_abs(pre, ERF_DGELU_ALLOW) + LIP_DGELU * pre_err
            aux_err = aux_err + (U8 * (ex["aux"].abs() + aux_err) if case.aux_dtype == BF16 else 0.0)
    elif case.act == DGELU:
        u = d["aux"].double()
        factor_err = FAST_GELU_ABS if case.fast_gelu else ERF_DGELU_ALLOW * u.abs().clamp(min=1.0)
        err = pre_err * LIP_GELU + (pre.abs() + pre_err) * factor_err + U23 * mag * LIP_GELU
        val = mag * LIP_GELU
    else:  # MULAUX
        u = d["aux"].double().abs()
        err = pre_err * u + U23 * mag * u
        val = mag * u
    if case.residual:
        val = val + d["res"].double().abs()
        err = err + U23 * val
    store = lambda dt: U8 * (ex["C"].abs() + err) if dt == BF16 else 0.0
    out = dict(C=err + store(case.c_dtype), C2=(err + store(case.c2_dtype)) if case.c2_dtype >= 0 else None, aux=aux_err, colsum=None)
    if case.colsum:
        per = err if case.fuse else out["C"]
        out["colsum"] = per.sum(0) + case.M * U23 * (ex["C"].abs() + per).sum(0)
    return out


def max_partial_sum(case, d):
    """Largest magnitude that any partial sum, in any order, of any output of an `integers` case can reach."""
    ex = exact(case, d)
    a = max(abs(case.alpha), 1.0)
    m = a * float(d["absP"].max()) + (float(d["bias"].abs().max()) if case.bias else 0.0)
    if case.act == MULAUX:
        m = m * float(d["aux"].double().abs().max())
    if case.residual:
        m = m + float(d["res"].abs().max())
    if case.colsum:
        m = max(m, float(ex["C"].abs().sum(0).max()) * 1.01)  # (bf16 rounding of the stored terms: < 2^-8 relative)
    return m


# ---- guarded buffers -----------------------------------------------------------------------------------------------------------------
class Guarded:
    """A [rows, width] view with row stride ld inside one flat NaN-filled allocation: `before` / `after` guard rows around it, the
    gap columns between the rows, and the view's first element `off` elements past a 256-byte boundary."""

    def __init__(self, flat, rows, width, ld, start):
        self.flat, self.rows, self.width, self.ld, self.start = flat, rows, width, ld, start

    @property
    def view(self):
        return torch.as_strided(self.flat, (self.rows, self.width), (self.ld, 1), self.start)

    @property
    def ptr(self):
        return self.flat.data_ptr() + self.start * self.flat.element_size()

    def to(self, device):
        return Guarded(self.flat.to(device), self.rows, self.width, self.ld, self.start)

    def outside_is_nan(self):
        f = self.flat.clone()
        torch.as_strided(f, (self.rows, self.width), (self.ld, 1), self.start).fill_(float("nan"))
        return bool(torch.isnan(f).all())


def guarded(shape, ld, dtype, fill=None, off=0, before=2, after=2):
    """fill = None: an output, NaN everywhere.  fill = a [rows, width] tensor: an input, NaN in the gaps and the guard rows."""
    rows, width = shape
    ld = ld or width
    assert ld >= width and before >= 2 and after >= 2
    start = (before * ld + 127) // 128 * 128 + off
    flat = torch.full((start + (rows + after) * ld + 128,), float("nan"), dtype=dtype)
    g = Guarded(flat, rows, width, ld, start)
    if fill is not None:
        g.view.copy_(fill)
    return g


# ---- case tables ---------------------------------------------------------------------------------------------------------------------
# NT epilogue instances: name -> (Case fields, NT256 epilogue instance, fused column sums on NT256).  Leading dimensions of the
# strided form: lda = K + 8, ldb = K + 16, ldc = N + 8, ldr = N + 4, ldaux = N + 8 (every one a multiple the tuned path accepts).
NT_INSTANCES = {
    "plain_bf16":   (dict(c_dtype=BF16), 1, False),                                                   # EPI_PLAIN_BF16
    "bias_res_f32": (dict(c_dtype=F32, bias=True, residual=True), 2, False),                          # EPI_RES_F32
    "gelu_aux":     (dict(act=GELU, bias=True, aux_dtype=BF16, gens=("gaussian",)), 3, False),        # EPI_GELU_BF16, aux = pre-activation
    "gelu_d":       (dict(act=GELU_D, bias=True, aux_dtype=BF16, gens=("gaussian",)), 3, False),      # EPI_GELU_BF16, aux = gelu'
    "dgelu":        (dict(act=DGELU, aux_dtype=BF16, gens=("gaussian",)), 4, False),                  # EPI_DGELU_BF16
    "dgelu_cs":     (dict(act=DGELU, aux_dtype=BF16, colsum=True, gens=("gaussian",)), 4, True),      # EPI_DGELU_CS: sums in the epilogue
    "mulaux_cs":    (dict(act=MULAUX, aux_dtype=BF16, colsum=True), 4, True),                         # EPI_DGELU_CS with a saved gelu'
    # the ways into EPI_GENERIC (runtime flags)
    "f32_bias":     (dict(c_dtype=F32, bias=True), 0, False),                                         # fp32 out without a residual
    "f32_c2_bf16":  (dict(c_dtype=F32, c2_dtype=BF16, bias=True, residual=True), 0, False),           # any C2
    "bf16_ldc4":    (dict(c_dtype=BF16, ldc=-4), 0, False),                                           # bf16 out, ldc % 8 == 4 (ldc = N + 4)
    "gelu_f32":     (dict(act=GELU, bias=True, c_dtype=F32, aux_dtype=F32, gens=("gaussian",)), 0, False),  # fp32 GELU, fp32 aux
    "gelu_res":     (dict(act=GELU, bias=True, residual=True, aux_dtype=BF16, gens=("gaussian",)), 0, False),  # residual after GELU
    "alpha_f32_cs": (dict(c_dtype=F32, alpha=-2.0, bias=True, colsum=True), 0, False),                # alpha != 1, column sums by the separate pass
    # alpha does not choose the instance (epilogue_mode never reads it): alpha = 0.5 on the plain bf16 one
    "alpha_bf16":   (dict(c_dtype=BF16, alpha=0.5), 1, False),
}
NT_M = (1, 65, 255, 257, 449)   # one row; a second 64-row wave; one short of a tile; one over; 192-row tiles: three, 65 rows in the last
NT_N = (16, 240, 272, 528)      # one 16-column stub; short of a tile; a tile + a 16-column stub; two tiles + a stub
NT256_K = (128, 320)            # two stage pairs (the shortest) and five (longer than the prefetch depth)
NT128_K = ((64, 0), (192, 128))  # K = 64 goes to the 128 x 128 kernel by itself; K = 192 only under hook 128


def _nt_case(kernel, M, N, K, inst, hook=0, form="strided", sk=False):
    f, mode, fuse = NT_INSTANCES[inst]
    f = dict(f)
    ldc = N + 4 if f.pop("ldc", 0) == -4 else N + 8
    if form == "lora":  # mae_plan.hip::lora_forward: the operand is the second half of [M, 2K] rows, C the second half of [M, 2N]
        ld = dict(lda=2 * K, a_off=K, ldb=K + 16, ldc=2 * N + (4 if ldc == N + 4 else 0), c_off=N, ldr=N + 4, ldaux=N + 8, ldc2=N + 24)
    else:
        ld = dict(lda=K + 8, ldb=K + 16, ldc=ldc, ldr=N + 4, ldaux=N + 8, ldc2=N + 24)
    # 192-row tiles: plain / +residual instances whose 256-row tiles fill less than a round while 192-row ones are more and still fit
    rows = 192 if kernel == NT256 and mode in (1, 2) and M in (255, 449) else 256
    return Case(name=f"{KERNEL_NAMES[kernel]}-{form}-{M}x{N}x{K}-{inst}", M=M, N=N, K=K, hook=hook, kernel=kernel,
                mode=mode if kernel == NT256 else 0, rows=rows, fuse=fuse and kernel == NT256, sk=sk, **ld, **f)


SK_CANDIDATES = ((2048, 256, 1024), (2048, 256, 1536), (2048, 256, 2048), (4096, 256, 3072))  # test_stream_k_follower_and_owner_items's list
SK_SHAPE_256_CUS = (2048, 256, 1536)  # the first of them whose remainder round the plan shares out on 256 CUs


def nt_shapes(kernel):
    """[(M, N, K, hook, form)]"""
    ks = [(K, 0) for K in NT256_K] if kernel == NT256 else list(NT128_K)
    out = [(M, N, K, hook, "strided") for M in NT_M for N in NT_N for K, hook in ks]
    out += [(M, 16, ks[-1][0], ks[-1][1], "lora") for M in (65, 257)]  # N = r = 16, operand and output column halves of wider rows
    return out


def nt_cases(kernel, M, N, K, hook, form, sk=False):
    return [_nt_case(kernel, M, N, K, inst, hook, form, sk) for inst in NT_INSTANCES]


# TN (wgrad): A [R, M], B [R, N]; lda = M + 8, ldb = N + 24, ldc = N + 4
TN_MN = ((16, 16), (48, 272), (256, 256), (272, 48))  # one MFMA tile; a stub + a tile and a stub; one full tile; the transpose of the second
TN_R = (1, 33, 128, 129, 200, 1000)  # one row; a ragged stage; TN256's smallest chunk exactly; one over; a ragged second chunk; split-K on both kernels
TN_VARIANTS = {  # name -> (fields, kernel)
    "tn256":        (dict(c_dtype=F32), TN256),
    "tn128_hook":   (dict(c_dtype=F32, hook=128), TN128),             # hook 128 keeps wgrads off the 256 x 256 kernel
    "tn128_bf16":   (dict(c_dtype=BF16), TN128),                      # a bf16 C
    "tn128_c2":     (dict(c_dtype=F32, c2_dtype=BF16), TN128),        # a C2 (with R = 1000: gemm_fold_kernel with a real epilogue)
    "tn256_halves": (dict(c_dtype=F32), TN256),                       # strided_wgrad: A and B are column halves of [R, 2M] / [R, 2N] rows
}


def tn_cases(M, N, R):
    out = []
    for i, (name, (f, kernel)) in enumerate(TN_VARIANTS.items()):
        f = dict(f)
        if name == "tn256_halves":
            ld = dict(lda=2 * M, a_off=M, ldb=2 * N, b_off=N, ldc=N + 4)
        else:
            ld = dict(lda=M + 8, ldb=N + 24, ldc=N + 4 if f["c_dtype"] == F32 else N + 8, ldc2=N + 8)
        if kernel == TN256:   # a chunk is ceil(R / 256 workgroups per tile) rounded up to 64, at least 128 rows
            split = R > 128
        else:                 # 64-row steps, at most steps / 4 pieces
            split = R >= 512
        out.append(Case(name=f"{name}-{R}x{M}x{N}", M=M, N=N, K=R, transA=1, transB=0, alpha=(1.0, 0.5)[(i + R) % 2], kernel=kernel,
                        split=split, **ld, **f))
    return out


TN_GROUP_JOBS = ((130, 48, 64), (33, 16, 16), (257, 768, 16), (1000, 272, 528))  # (R, M, N); alphas 1, 0.5, 1, 0.5

# generic kernel: all four layouts x the four operand dtype pairs x these shapes
GEN_SHAPES = ((1, 1, 1), (64, 64, 16), (65, 67, 17), (77, 53, 45))  # one element; one full tile and K step; tile + 1, K tail of 1; the old test's
GEN_LAYOUTS = ((0, 0), (0, 1), (1, 0), (1, 1))
GEN_DTYPES = ((F32, F32), (BF16, F32), (F32, BF16), (BF16, BF16))
GEN_INSTANCES = {  # every one with strides; scalar epilogue (epilogue1) where N % 4 != 0 or as the entry says
    "plain_f32":     dict(c_dtype=F32),                                                       # vector epilogue where N % 4 == 0
    "scalar_ldc":    dict(c_dtype=F32, bias=True, residual=True, ldc=-1),                     # ldc % 4 != 0 -> scalar epilogue
    "scalar_c_off":  dict(c_dtype=BF16, bias=True, residual=True, c_off=1),                   # C one element off its alignment -> scalar
    "gelu_aux":      dict(act=GELU, bias=True, c_dtype=F32, aux_dtype=F32, gens=("gaussian",)),
    "gelu_d_res":    dict(act=GELU_D, bias=True, residual=True, c_dtype=F32, aux_dtype=BF16, gens=("gaussian",)),
    "dgelu":         dict(act=DGELU, c_dtype=F32, aux_dtype=F32, gens=("gaussian",)),
    "mulaux_cs":     dict(act=MULAUX, c_dtype=BF16, aux_dtype=BF16, colsum=True),             # column sums by the separate pass
    "c2_alpha":      dict(c_dtype=F32, c2_dtype=BF16, alpha=0.5, bias=True, colsum=True),
    "scalar_c2":     dict(c_dtype=F32, c2_dtype=F32, alpha=-2.0, residual=True, ldc=-1),      # scalar epilogue with a C2 and a residual
}


def gen_case(M, N, K, tA, tB, da, db, inst, tag="generic", **over):
    f = dict(GEN_INSTANCES[inst])
    f.update(over)
    aw = M if tA else K
    bw = K if tB else N
    ldc = N + 3 if f.pop("ldc", 0) == -1 else N + 4
    while (N + 4 - ldc) and ldc % 4 == 0:
        ldc += 1  # (the scalar form: keep ldc % 4 != 0)
    ld = dict(lda=f.pop("lda", aw + 4), ldb=bw + 8, ldc=ldc, ldr=N + 4, ldaux=N + 8, ldc2=N + 12)
    if N % 4 and "colsum" not in over:
        f["colsum"] = False  # (the separate pass reads four columns at a time: hct_gemm refuses colsum_out there, see the refusals)
    return Case(name=f"{tag}-{'nt'[tA]}{'nt'[tB]}-{('f32', 'bf16')[da]}x{('f32', 'bf16')[db]}-{M}x{N}x{K}-{inst}", M=M, N=N, K=K, transA=tA,
                transB=tB, a_dtype=da, b_dtype=db, kernel=GENERIC, **ld, **f)


def generic_cases(M, N, K, tA, tB):
    return [gen_case(M, N, K, tA, tB, da, db, inst) for da, db in GEN_DTYPES for inst in GEN_INSTANCES]


def fallback_cases():
    """bf16 NT products that the tuned path refuses and the generic kernel must take."""
    M, N, K = 65, 32, 128
    return [
        gen_case(M, 24, K, 0, 1, BF16, BF16, "scalar_ldc", tag="fallback-N24", lda=K + 8),             # N % 16 != 0
        gen_case(M, N, 96, 0, 1, BF16, BF16, "c2_alpha", tag="fallback-K96", lda=96 + 8),               # K % 64 != 0
        gen_case(M, N, K, 0, 1, BF16, BF16, "mulaux_cs", tag="fallback-lda4", lda=K + 4),     # lda % 8 == 4
        gen_case(M, N, K, 0, 1, BF16, BF16, "plain_f32", tag="fallback-Aoff", lda=K + 8, a_off=4),  # A 8 bytes off a 16-byte boundary
    ]


def all_hct_gemm_cases():
    out = []
    for kernel in (NT256, NT128):
        for s in nt_shapes(kernel):
            out += nt_cases(kernel, *s)
    out += nt_cases(NT256, *SK_SHAPE_256_CUS, 0, "strided", sk=True)
    for M, N in TN_MN:
        for R in TN_R:
            out += tn_cases(M, N, R)
    for M, N, K in GEN_SHAPES:
        for tA, tB in GEN_LAYOUTS:
            out += generic_cases(M, N, K, tA, tB)
    return out + fallback_cases()


# ---- the plan (hct_gemm_describe: host arithmetic, no device) ---------------------------------------------------------------------------
def _args_for_plan(case):
    from headct_foundation_amd._lib import GemmArgs
    a = GemmArgs()
    a.M, a.N, a.K = case.M, case.N, case.K
    esz = lambda dt: 2 if dt == BF16 else 4
    base = 1 << 20  # any 256-byte aligned address: the plan reads alignments, never memory
    a.A, a.a_dtype, a.lda, a.transA = base + case.a_off * esz(case.a_dtype), case.a_dtype, case.lda, case.transA
    a.B, a.b_dtype, a.ldb, a.transB = base + case.b_off * esz(case.b_dtype), case.b_dtype, case.ldb, case.transB
    a.C, a.c_dtype, a.ldc = base + case.c_off * esz(case.c_dtype), case.c_dtype, case.ldc
    a.bias = base if case.bias else None
    a.residual, a.ldr = (base if case.residual else None), case.ldr
    a.act, a.alpha, a.force_generic = case.act, case.alpha, case.force_generic
    if case.aux_dtype >= 0:
        a.aux, a.aux_dtype, a.ldaux = base, case.aux_dtype, case.ldaux
    if case.c2_dtype >= 0:
        a.C2, a.c2_dtype, a.ldc2 = base, case.c2_dtype, case.ldc2
    a.colsum_out = base if case.colsum else None
    return a


def check_plan(lib, case, num_cus, args=None, workspace_bytes=-1):
    """None if hct_gemm_describe plans what the case claims, else the text of the first difference.  `args`: the hct_gemm_args of
    the call itself (default: stand-in pointers with the case's alignments); workspace_bytes: what the call passes (-1: as much
    as the plan asks for)."""
    import ctypes as C
    from headct_foundation_amd._lib import GemmPlanInfo
    info = GemmPlanInfo()
    a = args if args is not None else _args_for_plan(case)
    lib.hct_debug_set_gemm_variant(case.hook)
    try:
        assert lib.hct_gemm_describe(C.byref(a), num_cus, C.c_size_t(workspace_bytes).value, C.byref(info)) == 0
    finally:
        lib.hct_debug_set_gemm_variant(0)
    if info.kernel != case.kernel:
        return f"kernel {info.kernel}, not {case.kernel}"
    if case.kernel == NT256:
        if info.epilogue_mode != case.mode or bool(info.fuse_colsum) != case.fuse:
            return f"epilogue instance {info.epilogue_mode} (fused sums {info.fuse_colsum}), not {case.mode} ({case.fuse})"
        if 64 * info.row_tiles_per_wave != case.rows:
            return f"cu-dependent: {64 * info.row_tiles_per_wave}-row tiles, not {case.rows}"
        if (info.sk_tiles > 0) != case.sk:
            return f"cu-dependent: sk_tiles {info.sk_tiles}, sharing expected: {case.sk}"
    if case.split is not None and (info.splits > 1) != case.split:
        return f"splits {info.splits}, split expected: {case.split}"
    return None


# ---- where an element lives (failure reports) ------------------------------------------------------------------------------------------
def locate(case, row, col):
    """(tile row, tile column), (wave row, wave column) of an output element in the kernel the case plans."""
    if case.kernel in (NT256, TN256):  # 8 waves = 4 (M) x 2 (N): wm = wave >> 1, wn = wave & 1, each 64 (192-row tiles: 48) rows x 128 columns
        th = case.rows
        return (row // th, col // 256), ((row % th) // (th // 4), (col % 256) // 128)
    if case.kernel in (NT128, TN128):  # 4 waves = 2 x 2 (wr = wave >> 1, wc = wave & 1), each 64 x 64
        return (row // 128, col // 128), ((row % 128) // 64, (col % 128) // 64)
    return (row // 64, col // 64), ((row % 64) // 16, 0)  # generic: 64 x 64 tiles, thread (ty, tx) holds 4 x 4, wave = ty >> 2 = 16 rows


def worst(got64, want64, allow):
    """(ratio, row, col) of the largest |got - want| / allow; a non-finite `got` counts as infinitely wrong."""
    err = (got64 - want64).abs()
    ratio = err / torch.as_tensor(allow, dtype=torch.float64).expand_as(err).clamp(min=1e-300)
    ratio = torch.where(torch.isfinite(got64), ratio, torch.full_like(ratio, float("inf")))
    ratio = torch.where((err == 0) & torch.isfinite(got64), torch.zeros_like(ratio), ratio)
    i = int(ratio.argmax())
    w = ratio.shape[-1]
    return float(ratio.flatten()[i]), i // w, i % w
