"""Yardstick of the LayerNorm / RMSNorm kernels (csrc/elementwise.hip: norm_fwd[_reg]_kernel, norm_bwd_kernel, one template each for
both families, and fold_partials_kernel): plain torch restatements of the definitions in include/headct_hip.h, every output included.  The
arithmetic runs in `dt` (the tests ask for float64).  With `order=True` every reduction is taken in the kernels' own order -- the
4-column lane sums over chunks of 256 and the 64-lane butterfly (head_kernels_ref.sum_wave), rows w, w + W, ... per wave, the four
waves of a workgroup (0 + 1) + (2 + 3), the fold's 16 row groups and its 16-term tail: in fp32 that shows what fp32 arithmetic alone
costs, which tests/test_norm_ref_cpu.py measures and holds against the bars of tests/test_norm_kernels_gpu.py.  The second half builds
the inputs and the case lists of both files.  Nothing here calls the code under test."""
import functools

import torch

from tests.assembly_ref import U32, gen, sum_bound  # noqa: F401  (re-exported for the two test files)
from tests.head_kernels_ref import BF16_BAR, FP32_BAR, product_sum_bound, sum_wave, worst_col, worst_row  # noqa: F401

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
RSTD_BAR = 1e-6        # test_rmsnorm_kernels_vs_fp64_autograd's bar for the saved statistic

# ---- loop limits of the kernels (tests/test_norm_ref_cpu.py reads them back out of csrc/elementwise.hip) ------------------------------
CHUNK_COLS = 256       # `lane * 4 + 256 * i`: 64 lanes x 4 columns per chunk of a row, in every kernel of the family
MAX_NV = 4             # `else if (D <= 1024) HCT_NORM_FWD(4)` / `case 4:` of launch_norm_bwd: chunks held in registers; beyond: the
#                        multi-pass forward (norm_fwd_kernel), no backward
ROWS_PER_WG = 4        # 256 threads = 4 waves, one row per wave and trip: `(rows + 3) / 4` workgroups
FWD_WAVES = 2048 * 4   # `min((rows + 3) / 4, kNormFwdBlocks)`, kNormFwdBlocks = 2048, in norm_fwd: waves that stride over the rows
BWD_WAVES = 1024 * 4   # `kNormBwdBlocks = 1024`: the same for both families, and the number of partial blocks at most
FOLD_GROUPS = 16       # fold_partials_kernel: `rg = threadIdx.x >> 5` of kFoldThreads = 512
FOLD_IN_FLIGHT = 8     # ... `float v[8]`: loads per thread and trip
FOLD_TRIP = FOLD_GROUPS * FOLD_IN_FLIGHT   # `b0 += 16 * 8`: partial blocks per trip
FOLD_COLS = 32         # ... `c = threadIdx.x & 31`, `(D + 31) / 32` workgroups: columns per fold group

EPS_VALUES = (1e-5, 1e-6)   # nn.LayerNorm's default (the MAE) and the ViT path's ln.eps / every RMSNorm
FAMILIES = ("layernorm", "rmsnorm")
KINDS = ("gauss", "offset", "outlier", "tiny", "const")
CLEAN_KINDS = ("gauss", "outlier", "tiny")   # no RESTATEMENT entry may name one of these


# ---- reductions --------------------------------------------------------------------------------------------------------------------
def sum_rows_waves(t, order=False, waves=BWD_WAVES):
    """Column sums of t [rows, D] as a backward and its fold take them: wave w of W = 4 min(waves / 4, ceil(rows / 4)) adds rows w, w + W,
    ... in order; a workgroup adds its waves (0 + 1) + (2 + 3) into one partial block; fold group rg adds blocks rg, rg + 16, ... in
    order (eight per trip, which does not change the order); the tail adds the 16 groups in order, starting from zero."""
    if not order:
        return t.sum(0)
    rows, D = t.shape
    nblk = min(waves // ROWS_PER_WG, -(-rows // ROWS_PER_WG))
    nw = nblk * ROWS_PER_WG
    tt = torch.cat((t, t.new_zeros(-rows % nw, D))).reshape(-1, nw, D)  # adding +0 is exact
    acc = torch.zeros_like(tt[0])
    for trip in range(tt.shape[0]):
        acc = acc + tt[trip]
    w = acc.reshape(nblk, ROWS_PER_WG, D)
    part = (w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3])
    pp = torch.cat((part, part.new_zeros(-nblk % FOLD_GROUPS, D))).reshape(-1, FOLD_GROUPS, D)
    acc = torch.zeros_like(pp[0])
    for k in range(pp.shape[0]):
        acc = acc + pp[k]
    v = torch.zeros_like(acc[0])
    for i in range(FOLD_GROUPS):
        v = v + acc[i]
    return v


def _scalar(v, dt):
    return torch.tensor(v, dtype=F32).to(dt)  # a c_float argument as it arrives in the kernel


# ---- the four operations -------------------------------------------------------------------------------------------------------------
def layernorm_fwd(x, gamma, beta, eps, dt=F64, order=False):
    """y = (x - mean) rstd gamma + beta, mean = mean_d(x), rstd = 1 / sqrt(mean_d((x - mean)^2) + eps): two passes, as the kernel."""
    x, gamma, beta = x.to(dt), gamma.to(dt), beta.to(dt)
    D = x.shape[-1]
    mean = sum_wave(x, order) / D
    c = x - mean[:, None]
    rstd = 1.0 / (sum_wave(c * c, order) / D + _scalar(eps, dt)).sqrt()
    return dict(y=c * rstd[:, None] * gamma + beta, mean=mean, rstd=rstd)


def rmsnorm_fwd(x, gamma, eps, dt=F64, order=False):
    """y = x rstd gamma, rstd = 1 / sqrt(mean_d(x^2) + eps)."""
    x, gamma = x.to(dt), gamma.to(dt)
    rstd = 1.0 / (sum_wave(x * x, order) / x.shape[-1] + _scalar(eps, dt)).sqrt()
    return dict(y=x * rstd[:, None] * gamma, rstd=rstd)


def _residual(v, dres, rows_map, dt):
    if dres is None:
        return v
    if rows_map is None:
        return v + dres.to(dt)
    sel = rows_map >= 0
    add = torch.zeros_like(v)
    add[sel] = dres.to(dt)[rows_map[sel].long()]
    return v + add


def layernorm_bwd(dy, x, mean, rstd, gamma, dres=None, rows_map=None, dt=F64, order=False):
    """xhat = (x - mean) rstd, a = dy gamma:  dx = rstd (a - mean_d(a) - xhat mean_d(a xhat)) + dres[rows_map] (nothing where the map
    says -1; no map: row by row);  dgamma = sum_r dy xhat, dbeta = sum_r dy, dcolsum = sum_r dx.  mean and rstd are INPUTS."""
    dy, x, mean, rstd, gamma = (t.to(dt) for t in (dy, x, mean, rstd, gamma))
    D = x.shape[-1]
    xh = (x - mean[:, None]) * rstd[:, None]
    a = dy * gamma
    s1, s2 = sum_wave(a, order) / D, sum_wave(a * xh, order) / D
    v = _residual((a - s1[:, None] - xh * s2[:, None]) * rstd[:, None], dres, rows_map, dt)
    return dict(dx=v, dgamma=sum_rows_waves(dy * xh, order), dbeta=sum_rows_waves(dy, order), dcolsum=sum_rows_waves(v, order))


def rmsnorm_bwd(dy, x, rstd, gamma, dres=None, rows_map=None, dt=F64, order=False):
    """xhat = x rstd, a = dy gamma:  dx = rstd (a - xhat mean_d(a xhat)) + dres[rows_map];  dgamma = sum_r dy xhat, dcolsum = sum_r dx."""
    dy, x, rstd, gamma = (t.to(dt) for t in (dy, x, rstd, gamma))
    xh = x * rstd[:, None]
    a = dy * gamma
    s2 = sum_wave(a * xh, order) / x.shape[-1]
    v = _residual((a - xh * s2[:, None]) * rstd[:, None], dres, rows_map, dt)
    return dict(dx=v, dgamma=sum_rows_waves(dy * xh, order), dcolsum=sum_rows_waves(v, order))


def fwd(family, inp, eps, dt=F64, order=False):
    if family == "layernorm":
        return layernorm_fwd(inp["x"], inp["gamma"], inp["beta"], eps, dt, order)
    return rmsnorm_fwd(inp["x"], inp["gamma"], eps, dt, order)


def bwd(family, inp, dres=None, rows_map=None, dt=F64, order=False):
    """The backward of `inp` (dy, x, mean_in, rstd_in, gamma) with the residual gradient handed in."""
    if family == "layernorm":
        return layernorm_bwd(inp["dy"], inp["x"], inp["mean_in"], inp["rstd_in"], inp["gamma"], dres, rows_map, dt, order)
    return rmsnorm_bwd(inp["dy"], inp["x"], inp["rstd_in"], inp["gamma"], dres, rows_map, dt, order)


# ---- error measures and bars ---------------------------------------------------------------------------------------------------------
def fwd_figures(got, ref, x):
    """y: the worst row's relative L2; rstd: the worst row's relative error; mean: the worst row's absolute error over that row's
    mean |x| (on `gauss` the mean itself is near zero, relative to it the error is noise)."""
    out = dict(y=worst_row(got["y"], ref["y"]), rstd=worst_col(got["rstd"], ref["rstd"]))
    if "mean" in ref:
        out["mean"] = worst_col(got["mean"], ref["mean"], x.double().abs().mean(1))
    return out


# measured: the worst error of the order=True restatement in fp32 against float64 over every case of that (family, kind, eps, figure)
# that the GPU file walks, listed where it exceeds a tenth of the project bar of fp32 arithmetic (FP32_BAR; rstd: RSTD_BAR).
# tests/test_norm_ref_cpu.py asserts each entry against the measurement: not below it, not above twice it, and none for a clean kind.
# The GPU bar of such a figure is TEN times the entry where that is wider than the project bar: fp32 arithmetic in the kernel's own
# order cannot be held tighter.
RESTATEMENT = {
    ("layernorm", "offset", 1e-5, "y"): 7.2e-4,   # mean / std = 1000: x - mean loses three digits, in any order
    ("layernorm", "offset", 1e-6, "y"): 7.2e-4,
    ("layernorm", "const", 1e-5, "y"): 1.6e-3,    # y - beta is the rounding of the mean times rstd = 1 / sqrt(eps) = 316 ...
    ("layernorm", "const", 1e-6, "y"): 5.1e-3,    # ... = 1000
}
# rstd is the one figure that the rule above does not reach: 1 / sqrt(sum / D + eps) takes a rounded sum, a division, an addition, a
# square root and a reciprocal (LayerNorm: on rounded differences from a rounded mean), each a rounding of 2^-24 = 0.6e-7: the worst of
# thousands of rows measures 1.1e-7 to 2.7e-7 on every kind, whatever the inputs.  That is past a tenth of RSTD_BAR and within a third
# of it.  rstd therefore takes RSTD_BAR as it is, never widened, has no entry here, and the CPU test holds the restatement's rstd to
# RSTD_CEILING (five roundings) instead of a tenth.
RSTD_CEILING = 5 * U32


def bar(key, default):
    """The bar of one figure: the project bar, or ten times the restatement's recorded error where that is wider."""
    return max(default, 10.0 * RESTATEMENT[key]) if key in RESTATEMENT else default


# =================================================================================================================================
# Cases and inputs of tests/test_norm_kernels_gpu.py.  Everything is made on the CPU from seeded generators.
# =================================================================================================================================
ROW_LIMIT_D = (48, 260)      # one chunk with idle lanes; a second chunk of one quad (NV = 2)
ROW_LIMITS = (1, 3, 4, 5,                    # one workgroup, ragged
              60, 64, 68,                    # 15, 16, 17 partial blocks: the fold's 16 row groups
              508, 512, 516,                 # 127, 128, 129 blocks: the fold's second trip
              4092, 4096, 4097, 4101,        # BWD_WAVES: a second row trip for one wave and for five
              8191, 8192, 8193, 8197,        # FWD_WAVES: the same for the forward
              16387)                         # a third trip forward, a fifth backward
D_LIMIT_ROWS = (1, 5, 9, 517)
D_LIMITS = (4, 8, 252, 256, 260, 508, 512, 516, 764, 768, 772, 1020, 1024)   # each NV: last chunk short by a quad, full, one quad over
D_FWD_ONLY = (1028, 1280, 2052)              # the multi-pass forward: a fifth chunk of one quad, a whole fifth, a ninth of one quad
INT_MEAN_D = (256, 512, 1024)                # the exact-sum variant with non-zero row means
MAPPED_ROWS = (516, 4097)
BASE_ROWS = 517                              # the inputs of a (D, kind) are the leading rows of ONE matrix of this many rows, or
LONG_ROWS = ROW_LIMITS[-1]                   # ... of this many for the kinds that the row limits use at ROW_LIMIT_D
OUTLIER = 1.0e3

# storage and argument combinations of a backward call: dy x shadow in all four combinations and no shadow; the residual gradient absent,
# in place (dres == dx), in its own buffer, compact through a row map; with and without the column sum
VARIANTS = (
    dict(dydt=F32, shdt=F32, dres="alias", colsum=True),
    dict(dydt=BF16, shdt=BF16, dres="own", colsum=True),
    dict(dydt=F32, shdt=BF16, dres=None, colsum=False),
    dict(dydt=BF16, shdt=F32, dres="mapped", colsum=True),
    dict(dydt=BF16, shdt=None, dres="own", colsum=False),
    dict(dydt=F32, shdt=None, dres=None, colsum=True),
)


def base_rows(D, kind):
    return LONG_ROWS if D in ROW_LIMIT_D and kind in ("gauss", "int") else BASE_ROWS


@functools.lru_cache(maxsize=24)
def _base(D, kind):
    """x, gamma, beta, dy, dres of one (D, kind), base_rows(D, kind) rows.  "gauss": 2 randn + 0.3 (test_layernorm_fwd_bwd's); "offset":
    mean 100, std 0.1; "outlier": unit normal with column D // 3 at 1e3; "tiny": 1e-4 randn (variance below both eps); "const": every
    element of a row equal; "int": integers in [-4, 4] (the forward's: the row sum is exact)."""
    rows = base_rows(D, kind)
    g = gen(D, KINDS.index(kind) if kind in KINDS else 7, 41)
    x = torch.randn(rows, D, generator=g)
    if kind == "gauss":
        x = x * 2 + 0.3
    elif kind == "offset":
        x = 100.0 + 0.1 * x
    elif kind == "outlier":
        x[:, D // 3] = OUTLIER
    elif kind == "tiny":
        x = 1e-4 * x
    elif kind == "const":
        x = (x[:, :1] * 2 + 0.3).expand(rows, D).contiguous()
    elif kind == "int":
        x = torch.randint(-4, 5, (rows, D), generator=g).float()
    gamma, beta = 1 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    dy, dres = torch.randn(rows, D, generator=g), torch.randn(rows, D, generator=g)
    return dict(x=x, gamma=gamma, beta=beta, dy=_conditioned(dy, x, gamma) if D <= SMALL_D else dy, dres=dres)


SMALL_D = 8


def _conditioned(dy, x, gamma):
    """At D = 4 the LayerNorm backward takes a = dy gamma off the span of (1, xhat) and keeps what is left of it in two dimensions: among
    517 random rows some keep a few per cent, and their relative error measures that cancellation (1e-6 to 2e-6 in fp32 in any order),
    not the kernel.  So at D <= SMALL_D every row of dy gets its own remainder's direction added at the length of a: the remainder is
    then at least half of a, for RMSNorm (which takes a off xhat alone) as well."""
    g, D = gamma.double(), x.shape[1]
    a = dy.double() * g
    c = x.double() - x.double().mean(1, keepdim=True)
    cn = c / c.norm(dim=1, keepdim=True).clamp(min=1e-300)  # "const": zero
    r = a - a.mean(1, keepdim=True)
    r = r - (r * cn).sum(1, keepdim=True) * cn
    return ((a + r / r.norm(dim=1, keepdim=True) * a.norm(dim=1, keepdim=True)) / g).float()


@functools.lru_cache(maxsize=24)
def _base_fwd(family, D, kind, eps):
    """The float64 forward of the whole base matrix: rows are independent, so any leading part of it is that part's reference."""
    return fwd(family, _base(D, kind), eps)


def fwd_case(family, rows, D, kind, eps):
    """(inputs, float64 reference) of the leading `rows` rows."""
    assert rows <= base_rows(D, kind)
    inp = {k: (v[:rows] if v.dim() == 2 else v) for k, v in _base(D, kind).items()}
    return inp, {k: v[:rows] for k, v in _base_fwd(family, D, kind, eps).items()}


def row_map(rows, seed=0):
    """(map [rows] int32, compact row count): about half the rows, in shuffled order, have a row of the compact matrix; the others -1."""
    g = gen(rows, seed, 43)
    mc = (rows + 1) // 2
    sel = torch.randperm(rows, generator=g)[:mc]
    m = torch.full((rows,), -1, dtype=torch.int32)
    m[sel] = torch.arange(mc, dtype=torch.int32)
    return m, mc


def bwd_case(family, rows, D, kind, eps, var):
    """Inputs of one backward call: dy rounded to its storage type, mean_in / rstd_in the float64 forward's rounded to fp32 (the
    backward is held on its own: they are inputs), the residual gradient in the form `var` asks for (dres [rows, D] or compact
    [mc, D] with rows_map)."""
    if kind == "int":
        inp = int_case(family, rows, D)
    else:
        inp, ref = fwd_case(family, rows, D, kind, eps)
        inp["rstd_in"] = ref["rstd"].float()
        if family == "layernorm":
            inp["mean_in"] = ref["mean"].float()
    inp["dy"] = inp["dy"].to(var["dydt"])
    full = inp.pop("dres")
    inp["dres"] = inp["rows_map"] = None
    if var["dres"] == "mapped":
        inp["rows_map"], mc = row_map(rows)
        comp = torch.zeros(mc, D)
        sel = inp["rows_map"] >= 0
        comp[inp["rows_map"][sel].long()] = full[sel]
        inp["dres"] = comp
    elif var["dres"] is not None:
        inp["dres"] = full
    return inp


def bwd_ref(family, inp, dt=F64, order=False):
    return bwd(family, inp, inp["dres"], inp["rows_map"], dt, order)


@functools.lru_cache(maxsize=8)
def _int_base(D, means):
    """Exact sums.  mean = 0 and rstd = 1 are handed in, so xhat = x.  Each quad holds a = dy gamma = (p, -p, q, -q) and
    xhat = (u, u, w, w) with gamma a power of two per column pair: mean_d(a) and mean_d(a xhat) are exactly 0 for any D, dx = a + dres,
    and every figure is an integer below 2^24 at LONG_ROWS rows (|a| <= 16, |dy xhat| <= 16, |dres| <= 4).
    `means`: D a power of two, arbitrary integer dy and x, gamma in {1, 2}, for LayerNorm an integer mean per row: mean_d(a) and
    mean_d(a xhat) are integers over D, every figure a multiple of 1 / D small enough to be exact (test_norm_ref_cpu.py asserts it)."""
    rows = BASE_ROWS if means else base_rows(D, "int")
    g = gen(D, means, 47)
    ri = lambda lo, hi, *shape: torch.randint(lo, hi, shape, generator=g).float()
    if means:
        assert D & (D - 1) == 0
        mean = ri(-2, 3, rows)
        return dict(x=ri(-4, 5, rows, D) + mean[:, None], dy=ri(-4, 5, rows, D), gamma=2.0 ** ri(0, 2, D), dres=ri(-4, 5, rows, D),
                    mean_in=mean, rstd_in=torch.ones(rows))
    pair = lambda t: torch.stack((t[..., 0], t[..., 0], t[..., 1], t[..., 1]), -1).reshape(*t.shape[:-2], D)
    sign = torch.tensor([1.0, -1.0, 1.0, -1.0]).repeat(D // 4)
    return dict(x=pair(ri(-4, 5, rows, D // 4, 2)), dy=pair(ri(-4, 5, rows, D // 4, 2)) * sign, gamma=pair(2.0 ** ri(0, 3, D // 4, 2)),
                dres=ri(-4, 5, rows, D), mean_in=torch.zeros(rows), rstd_in=torch.ones(rows))


def int_case(family, rows, D, means=False):
    base = _int_base(D, means)
    inp = {k: (v[:rows] if v.shape[0] == base["x"].shape[0] and k != "gamma" else v) for k, v in base.items()}
    inp["gamma"] = base["gamma"]
    if family == "rmsnorm":  # no mean: xhat = x rstd
        inp["x"] = inp["x"] - inp["mean_in"][:, None]
        inp["mean_in"] = None
    return inp


def fwd_ds():
    return tuple(sorted(set(ROW_LIMIT_D + D_LIMITS + D_FWD_ONLY)))


def bwd_ds():
    return tuple(sorted(set(ROW_LIMIT_D + D_LIMITS)))


def bwd_plan(kinds, variants=None):
    """(kind, eps, variant) of one backward test: every kind with every variant (or with the one given per kind), eps alternating."""
    for i, kind in enumerate(kinds):
        for var in (VARIANTS if variants is None else [variants[i]]):
            yield kind, EPS_VALUES[(i + VARIANTS.index(var)) % 2], var


def measure(family):
    """{(family, kind, eps, figure): the worst error of the fp32 restatement in the kernels' order against float64} over every
    (D, kind) base matrix -- whose leading rows are all that the GPU file ever hands to a kernel -- with both eps, and for the backward
    with dy in both storage types, with and without a residual gradient (a mapped one adds the same rows' values or nothing)."""
    worst = {}

    def note(kind, eps, name, e):
        k = (family, kind, eps, name)
        worst[k] = max(worst.get(k, 0.0), e)
    for kind in KINDS:
        for eps in EPS_VALUES:
            for D in fwd_ds():
                inp, ref = fwd_case(family, base_rows(D, kind), D, kind, eps)
                for name, e in fwd_figures(fwd(family, inp, eps, F32, True), ref, inp["x"]).items():
                    note(kind, eps, name, e)
            for D in bwd_ds():
                for dydt in (F32, BF16):
                    for dres in (None, "own"):
                        inp = bwd_case(family, base_rows(D, kind), D, kind, eps, dict(dydt=dydt, dres=dres))
                        note(kind, eps, "dx", worst_row(bwd_ref(family, inp, F32, True)["dx"], bwd_ref(family, inp)["dx"]))
    return worst


def sum_terms(family, inp):
    """{figure: (roundings, sum_r |term|)} of the column sums whose terms are inputs or rounded products of inputs: dbeta adds dy as it
    is; a term of dgamma is dy xhat with xhat = (x - mean) rstd (RMSNorm: x rstd) formed in fp32: 3 (2) roundings."""
    dy, x, rstd = inp["dy"].double(), inp["x"].double(), inp["rstd_in"].double()
    if family == "layernorm":
        xh = (x - inp["mean_in"].double()[:, None]) * rstd[:, None]
        return dict(dgamma=(3, (dy * xh).abs().sum(0)), dbeta=(0, dy.abs().sum(0)))
    return dict(dgamma=(2, (dy * x * rstd[:, None]).abs().sum(0)))
