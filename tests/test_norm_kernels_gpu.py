"""The LayerNorm and RMSNorm kernels of csrc/elementwise.hip (one template family: norm_fwd[_reg]_kernel, norm_bwd_kernel) through
the C ABI, one entry point at a time (hct_layernorm_fwd / _bwd / _bwd_mapped, hct_rmsnorm_fwd / _bwd / _bwd_mapped and their *_workspace_bytes), against the restatements of tests/norm_ref.py evaluated
in float64.  One family table serves both norms.

Row counts are crossed with a small D, D limits with few rows (N.ROW_LIMITS, N.D_LIMITS: every loop limit of the kernels with a case on
each side; tests/test_norm_ref_cpu.py asserts that).  Every output sits NaN-filled between guard bands that must come back untouched;
an output that is not asked for stays untouched; every input matrix has NaN rows behind its last row, so a partial that reads one row
too far turns a column sum NaN; the workspace is exactly *_workspace_bytes long with a guard behind it; every call is made twice and the
two results are bit-identical.  Error is taken per row: y, dx and the shadow as relative L2 (the shadow is also the rounded dx, bit for
bit), rstd relative, mean over the row's mean |x|; the worst row holds the project's bars (fp32 1e-5, stored bf16 4e-3, rstd 1e-6) or,
for the (family, kind, eps, figure) listed in N.RESTATEMENT, ten times what fp32 arithmetic in the kernels' order costs on the CPU.
dgamma and dbeta are within (n + roundings) 2^-24 sum|terms| of the float64 sum per column, the column sum of dx within
(n - 1) 2^-24 sum|dx| of the float64 sum of the very dx that the kernel stored; on the integer inputs all of them, and dx, are bit-equal."""
import pytest
import torch

from headct_foundation_amd import _lib
from tests import norm_ref as N
from tests.test_assembly_kernels_gpu import _Out, _bits, _check_sum, _code, _p, _st, _twice

pytestmark = pytest.mark.gpu

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
GUARD_ROWS = 4     # NaN rows behind every input matrix: one per wave of the workgroup that holds the last row
WS_GUARD = 256     # bytes behind the workspace
WS_FILL = 0xA5
FAMILY_TABLE = {   # family: (forward, backward, mapped backward, workspace size, figures of the forward, column sums of the backward)
    "layernorm": ("hct_layernorm_fwd", "hct_layernorm_bwd", "hct_layernorm_bwd_mapped", "hct_layernorm_bwd_workspace_bytes",
                  ("y", "mean", "rstd"), ("dgamma", "dbeta")),
    "rmsnorm": ("hct_rmsnorm_fwd", "hct_rmsnorm_bwd", "hct_rmsnorm_bwd_mapped", "hct_rmsnorm_bwd_workspace_bytes", ("y", "rstd"), ("dgamma",)),
}


def _in(t, dev, dtype=None):
    """An input [rows, ...] with GUARD_ROWS rows of NaN (a row map: of a huge index) behind it; None stays None."""
    if t is None:
        return None
    t = t.to(dtype or t.dtype)
    buf = torch.full((t.shape[0] + GUARD_ROWS,) + tuple(t.shape[1:]), float("nan") if t.dtype.is_floating_point else 2 ** 30, dtype=t.dtype)
    buf[:t.shape[0]] = t
    return buf.to(dev)


class _Ws:
    """A workspace of exactly `nbytes` with WS_GUARD bytes behind it."""

    def __init__(self, nbytes, dev):
        self.nbytes = int(nbytes)
        self.buf = torch.full((self.nbytes + WS_GUARD,), WS_FILL, dtype=torch.uint8, device=dev)
        self.ptr = self.buf.data_ptr()

    def check(self):
        assert bool((self.buf[self.nbytes:] == WS_FILL).all()), "the guard behind the workspace was written"


def _bar(key, name, stored):
    return N.bar(key + (name,), N.BF16_BAR if stored == BF16 else N.FP32_BAR)


# ---- forward --------------------------------------------------------------------------------------------------------------------------
def _fwd_call(lib, family, d, rows, D, eps, ydt, dev):
    outs = dict(y=_Out((rows, D), ydt, dev), rstd=_Out((rows,), F32, dev))
    if family == "layernorm":
        outs["mean"] = _Out((rows,), F32, dev)
        rc = lib.hct_layernorm_fwd(_p(d["x"]), _p(d["gamma"]), _p(d["beta"]), rows, D, eps, outs["y"].ptr, _code(ydt), outs["mean"].ptr,
                                   outs["rstd"].ptr, _st())
    else:
        rc = lib.hct_rmsnorm_fwd(_p(d["x"]), _p(d["gamma"]), rows, D, eps, outs["y"].ptr, _code(ydt), outs["rstd"].ptr, _st())
    return rc, outs


def _forward(lib, dev, family, rows, D, kinds):
    for kind in kinds:
        for eps in N.EPS_VALUES:
            inp, ref = N.fwd_case(family, rows, D, kind, eps)
            d = dict(x=_in(inp["x"], dev), gamma=inp["gamma"].to(dev), beta=inp["beta"].to(dev))
            key = (family, kind, eps)
            for ydt in (F32, BF16):
                def run():
                    rc, outs = _fwd_call(lib, family, d, rows, D, eps, ydt, dev)
                    _lib.check(rc, FAMILY_TABLE[family][0])
                    return outs
                got = _twice(run)
                assert set(got) == set(FAMILY_TABLE[family][4])
                if kind == "int":  # the row sum of integers is exact, and so is its division by a power of two
                    assert not any(bool(torch.isnan(v.float()).any()) for v in got.values())
                    if family == "layernorm" and D & (D - 1) == 0:
                        assert torch.equal(got["mean"].double(), ref["mean"]), (key, rows, D)
                    continue
                fig = N.fwd_figures(got, ref, inp["x"])
                bars = dict(y=_bar(key, "y", ydt), rstd=N.RSTD_BAR, mean=_bar(key, "mean", F32))
                print(key, rows, D, str(ydt)[6:], {k: f"{e:.2e} / {bars[k]:.1e}" for k, e in fig.items()})
                for k, e in fig.items():
                    assert e < bars[k], (key, rows, D, ydt, k, e, bars[k])


@pytest.mark.parametrize("rows", N.ROW_LIMITS)
@pytest.mark.parametrize("D", N.ROW_LIMIT_D)
@pytest.mark.parametrize("family", N.FAMILIES)
def test_forward_row_limits(lib, cuda, family, D, rows):
    """One workgroup with idle waves ... FWD_WAVES waves and the row loop's second and third trip (N.ROW_LIMITS)."""
    _forward(lib, cuda, family, rows, D, ("gauss",))


@pytest.mark.parametrize("D", N.D_LIMITS + N.D_FWD_ONLY)
@pytest.mark.parametrize("family", N.FAMILIES)
def test_forward_d_limits(lib, cuda, family, D):
    """Every NV with its last chunk short by a quad, full, one quad over; beyond 1024 the multi-pass kernels.  Every input kind, both eps."""
    for rows in N.D_LIMIT_ROWS:
        _forward(lib, cuda, family, rows, D, N.KINDS + ("int",))


# ---- backward -------------------------------------------------------------------------------------------------------------------------
def _bwd_device(inp, dev):
    """The inputs of a backward on the device, NaN rows behind each matrix and behind mean / rstd."""
    d = {k: _in(inp[k], dev) for k in ("dy", "x", "rstd_in", "rows_map")}
    d["mean_in"] = _in(inp.get("mean_in"), dev)
    d["gamma"] = inp["gamma"].to(dev)
    d["dres"] = _in(inp["dres"], dev)
    return d


def _bwd_call(lib, family, d, rows, D, var, ws, dev, mapped=None, nbytes=None):
    """One backward call; every output is allocated, the ones `var` does not ask for are not handed in."""
    fwd, plain, via_map, _, _, sums = FAMILY_TABLE[family]
    outs = dict(dx=_Out((rows, D), F32, dev), shadow=_Out((rows, D), var["shdt"] or BF16, dev), dcolsum=_Out((D,), F32, dev))
    outs.update({k: _Out((D,), F32, dev) for k in sums})
    dres = _p(d["dres"])
    if var["dres"] == "alias":
        outs["dx"].t.copy_(d["dres"][:rows])
        dres = outs["dx"].ptr
    mapped = d["rows_map"] is not None if mapped is None else mapped
    head = (_p(d["dy"]), _code(d["dy"].dtype), _p(d["x"])) + ((_p(d["mean_in"]),) if family == "layernorm" else ()) + (_p(d["rstd_in"]), _p(d["gamma"]), dres)
    head += (_p(d["rows_map"]),) if mapped else ()
    tail = (rows, D, outs["dx"].ptr, outs["shadow"].ptr if var["shdt"] else None, _code(var["shdt"]) if var["shdt"] else 0)
    tail += tuple(outs[k].ptr for k in sums) + (outs["dcolsum"].ptr if var["colsum"] else None, ws.ptr, ws.nbytes if nbytes is None else nbytes, _st())
    return getattr(lib, via_map if mapped else plain)(*(head + tail)), outs


def _hold_bwd(family, key, kind, inp, var, got, rows):
    """The figures of one backward call against float64 (see the head of this file)."""
    ref = N.bwd_ref(family, inp)
    what = (key, rows, inp["x"].shape[1], {k: str(v)[6:] if isinstance(v, torch.dtype) else v for k, v in var.items()})
    assert not bool(torch.isnan(got["dx"]).any()), what
    if kind == "int":
        assert torch.equal(got["dx"].double(), ref["dx"]), (what, "dx of integer inputs is not exact")
    else:
        e, b = N.worst_row(got["dx"], ref["dx"]), _bar(key, "dx", F32)
        print(what, f"dx {e:.2e} / {b:.1e}")
        assert e < b, (what, "dx", e, b)
    if var["shdt"]:
        assert torch.equal(_bits(got["shadow"]), _bits(got["dx"].to(var["shdt"]))), (what, "the shadow is not dx in its storage type")
        assert N.worst_row(got["shadow"], ref["dx"]) < _bar(key, "dx", var["shdt"]), (what, "shadow")
    else:
        assert bool(torch.isnan(got["shadow"].float()).all()), (what, "a shadow that was not asked for was written")
    for name, (roundings, mag) in N.sum_terms(family, inp).items():
        _check_sum(got[name], ref[name], torch.tensor(float(rows + roundings + (1 if roundings else 0))), mag, kind, f"{what} {name}")
    if not var["colsum"]:
        assert bool(torch.isnan(got["dcolsum"]).all()), (what, "a column sum that was not asked for was written")
    elif kind == "int":
        assert torch.equal(got["dcolsum"].double(), ref["dcolsum"]), (what, "dcolsum of integer inputs is not exact")
    else:  # against the dx that the kernel itself stored and added up; dx is held above
        mine = got["dx"].double()
        _check_sum(got["dcolsum"], mine.sum(0), torch.tensor(float(rows)), mine.abs().sum(0), kind, f"{what} dcolsum")


def _backward(lib, dev, family, rows, D, plan, ws):
    for kind, eps, var in plan:
        inp = N.bwd_case(family, rows, D, kind, eps, var)
        d = _bwd_device(inp, dev)

        def run():
            rc, outs = _bwd_call(lib, family, d, rows, D, var, ws, dev)
            _lib.check(rc, FAMILY_TABLE[family][1])
            return outs
        got = _twice(run)
        ws.check()
        _hold_bwd(family, (family, kind, eps), kind, inp, var, got, rows)


def _workspace(lib, family, rows, D, dev):
    nbytes = getattr(lib, FAMILY_TABLE[family][3])(rows, D)
    assert nbytes == N.BWD_WAVES // N.ROWS_PER_WG * 3 * D * 4  # partial[block][3][D] fp32 for both norms (RMSNorm uses two planes)
    return _Ws(nbytes, dev)


@pytest.mark.parametrize("rows", N.ROW_LIMITS)
@pytest.mark.parametrize("D", N.ROW_LIMIT_D)
@pytest.mark.parametrize("family", N.FAMILIES)
def test_backward_row_limits(lib, cuda, family, D, rows):
    """One workgroup ... the fold's 16 row groups and its second trip ... BWD_WAVES waves and up to a fifth trip of the row loop.  Normal
    inputs to their bars and bounds, integer inputs bit-equal; the call variants take turns over the row counts."""
    i = N.ROW_LIMITS.index(rows)
    variants = [N.VARIANTS[i % len(N.VARIANTS)], N.VARIANTS[(i + 3) % len(N.VARIANTS)]]
    _backward(lib, cuda, family, rows, D, N.bwd_plan(("gauss", "int"), variants), _workspace(lib, family, rows, D, cuda))


@pytest.mark.parametrize("D", N.D_LIMITS)
@pytest.mark.parametrize("family", N.FAMILIES)
def test_backward_d_limits(lib, cuda, family, D):
    """Every NV with its last chunk short by a quad, full, one quad over: every input kind with every call variant."""
    ws = _workspace(lib, family, max(N.D_LIMIT_ROWS), D, cuda)
    for rows in N.D_LIMIT_ROWS:
        _backward(lib, cuda, family, rows, D, N.bwd_plan(N.KINDS + ("int",)), ws)


@pytest.mark.parametrize("D", N.INT_MEAN_D)
@pytest.mark.parametrize("family", N.FAMILIES)
def test_backward_exact_with_row_means(lib, cuda, family, D):
    """Integer inputs whose mean_d(a) and mean_d(a xhat) are non-zero multiples of 1 / D: still bit-equal, in every call variant."""
    rows = N.BASE_ROWS
    ws = _workspace(lib, family, rows, D, cuda)
    for var in N.VARIANTS:
        inp = N.int_case(family, rows, D, means=True)
        inp["dy"] = inp["dy"].to(var["dydt"])
        full = inp.pop("dres")
        inp["dres"], inp["rows_map"] = (full if var["dres"] else None), None
        if var["dres"] == "mapped":
            inp["rows_map"], mc = N.row_map(rows)
            sel = inp["rows_map"] >= 0
            inp["dres"] = torch.zeros(mc, D)
            inp["dres"][inp["rows_map"][sel].long()] = full[sel]
        d = _bwd_device(inp, cuda)

        def run():
            rc, outs = _bwd_call(lib, family, d, rows, D, var, ws, cuda)
            _lib.check(rc, FAMILY_TABLE[family][1])
            return outs
        got = _twice(run)
        ws.check()
        _hold_bwd(family, (family, "int", 0.0), "int", inp, var, got, rows)


@pytest.mark.parametrize("rows", N.MAPPED_ROWS)
@pytest.mark.parametrize("family", N.FAMILIES)
def test_mapped_equals_plain_on_the_scattered_matrix(lib, cuda, family, rows):
    """The residual gradient read from a compact matrix through a row map with -1 entries == the plain call on the zero-filled full matrix,
    bit for bit, past the fold's first trip (516 rows) and past the backward's wave count (4097)."""
    D = 260
    var = dict(dydt=BF16, shdt=BF16, dres="mapped", colsum=True)
    inp = N.bwd_case(family, rows, D, "gauss", 1e-6, var)
    ws = _workspace(lib, family, rows, D, cuda)
    sel = inp["rows_map"] >= 0
    full = torch.zeros(rows, D)
    full[sel] = inp["dres"][inp["rows_map"][sel].long()]
    d = _bwd_device(inp, cuda)
    d_plain = dict(d, dres=_in(full, cuda), rows_map=None)
    res = []
    for dd in (d, d_plain):
        def run():
            rc, outs = _bwd_call(lib, family, dd, rows, D, var, ws, cuda)
            _lib.check(rc, FAMILY_TABLE[family][1])
            return outs
        res.append(_twice(run))
        ws.check()
    for k in res[0]:
        assert torch.equal(_bits(res[0][k]), _bits(res[1][k])), k
    _hold_bwd(family, (family, "gauss", 1e-6), "gauss", inp, var, res[0], rows)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_layernorm_refusals(lib, cuda):
    """D % 4 != 0 forward and backward, D = 1280 backward (the multi-pass forward has no backward), a short workspace, a mapped residual
    gradient that aliases dx: refused before anything is launched, nothing written."""
    rows = 5
    var = dict(dydt=F32, shdt=F32, dres="own", colsum=True)
    inp = N.bwd_case("layernorm", rows, 1280, "gauss", 1e-5, var)
    d = _bwd_device(inp, cuda)
    d["beta"] = inp["beta"].to(cuda)
    ws = _workspace(lib, "layernorm", rows, 1280, cuda)

    def refused(rc, outs, word, kept=()):
        torch.cuda.synchronize()
        assert rc != 0 and word in lib.hct_last_error_string().decode(), (word, rc, lib.hct_last_error_string())
        for k, o in outs.items():
            o.result()
            assert k in kept or o.untouched(), (word, k)
        ws.check()
    for ydt in (F32, BF16):
        refused(*_fwd_call(lib, "layernorm", d, rows, 1278, 1e-5, ydt, cuda), "hct_layernorm_fwd")
    for v in (var, dict(var, dydt=BF16, shdt=BF16)):
        dd = dict(d, dy=d["dy"].to(v["dydt"]))
        refused(*_bwd_call(lib, "layernorm", dd, rows, 1278, v, ws, cuda), "hct_layernorm_bwd")
        refused(*_bwd_call(lib, "layernorm", dd, rows, 1280, v, ws, cuda), "1024")
        refused(*_bwd_call(lib, "layernorm", dd, rows, 768, v, ws, cuda, nbytes=lib.hct_layernorm_bwd_workspace_bytes(rows, 768) - 1), "workspace")
    m = dict(d, rows_map=_in(N.row_map(rows)[0], cuda))
    rc, outs = _bwd_call(lib, "layernorm", m, rows, 1280, dict(var, dres="alias"), ws, cuda)  # dx holds the residual gradient it aliases
    refused(rc, outs, "alias", kept=("dx",))
    assert torch.equal(_bits(outs["dx"].result()), _bits(inp["dres"]))
