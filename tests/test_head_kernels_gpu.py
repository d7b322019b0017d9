"""The DINO loss, projection-head and classifier-head kernels of csrc/dino.hip, csrc/heads.hip and csrc/finetune.hip through the C ABI,
one entry point at a time, against the plain restatements of tests/head_kernels_ref.py evaluated in float64.

Every output is pre-filled with NaN inside a buffer with a guard band on each side that must come back untouched, and every call is
made twice: the two results must agree bit for bit.  Error is taken per row (per column for column statistics) and the worst row must
hold the bar.  Copies, single additions and multiplications and the centre update are held bit-equal; sums are bit-equal on
integer-valued inputs and within (n - 1) 2^-24 sum|terms| otherwise (sums of rounded products: H.product_sum_bound); everything
composite takes the project's bars (fp32 1e-5, stored bf16 4e-3; the DINO loss 2e-5, its gradient 1e-4 / 6e-3), or, for the cases
listed in H.RESTATEMENT, ten times the error that fp32 arithmetic in the kernel's own order has on the CPU.  The sizes are the ones at
which each kernel's loop is taken a second time or ends raggedly; tests/test_head_kernels_ref_cpu.py asserts that they are.

Of the classifier heads this file holds the linear one's training kernels (batch statistics, hct_bn_norm, hct_bn_bwd_input, the
cross-entropy, the clip).  The attentive head's (hct_query_attention / _lse / _bwd, hct_head_linear / _x / _bwd / _wgrad,
hct_channel_norm) and the copy passes around them are in tests/test_attn_head_kernels_gpu.py."""
import pytest
import torch

from headct_foundation_amd import _lib
from headct_foundation_amd._lib import HCT_F32
from tests import head_kernels_ref as H
from tests.test_assembly_kernels_gpu import _Out, _bits, _check_sum, _code, _p, _st, _twice

pytestmark = pytest.mark.gpu

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
HCT_E_WORKSPACE = -3
EPS = H.EPS


def _dev(inp, dev, *names):
    return {k: inp[k].contiguous().to(dev) for k in names}


def _inout(src, dev):
    """An in / out argument: `src` inside a guarded buffer."""
    o = _Out(tuple(src.shape), src.dtype, dev)
    o.t.copy_(src)
    return o


def _ws(nbytes, dev):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=dev)


def _hold(key, inp, var, got, ref, spec):
    """Every "row" / "col" figure of `got` within its bar, every "sum" figure within its bound (exact on integer inputs)."""
    fig = H.errors(key, inp, var, got, ref, spec)
    print(key, {k[-1]: f"{e:.2e} / {b:.1e}" for k, (e, b, _) in fig.items()})
    for k, (e, b, _) in fig.items():
        assert e < b, (k, e, b)
    for name, (how, roundings) in spec.items():
        if how == "sum" and name in got:
            n, _ = H.sum_limits(inp, name, roundings)
            _check_sum(got[name], ref[name], n + (roundings + 1 if roundings else 0), inp["sum_terms"][name][1], var["kind"], f"{key} {name}")


def _refused(rc, outs, lib, name):
    torch.cuda.synchronize()
    assert rc != 0 and name in lib.hct_last_error_string().decode(), (name, rc)
    for o in outs.values():
        o.result()
        assert o.untouched(), name


# ---- hct_l2norm_rows_fwd / _bwd ---------------------------------------------------------------------------------------------------
# one wave per row, four rows per block: M = 1, 5, 9 leave three waves of the last block idle
# lane loop, 64 lanes x 4 columns per trip: n = 4 one lane, 252 all but one, 256 one whole trip, 260 a second trip by lane 0, 1028 five
def _l2_call(lib, d, M, n, zdt, dev, rows=None):
    rows = M if rows is None else rows
    outs = dict(zn=_Out((rows, n), zdt, dev), inv_norm=_Out((rows,), F32, dev), dz=_Out((rows, n), F32, dev))
    rc = lib.hct_l2norm_rows_fwd(d["z"].data_ptr(), M, n, outs["zn"].ptr, _code(zdt), outs["inv_norm"].ptr, _st())
    rc2 = lib.hct_l2norm_rows_bwd(d["dzn"].data_ptr(), d["zn_in"].data_ptr(), _code(zdt), d["inv_in"].data_ptr(), M, n, outs["dz"].ptr, _st())
    return rc, rc2, outs


@pytest.mark.parametrize("M,n", H.L2_CASES)
def test_l2norm_rows(lib, cuda, M, n):
    for key, inp, var in H.l2_runs(M, n):
        d = _dev(inp, cuda, "z", "dzn", "zn_in", "inv_in")

        def run():
            rc, rc2, outs = _l2_call(lib, d, M, n, var["zdt"], cuda)
            _lib.check(rc, "hct_l2norm_rows_fwd")
            _lib.check(rc2, "hct_l2norm_rows_bwd")
            return outs
        got = _twice(run)
        _hold(key, inp, var, got, H.l2_ref(inp, var), H.l2_spec(var))
        if M > H.L2_ZERO_ROW:  # the all-zero row: zn = 0, the norm clamped at 1e-12
            assert bool((got["zn"][H.L2_ZERO_ROW] == 0).all()) and float(got["inv_norm"][H.L2_ZERO_ROW]) == float(torch.tensor(1e12, dtype=F32))


def test_l2norm_rows_empty_and_refused(lib, cuda):
    """M = 0 returns 0 and writes nothing; n = 6 (not a multiple of 4) is refused before anything is launched."""
    inp = next(iter(H.l2_runs(5, 8)))[1]
    d = _dev(inp, cuda, "z", "dzn", "zn_in", "inv_in")
    rc, rc2, outs = _l2_call(lib, d, 0, 8, F32, cuda, rows=5)
    torch.cuda.synchronize()
    assert rc == 0 and rc2 == 0 and all(o.untouched() for o in outs.values())
    for o in outs.values():
        o.result()
    for zdt in (F32, BF16):
        rc, rc2, outs = _l2_call(lib, d, 5, 6, zdt, cuda, rows=5)  # 5 x 6 <= the 5 x 8 elements every buffer holds
        assert rc2 != 0
        _refused(rc, outs, lib, "hct_l2norm_rows")


# ---- hct_weight_norm_fwd / _bwd ---------------------------------------------------------------------------------------------------
# the same wave-per-row shape: K = 3 one block with an idle wave, 6 a second block, 65 seventeen blocks with one row in the last
@pytest.mark.parametrize("K,n", H.WN_CASES)
def test_weight_norm(lib, cuda, K, n):
    for key, inp, var in H.wn_runs(K, n):
        d = _dev(inp, cuda, "v", "g", "dw", "inv_in")
        wdt = var["wdt"]

        def run(with_dg=True):
            outs = dict(w=_Out((K, n), wdt, cuda), inv_norm=_Out((K,), F32, cuda), dv=_Out((K, n), F32, cuda))
            if with_dg:
                outs["dg"] = _Out((K,), F32, cuda)
            _lib.check(lib.hct_weight_norm_fwd(d["v"].data_ptr(), d["g"].data_ptr(), K, n, outs["w"].ptr, _code(wdt), outs["inv_norm"].ptr, _st()),
                       "hct_weight_norm_fwd")
            _lib.check(lib.hct_weight_norm_bwd(d["dw"].data_ptr(), d["v"].data_ptr(), d["g"].data_ptr(), d["inv_in"].data_ptr(), K, n, outs["dv"].ptr,
                                               _p(outs.get("dg")), _st()), "hct_weight_norm_bwd")
            return outs
        got = _twice(run)
        _hold(key, inp, var, got, H.wn_ref(inp, var), H.wn_spec(var))
        if wdt == F32:  # dg NULL: dv is what it was
            assert torch.equal(_bits(_twice(lambda: run(False))["dv"]), _bits(got["dv"]))


# ---- hct_bn_gelu_fwd / _bwd_sums / _bwd_apply -----------------------------------------------------------------------------------
# fwd / apply: a quad per thread, 256 per block: M D / 4 = 2 (254 idle threads) ... 33667 = 131.5 blocks; the column of a quad is (4 i) % D
# sums: one thread per column, rows in index order: D = 260 and 1028 need a second (fifth) block, whose last one is ragged
@pytest.mark.parametrize("M,D", H.BNG_CASES)
def test_bn_gelu(lib, cuda, M, D):
    for key, inp, var in H.bng_runs(M, D):
        d = _dev(inp, cuda, "u", "mean", "var", "gamma", "beta", "dh", "xhat", "dact", "sums_in")
        hdt, dudt, count = var["hdt"], var["dudt"], var["count"]

        def run(aux=True):
            outs = dict(h=_Out((M, D), hdt, cuda))
            if aux:
                outs.update(xhat=_Out((M, D), F32, cuda), dact=_Out((M, D), F32, cuda), sums=_Out((2, D), F32, cuda), du=_Out((M, D), dudt, cuda))
            _lib.check(lib.hct_bn_gelu_fwd(d["u"].data_ptr(), d["mean"].data_ptr(), d["var"].data_ptr(), d["gamma"].data_ptr(), d["beta"].data_ptr(), EPS,
                                           M, D, outs["h"].ptr, _code(hdt), _p(outs.get("xhat")), _p(outs.get("dact")), _st()), "hct_bn_gelu_fwd")
            if aux:
                _lib.check(lib.hct_bn_gelu_bwd_sums(d["dh"].data_ptr(), _code(hdt), d["dact"].data_ptr(), d["xhat"].data_ptr(), M, D, outs["sums"].ptr, _st()),
                           "hct_bn_gelu_bwd_sums")
                _lib.check(lib.hct_bn_gelu_bwd_apply(d["dh"].data_ptr(), _code(hdt), d["dact"].data_ptr(), d["xhat"].data_ptr(), d["gamma"].data_ptr(),
                                                     d["var"].data_ptr(), EPS, d["sums_in"].data_ptr(), float(count), M, D, outs["du"].ptr, _code(dudt), _st()),
                           "hct_bn_gelu_bwd_apply")
            return outs
        got = _twice(run)
        _hold(key, inp, var, got, H.bng_ref(inp, var), H.bng_spec(var))
        if (M, D) == H.BNG_NULL_CASE:  # xhat and dact NULL (evaluation): h is what it was
            assert torch.equal(_bits(_twice(lambda: run(False))["h"]), _bits(got["h"]))


# ---- hct_batchnorm_stats / hct_bn_stats_rows ---------------------------------------------------------------------------------------
# one thread per column: D = 1, 255, 257 (a second block of one thread); batch_stats_kernel takes all rows in one pass,
# bn_stats_chunk_kernel 128 per block: rows = 128 one full chunk, 129 a chunk of ONE row (its M2 is 0), 257 two folds, 300 a ragged third
def _stats_outs(inp, D, dev, running):
    outs = dict(mean=_Out((D,), F32, dev), var=_Out((D,), F32, dev))
    if running:
        outs.update(running_mean=_inout(inp["rmean"], dev), running_var=_inout(inp["rvar"], dev))
    return outs


def _batch_stats(lib, x_d, rows, D, outs):
    return lib.hct_batchnorm_stats(x_d.data_ptr(), rows, D, 0.1, outs["mean"].ptr, outs["var"].ptr, _p(outs.get("running_mean")),
                                   _p(outs.get("running_var")), _st())


def _stats_rows(lib, x_d, xdt, ldx, rows, D, outs, ws, short=0):
    return lib.hct_bn_stats_rows(x_d.data_ptr(), _code(xdt), ldx, rows, D, 0.1, outs["mean"].ptr, outs["var"].ptr, _p(outs.get("running_mean")),
                                 _p(outs.get("running_var")), ws.data_ptr(), lib.hct_bn_rows_workspace_bytes(rows, D) - short, _st())


def _hold_stats(key, inp, var, got, single_chunk):
    _hold(key, inp, var, got, H.stats_ref(inp, var), H.stats_spec(var))
    if var["kind"] == "int" and single_chunk:  # an exact sum and one division
        assert torch.equal(got["mean"], inp["x"].double().mean(0).float()), key


@pytest.mark.parametrize("B,D", [(B, D) for B in H.STATS_B for D in H.STATS_D])
def test_batchnorm_stats(lib, cuda, B, D):
    for key, inp, var in H.stats_runs(B, D):
        x_d = inp["x"].to(cuda)

        def run(running=True):
            outs = _stats_outs(inp, D, cuda, running)
            _lib.check(_batch_stats(lib, x_d, B, D, outs), "hct_batchnorm_stats")
            return outs
        got = _twice(run)
        _hold_stats(key, inp, var, got, True)
        bare = _twice(lambda: run(False))  # running statistics NULL: mean and variance are what they were
        assert all(torch.equal(_bits(bare[k]), _bits(got[k])) for k in ("mean", "var"))


@pytest.mark.parametrize("rows,D", [(r, D) for r in H.STATS_ROWS for D in H.STATS_D])
def test_bn_stats_rows(lib, cuda, rows, D):
    ws = _ws(lib.hct_bn_rows_workspace_bytes(rows, D), cuda)
    assert lib.hct_bn_rows_workspace_bytes(rows, D) == -(-rows // H.CHUNK_ROWS) * 2 * D * 4
    for key, inp, var in H.stats_runs(rows, D, (F32, BF16), "bn_stats_rows"):
        xdt = var["xdt"]
        res = {}
        for ldx in (D, D + 12):  # the gap columns hold NaN, which must not reach the result
            x_d = H.strided(inp["x"], ldx).to(cuda)

            def run(running=True):
                outs = _stats_outs(inp, D, cuda, running)
                _lib.check(_stats_rows(lib, x_d, xdt, ldx, rows, D, outs, ws), "hct_bn_stats_rows")
                return outs
            res[ldx] = _twice(run)
            bare = _twice(lambda: run(False))
            assert all(torch.equal(_bits(bare[k]), _bits(res[ldx][k])) for k in ("mean", "var"))
        got = res[D]
        assert all(torch.equal(_bits(res[D + 12][k]), _bits(got[k])) for k in got), (key, "the row stride changes the result")
        _hold_stats(key, inp, var, got, rows <= H.CHUNK_ROWS)
        if rows <= H.CHUNK_ROWS and xdt == F32:  # the promise of finetune.hip: one chunk is hct_batchnorm_stats bit for bit
            x_d = inp["x"].to(cuda)

            def plain():
                outs = _stats_outs(inp, D, cuda, True)
                _lib.check(_batch_stats(lib, x_d, rows, D, outs), "hct_batchnorm_stats")
                return outs
            one = _twice(plain)
            assert all(torch.equal(_bits(one[k]), _bits(got[k])) for k in got), (key, "not bit-identical to hct_batchnorm_stats")


def test_bn_stats_refusals(lib, cuda):
    """One row is refused by both entry points, a workspace one byte short by hct_bn_stats_rows; the outputs stay untouched."""
    rows, D = 129, 7
    inp = H.stats_inputs(rows, D, "centred")
    x_d, ws = inp["x"].to(cuda), _ws(lib.hct_bn_rows_workspace_bytes(rows, D), cuda)
    outs = _stats_outs(inp, D, cuda, False)
    _refused(_batch_stats(lib, x_d, 1, D, outs), outs, lib, "hct_batchnorm_stats")
    outs = _stats_outs(inp, D, cuda, False)
    _refused(_stats_rows(lib, x_d, F32, D, 1, D, outs, ws), outs, lib, "hct_bn_stats_rows")
    outs = _stats_outs(inp, D, cuda, False)
    _refused(_stats_rows(lib, x_d, F32, D, rows, D, outs, ws, short=1), outs, lib, "hct_bn_stats_rows")


# ---- hct_bn_norm -------------------------------------------------------------------------------------------------------------------
# a quad per thread: 7 x 260 / 4 = 455 quads = 1.8 blocks; 1 x 4 a single thread; 5 x 1028 / 4 = 1285 = 5.02 blocks
@pytest.mark.parametrize("rows,D", H.NORM_CASES)
def test_bn_norm(lib, cuda, rows, D):
    for key, inp, var in H.norm_runs(rows, D):
        xdt, odt = var["xdt"], var["odt"]
        d = _dev(inp, cuda, "mean", "var")
        res = {}
        for ldx in (D, D + 12):
            x_d = H.strided(inp["x"], ldx).to(cuda)

            def run():
                out = _Out((rows, D), odt, cuda)
                _lib.check(lib.hct_bn_norm(x_d.data_ptr(), _code(xdt), ldx, rows, D, d["mean"].data_ptr(), d["var"].data_ptr(), EPS, out.ptr, _code(odt),
                                           _st()), "hct_bn_norm")
                return dict(out=out)
            res[ldx] = _twice(run)
        assert torch.equal(_bits(res[D]["out"]), _bits(res[D + 12]["out"]))
        _hold(key, inp, var, res[D], H.norm_ref(inp, var), H.norm_spec(var))


# ---- hct_bn_bwd_input --------------------------------------------------------------------------------------------------------------
# chunk kernel: 128 rows per block: rows = 6 one short chunk, 129 a chunk of one row, 258 a third chunk of two; D = 7 (no multiple of 4)
# and 260 (a second block of four columns); the apply kernel one element per thread: 6 x 7 = 42 ... 258 x 260 = 262.03 blocks
def _bwd_call(lib, d, var, rows, D, dev, ws, strides=(3, 5, 8), nq=None):
    ldx, ldg, ldo = D + strides[0], D + strides[1], D + strides[2]
    dx = _Out((rows, ldo), var["odt"], dev)
    fused = var["form"] == "fused"
    rc = lib.hct_bn_bwd_input(d[("x", ldx)].data_ptr(), _code(var["xdt"]), ldx, d["mean"].data_ptr(), d["var"].data_ptr(), EPS,
                              None if fused else d[("g", ldg)].data_ptr(), 0 if fused else ldg, d["dlogits"].data_ptr() if fused else None,
                              d["W"].data_ptr() if fused else None, nq or var["nq"], var["ncls"], rows, D, dx.ptr, _code(var["odt"]), ldo, ws.data_ptr(),
                              ws.numel(), _st())
    return rc, dict(dx=dx)


@pytest.mark.parametrize("rows,D", H.BWD_CASES)
def test_bn_bwd_input(lib, cuda, rows, D):
    ws = _ws(lib.hct_bn_rows_workspace_bytes(rows, D) + 2 * D * 4, cuda)
    for key, inp, var in H.bwd_runs(rows, D):
        d = _dev(inp, cuda, "mean", "var", "dlogits", "W")
        res = {}
        for strides in ((3, 5, 8), (0, 0, 8)):  # x and g with a NaN-filled gap, and dense
            d[("x", D + strides[0])] = H.strided(inp["x"], D + strides[0]).to(cuda)
            d[("g", D + strides[1])] = H.strided(inp["g"], D + strides[1]).to(cuda)

            def run():
                rc, outs = _bwd_call(lib, d, var, rows, D, cuda, ws, strides)
                _lib.check(rc, "hct_bn_bwd_input")
                return outs
            res[strides] = _twice(run)["dx"]
        full = res[(3, 5, 8)]
        assert torch.equal(_bits(full), _bits(res[(0, 0, 8)])), (key, "the row strides change the result")
        assert bool(torch.isnan(full[:, D:].float()).all()), (key, "the gap columns of dx were written")
        _hold(key, inp, var, dict(dx=full[:, :D]), H.bwd_ref(inp, var), H.bwd_spec(var))


def test_bn_bwd_input_refusals(lib, cuda):
    """Rows that are no multiple of nq (fused form) and a workspace one byte short are refused; dx stays untouched."""
    rows, D = 6, 7
    key, inp, var = next(r for r in H.bwd_runs(rows, D) if r[2]["form"] == "fused" and r[2]["nq"] == 3)
    d = _dev(inp, cuda, "mean", "var", "dlogits", "W")
    d[("x", D + 3)], d[("g", D + 5)] = H.strided(inp["x"], D + 3).to(cuda), H.strided(inp["g"], D + 5).to(cuda)
    ws = _ws(lib.hct_bn_rows_workspace_bytes(rows, D) + 2 * D * 4, cuda)
    rc, outs = _bwd_call(lib, d, var, rows, D, cuda, ws, nq=4)  # 6 rows in groups of 4
    _refused(rc, outs, lib, "hct_bn_bwd_input")
    rc, outs = _bwd_call(lib, d, var, rows, D, cuda, ws[:-1])
    _refused(rc, outs, lib, "hct_bn_bwd_input")


# ---- hct_softmax_xent ---------------------------------------------------------------------------------------------------------------
# a single workgroup, thread t takes rows t, t + 256, ...: B = 255 / 256 / 257 end before, on and one past the first trip, 600 = 2.3 trips
def _xent_call(lib, d, B, C, dev, dloss, want_loss=True, want_dl=True):
    outs = {}
    if want_loss:
        outs["loss"] = _Out((1,), F32, dev)
    if want_dl:
        outs["dlogits"] = _Out((B, C), F32, dev)
    rc = lib.hct_softmax_xent(d["logits"].data_ptr(), d["target"].data_ptr(), B, C, _p(dloss), _p(outs.get("loss")), _p(outs.get("dlogits")), _st())
    return rc, outs


@pytest.mark.parametrize("B,C", H.XENT_CASES)
def test_softmax_xent(lib, cuda, B, C):
    three = torch.tensor([3.0], device=cuda)
    for key, inp, var in H.xent_runs(B, C):
        d = _dev(inp, cuda, "logits", "target")
        assert d["target"].dtype == torch.int64
        dloss = three if var["dloss"] else None

        def run(want_loss=True, want_dl=True):
            rc, outs = _xent_call(lib, d, B, C, cuda, dloss, want_loss, want_dl)
            _lib.check(rc, "hct_softmax_xent")
            return outs
        got = _twice(run)
        _hold(key, inp, var, got, H.xent_ref(inp, var), H.xent_spec(var))
        assert torch.equal(_bits(_twice(lambda: run(want_loss=False))["dlogits"]), _bits(got["dlogits"]))  # loss NULL
        assert torch.equal(_bits(_twice(lambda: run(want_dl=False))["loss"]), _bits(got["loss"]))          # dlogits NULL
    rc, outs = _xent_call(lib, d, B, C, cuda, None, False, False)  # both NULL: nothing to compute
    _refused(rc, outs, lib, "hct_softmax_xent")


def test_softmax_xent_target_out_of_range(lib, cuda):
    """Targets -1 and n_classes: the loss is NaN, every other row's gradient is what it was, nothing outside the outputs is written."""
    B, C = 257, 5
    inp = H.xent_inputs(B, C)
    bad = inp["target"].clone()
    bad[3], bad[256] = -1, C
    d, d_bad = _dev(inp, cuda, "logits", "target"), _dev(dict(inp, target=bad), cuda, "logits", "target")

    def run(dd):
        rc, outs = _xent_call(lib, dd, B, C, cuda, None)
        _lib.check(rc, "hct_softmax_xent")
        return outs
    good, got = _twice(lambda: run(d)), _twice(lambda: run(d_bad))
    keep = torch.ones(B, dtype=torch.bool)
    keep[3] = keep[256] = False
    assert bool(torch.isnan(got["loss"]).all()) and bool(torch.isfinite(good["loss"]).all())
    assert torch.equal(_bits(got["dlogits"][keep]), _bits(good["dlogits"][keep]))
    ref = H.softmax_xent(inp["logits"].double(), bad)[1]
    assert H.worst_row(got["dlogits"], ref) < H.FP32_BAR  # the two rows: the plain softmax, no one-hot entry


# ---- hct_clip_total_norm, hct_add_f32 ---------------------------------------------------------------------------------------------
# a quad per thread: total = 4 a single thread, 1028 = 257 quads: a second block of one thread
@pytest.mark.parametrize("nseg,total", H.CLIP_CASES)
def test_clip_total_norm_and_add(lib, cuda, nseg, total):
    for key, inp, var in H.clip_runs(nseg, total):
        d = _dev(inp, cuda, "norms")

        def run():
            outs = dict(grads=_inout(inp["grads"], cuda), nrm=_Out((2,), F32, cuda))
            _lib.check(lib.hct_clip_total_norm(outs["grads"].ptr, total, d["norms"].data_ptr(), nseg, var["max_norm"], outs["nrm"].ptr, _st()),
                       "hct_clip_total_norm")
            return outs
        got = _twice(run)
        _hold(key, inp, var, got, H.clip_ref(inp, var), H.clip_spec(var))
        if var["where"] == "above":  # nothing to clip: the buffer comes back bit-unchanged
            assert float(got["nrm"][1]) == 1.0 and torch.equal(_bits(got["grads"]), _bits(inp["grads"]))
        else:  # one multiplication by the coefficient the kernel itself wrote
            assert float(got["nrm"][1]) < 1.0 and torch.equal(_bits(got["grads"]), _bits(inp["grads"] * got["nrm"][1]))
    src = H.values((total,), "normal", H.gen(nseg, total, 32))
    src_d = src.to(cuda)

    def add():
        dst = _inout(inp["grads"], cuda)
        _lib.check(lib.hct_add_f32(dst.ptr, src_d.data_ptr(), total, _st()), "hct_add_f32")
        return dict(dst=dst)
    assert torch.equal(_bits(_twice(add)["dst"]), _bits(inp["grads"] + src))


# ---- hct_dino_loss -----------------------------------------------------------------------------------------------------------------
# dino_row_stats_kernel, 1024 columns per trip: K = 4 a single thread, 1000 a ragged first trip, 1024 a whole one, 1028 a second trip by
#   thread 0, 2052 a third; dino_loss_grad_kernel one block per 1024 columns and sample, looping over the V crops (2: global only;
#   3: one local crop paired with both teachers; 10: the training default); dino_fold_kernel folds B x nchunk <= 9 partials
def _dino_call(lib, d, var, V, B, K, dev, ws, dloss=None, want_ds=True, want_cs=True, short=0):
    dt = var["dtype"]
    outs = dict(loss=_Out((1,), F32, dev))
    if want_ds:
        outs["dstudent"] = _Out((V * B, K), dt, dev)
    if want_cs:
        outs["center_sum"] = _Out((K,), F32, dev)
    rc = lib.hct_dino_loss(d["student"].data_ptr(), d["teacher"].data_ptr(), _code(dt), V, B, K, d["center"].data_ptr(), var["Ts"], var["Tt"], outs["loss"].ptr,
                           _p(outs.get("dstudent")), _p(dloss), _p(outs.get("center_sum")), ws.data_ptr(), lib.hct_dino_loss_workspace_bytes(V, B, K) - short,
                           _st())
    return rc, outs


@pytest.mark.parametrize("V,B,K", H.DINO_CASES)
def test_dino_loss(lib, cuda, V, B, K):
    ws = _ws(lib.hct_dino_loss_workspace_bytes(V, B, K), cuda)
    three = torch.tensor([3.0], device=cuda)
    for key, inp, var in H.dino_runs(V, B, K):
        d = _dev(inp, cuda, "student", "teacher", "center")
        assert d["student"].dtype == var["dtype"]

        def run(**kw):
            rc, outs = _dino_call(lib, d, var, V, B, K, cuda, ws, **kw)
            _lib.check(rc, "hct_dino_loss")
            return outs
        got = _twice(run)
        assert bool(torch.isfinite(got["dstudent"].float()).all())
        _hold(key, inp, var, got, H.dino_ref(inp, var), H.dino_spec(var))
        no_ds, no_cs = _twice(lambda: run(want_ds=False)), _twice(lambda: run(want_cs=False))  # dstudent NULL; batch_center_sum NULL
        assert torch.equal(_bits(no_ds["loss"]), _bits(got["loss"])) and torch.equal(_bits(no_ds["center_sum"]), _bits(got["center_sum"]))
        assert torch.equal(_bits(no_cs["loss"]), _bits(got["loss"])) and torch.equal(_bits(no_cs["dstudent"]), _bits(got["dstudent"]))
        if var["kind"] == "normal":  # dloss = 3: the gradient scales, the loss does not
            scaled = _twice(lambda: run(dloss=three))
            assert torch.equal(_bits(scaled["loss"]), _bits(got["loss"]))
            _hold(key, inp, var, dict(dstudent=scaled["dstudent"]), H.dino_ref(inp, var, dloss=3.0), H.dino_spec(var))


def test_dino_loss_workspace_too_small(lib, cuda):
    V, B, K = 3, 3, 1028
    key, inp, var = next(iter(H.dino_runs(V, B, K)))
    d = _dev(inp, cuda, "student", "teacher", "center")
    nws = lib.hct_dino_loss_workspace_bytes(V, B, K)
    assert nws >= (V + 2) * B * 8 + B * 2 * 4 + B * K * 4
    rc, outs = _dino_call(lib, d, var, V, B, K, cuda, _ws(nws, cuda), short=1)
    assert rc == HCT_E_WORKSPACE
    _refused(rc, outs, lib, "hct_dino_loss")


# ---- hct_dino_center_update ---------------------------------------------------------------------------------------------------------
# one thread per column: K = 1, 255, 257 (a second block of one thread)
@pytest.mark.parametrize("K,count", H.CENTER_CASES)
def test_dino_center_update(lib, cuda, K, count):
    """In place, bit-equal to torch's fp32 sequence center * m + (sum / count) * (1 - m): the library is built with -ffp-contract=off."""
    inp = H.center_inputs(K, count)
    sum_d = inp["sum"].to(cuda)

    def run():
        center = _inout(inp["center"], cuda)
        _lib.check(lib.hct_dino_center_update(center.ptr, sum_d.data_ptr(), K, 0.9, float(count), _st()), "hct_dino_center_update")
        return dict(center=center)
    assert torch.equal(_bits(_twice(run)["center"]), _bits(H.center_update(inp["center"], inp["sum"], 0.9, count)))
