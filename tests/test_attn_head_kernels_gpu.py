"""The attentive classification head's kernels (csrc/heads.hip: hct_query_attention / _lse, hct_head_linear / _x / _bwd / _wgrad,
hct_channel_norm; csrc/finetune.hip: hct_query_attention_bwd) and the copy passes its training step launches (csrc/elementwise.hip:
hct_cast, hct_transpose_cast, hct_colsum, hct_gather_rows) through the C ABI, one entry point at a time, against the plain restatements
of tests/attn_head_ref.py evaluated in float64.

Every output is pre-filled with NaN (integers: a sentinel) inside a buffer with a guard band on each side that must come back untouched,
and every call is made twice: the two results must agree bit for bit.  Padding of a strided input is NaN.  Error is taken per row and
the worst row must hold the bar: the project's (fp32 1e-5, stored bf16 4e-3) or, for the cases listed in R.RESTATEMENT, ten times the
error that fp32 arithmetic in the kernel's own order has on the CPU; a "peaked" case adds the allowance for the fast exponential that
R.exponent_allowance works out from its own logits.  Rows of dK and dq are measured on the un-cancelled magnitude of their sum.  Copies
are held bit-equal; sums are bit-equal on integer-valued inputs and within their rounding bound otherwise.  The sizes are the ones at
which each kernel's loop is taken a second time or ends raggedly; tests/test_attn_head_ref_cpu.py asserts that they are.  Every figure
is printed beside its bar (`FIG entry figure error bar`)."""
import pytest
import torch

from headct_foundation_amd import _lib
from headct_foundation_amd._lib import HCT_ACT_GELU, HCT_ACT_NONE, HCT_ACT_TANH, HCT_BF16, HCT_F16, HCT_F32
from tests import attn_head_ref as R
from tests import head_kernels_ref as H
from tests.test_assembly_kernels_gpu import _Out, _bits, _check_sum, _code, _p, _st, _twice

pytestmark = pytest.mark.gpu

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
HCT_E_BADARG, HCT_E_UNSUPPORTED, HCT_E_WORKSPACE = -1, -2, -3
EPS = R.EPS


def _ws(nbytes, dev):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=dev)


def _fig(entry, key, name, err, bar):
    print(f"FIG {entry} {name} {err:.3e} {bar:.3e} {key}")
    assert err < bar, (entry, key, name, err, bar)


def _refused(rc, outs, lib, name, code=None):
    torch.cuda.synchronize()
    assert rc != 0 and (code is None or rc == code) and name in lib.hct_last_error_string().decode(), (name, rc, lib.hct_last_error_string())
    for o in outs.values():
        o.result()
        assert o.untouched(), name


def _within(got, ref, bound, exact, what):
    """A sum: exact where the inputs make it so, else every element within its rounding bound of the float64 value."""
    assert got.dtype == F32 and not bool(torch.isnan(got).any()), what
    err = (got.double() - ref.reshape(got.shape)).abs()
    if exact:
        assert float(err.max()) == 0.0, (what, "integer-valued sum is not exact", float(err.max()))
        return
    over = float((err - bound.reshape(got.shape)).max())
    print(f"FIG {what}: max err {float(err.max()):.3e}, max bound {float(bound.max()):.3e}, max (err - bound) {over:.3e}")
    assert over <= 0.0, (what, over)


# ---- hct_query_attention / _lse / _bwd ----------------------------------------------------------------------------------------------
# forward: scores by 256 threads; a wave per query (Q = 5: a second trip), lanes over n (N = 65: a second trip); P V per wave over n =
# wave, wave + 4, ... (N < 4: idle waves).  backward: lanes hold d and d + 64 (dh = 48: idle lanes; 72, 128: the second slot).
def _fwd(lib, d, dims, ls, kvdt, dev, entry="lse"):
    B, N, Hh, Q, dh = dims
    outs = dict(out=_Out((B, Hh, Q, dh), F32, dev))
    if entry == "plain":
        rc = lib.hct_query_attention(d["q"].data_ptr(), Q, d["kv"].data_ptr(), _code(kvdt), B, N, Hh, dh, ls, outs["out"].ptr, _st())
    else:
        if entry == "lse":
            outs["lse"] = _Out((B, Hh, Q), F32, dev)
        rc = lib.hct_query_attention_lse(d["q"].data_ptr(), Q, d["kv"].data_ptr(), _code(kvdt), B, N, Hh, dh, ls, outs["out"].ptr, _p(outs.get("lse")), _st())
    return rc, outs


def _bwd(lib, d, dims, ls, kvdt, dev, out_ptr, lse_ptr, short=0):
    B, N, Hh, Q, dh = dims
    outs = dict(dkv=_Out((B, N, 2, Hh, dh), kvdt, dev), dq=_Out((Q, Hh * dh), F32, dev))
    need = lib.hct_query_attention_bwd_workspace_bytes(B, Q, Hh, dh)
    ws = _ws(need, dev)
    rc = lib.hct_query_attention_bwd(d["q"].data_ptr(), Q, d["kv"].data_ptr(), _code(kvdt), B, N, Hh, dh, ls, out_ptr, lse_ptr, d["dout"].data_ptr(),
                                     outs["dkv"].ptr, outs["dq"].ptr, ws.data_ptr(), need - short, _st())
    return rc, outs


def _grads(got):
    return dict(dk=got["dkv"][:, :, 0], dv=got["dkv"][:, :, 1], dq=got["dq"])


def _hold(entry, figs, only=None):
    for k, (e, b, _) in figs.items():
        if only is None or k[-1] in only:
            _fig(entry, k[:-1], k[-1], e, b)


@pytest.mark.parametrize("Q,dh", R.ATTN_GROUPS)
def test_query_attention_forward_and_backward(lib, cuda, Q, dh):
    for key, inp, var in R.attn_runs(Q, dh):
        B, N = key[1], key[2]
        dims, ls, kvdt = (B, N, R.ATTN_H, Q, dh), inp["ls"], var["kv_dtype"]
        ref = R.attn_ref(inp, var)
        d = {k: inp[k].contiguous().to(cuda) for k in ("q", "kv", "dout")}
        d.update(out=ref["out"].float().contiguous().to(cuda), lse=ref["lse"].float().contiguous().to(cuda))   # the backward's: the float64 forward, rounded
        chained = N in R.ATTN_CHAINED_N

        def run():
            rc, outs = _fwd(lib, d, dims, ls, kvdt, cuda)
            _lib.check(rc, "hct_query_attention_lse")
            for entry in ("plain", "null"):
                rc, other = _fwd(lib, d, dims, ls, kvdt, cuda, entry)
                _lib.check(rc, "hct_query_attention " + entry)
                outs[entry] = other["out"]
            rc, grads = _bwd(lib, d, dims, ls, kvdt, cuda, d["out"].data_ptr(), d["lse"].data_ptr())
            _lib.check(rc, "hct_query_attention_bwd")
            outs.update(grads)
            if chained:  # after the kernel's own forward
                rc, grads = _bwd(lib, d, dims, ls, kvdt, cuda, outs["out"].ptr, outs["lse"].ptr)
                _lib.check(rc, "hct_query_attention_bwd (chained)")
                outs.update(chained_dkv=grads["dkv"], chained_dq=grads["dq"])
            return outs
        got = _twice(run)
        assert torch.equal(_bits(got["plain"]), _bits(got["out"])) and torch.equal(_bits(got["null"]), _bits(got["out"])), key
        _hold("hct_query_attention", R.attn_errors(key, var, dict(out=got["out"], lse=got["lse"]), ref))
        _hold("hct_query_attention_bwd", R.attn_errors(key, var, _grads(got), ref))   # (worst_row refuses a NaN: every row of dkv was written)
        if chained:
            ref2 = R.attn_ref(inp, var, fwd=(got["out"], got["lse"]))
            _hold("hct_query_attention_bwd(chained)", R.attn_errors(key, var, _grads(dict(dkv=got["chained_dkv"], dq=got["chained_dq"])), ref2))


def test_query_attention_at_the_lds_boundary(lib, cuda):
    """Q N + 4 Q dh + Q = 16384 floats is accepted and correct; one token more is refused before anything is launched."""
    for key, inp, var in R.attn_lds_runs():
        N, Q, dh = key[2], key[3], key[4]
        dims, kvdt = (1, N, 1, Q, dh), var["kv_dtype"]
        d = {k: inp[k].contiguous().to(cuda) for k in ("q", "kv")}

        def run():
            rc, outs = _fwd(lib, d, dims, inp["ls"], kvdt, cuda)
            _lib.check(rc, "hct_query_attention_lse")
            return outs
        _hold("hct_query_attention", R.attn_errors(key, var, _twice(run), R.attn_ref(inp, var, bwd=False)))
        more = dict(q=d["q"], kv=torch.zeros(1, N + 1, 2, 1, dh, dtype=kvdt, device=cuda))
        for entry in ("lse", "plain"):
            rc, outs = _fwd(lib, more, (1, N + 1, 1, Q, dh), inp["ls"], kvdt, cuda, entry)
            _refused(rc, outs, lib, "hct_query_attention", HCT_E_UNSUPPORTED)


def test_query_attention_equal_keys_and_refusals(lib, cuda):
    """Integer inputs, Q = 1, every key the same and orthogonal to the query: p = 1 / N exactly, so dV[n] = dout / N bit for bit and out is
    the mean of V.  Then the refusals: a kv dtype other than fp32 / bf16, dh = 132, a workspace one byte short, 6 Q dh + 2 Q > 16384."""
    for N in R.ATTN_EQUAL_KEY_N:
        for kvdt in (F32, BF16):
            inp = R.attn_equal_key_inputs(N, kvdt)
            dims = (2, N, 3, 1, 16)
            out, lse = R.query_attention(inp["q"].double(), inp["kv"].double(), inp["ls"])
            d = {k: inp[k].contiguous().to(cuda) for k in ("q", "kv", "dout")}
            d.update(out=out.float().contiguous().to(cuda), lse=lse.float().contiguous().to(cuda))

            def run():
                rc, outs = _fwd(lib, d, dims, inp["ls"], kvdt, cuda)
                _lib.check(rc, "hct_query_attention_lse")
                rc, grads = _bwd(lib, d, dims, inp["ls"], kvdt, cuda, d["out"].data_ptr(), d["lse"].data_ptr())
                _lib.check(rc, "hct_query_attention_bwd")
                return dict(outs, **grads)
            got = _twice(run)
            _fig("hct_query_attention", ("equal keys", N, kvdt), "out", H.worst_row(got["out"], out), R.FP32_BAR)
            want = (inp["dout"][:, :, 0] / N)[:, None].expand(-1, N, -1, -1).to(kvdt)
            assert torch.equal(_bits(got["dkv"][:, :, 1].contiguous()), _bits(want.contiguous())), (N, kvdt)
            assert not bool(torch.isnan(got["dkv"].float()).any()) and not bool(torch.isnan(got["dq"]).any())
    assert lib.hct_query_attention_bwd_workspace_bytes(2, 5, 3, 72) == 2 * 5 * 3 * 72 * 4   # the per-volume dq partials
    inp = R.attn_inputs(1, 4, 1, 22, 132, "moderate", F32)
    d = {k: inp[k].contiguous().to(cuda) for k in ("q", "kv", "dout")}
    d.update(out=torch.zeros(1, 1, 22, 132, device=cuda), lse=torch.zeros(1, 1, 22, device=cuda))
    for entry in ("lse", "plain"):
        rc, outs = _fwd(lib, d, (1, 4, 1, 1, 16), 0.25, F16, cuda, entry)
        _refused(rc, outs, lib, "hct_query_attention", HCT_E_BADARG)
    for dims, kvdt, short, code in (((1, 4, 1, 1, 132), F32, 0, HCT_E_BADARG), ((1, 4, 1, 1, 16), F32, 1, HCT_E_BADARG),
                                    ((1, 4, 1, 22, 128), F32, 0, HCT_E_UNSUPPORTED), ((1, 4, 1, 1, 16), F16, 0, HCT_E_BADARG)):
        rc, outs = _bwd(lib, d, dims, 0.25, kvdt, cuda, d["out"].data_ptr(), d["lse"].data_ptr(), short)
        _refused(rc, outs, lib, "hct_query_attention_bwd", code)


# ---- hct_head_linear / _x ------------------------------------------------------------------------------------------------------------
# one wave per output, four to a block: rows x n_out = 1, 3, 5, 13 leave waves of the last block idle; the lanes add k = lane, lane + 64,
# ...: D = 1 one lane, 63 all but one, 64 a whole trip, 65 a second by lane 0, 768 twelve
def _hl_call(lib, d, var, rows, D, n_out, nq, ldx, dev, entry, act=None, x_code=None, stats=None):
    out = _Out((rows, n_out), F32, dev)
    stats = (var["stats"], var["stats"]) if stats is None else stats
    mean, v = (d["mean"].data_ptr() if stats[0] else None), (d["var"].data_ptr() if stats[1] else None)
    bias = d["bias"].data_ptr() if var["bias"] else None
    if entry == "hct_head_linear":
        act = (HCT_ACT_TANH if var["tanh"] else HCT_ACT_NONE) if act is None else act
        rc = lib.hct_head_linear(d["x"].data_ptr(), ldx, nq, mean, v, EPS, d["W"].data_ptr(), bias, act, out.ptr, rows, D, n_out, _st())
    else:
        rc = lib.hct_head_linear_x(d["x"].data_ptr(), _code(var["xdt"]) if x_code is None else x_code, ldx, nq, mean, v, EPS, d["W"].data_ptr(), bias, out.ptr,
                                   rows, D, n_out, _st())
    return rc, dict(out=out)


@pytest.mark.parametrize("D", R.HL_D)
def test_head_linear(lib, cuda, D):
    for key, inp, var in R.hl_runs(D):
        rows, n_out, nq, xdt = key[1], key[3], key[4], var["xdt"]
        ref = R.hl_ref(inp, var)
        for pad in R.HL_PAD:
            ldx = nq * D + pad
            d = {k: inp[k].contiguous().to(cuda) for k in ("W", "bias", "mean", "var")}
            d["x"] = R.strided(inp["x"].reshape(rows, nq * D), ldx).to(cuda)
            entries = (["hct_head_linear"] if xdt == F32 else []) + ([] if var["tanh"] else ["hct_head_linear_x"])

            def run():
                outs = {}
                for entry in entries:
                    rc, o = _hl_call(lib, d, var, rows, D, n_out, nq, ldx, cuda, entry)
                    _lib.check(rc, entry)
                    outs[entry] = o["out"]
                return outs
            got = _twice(run)
            for entry in entries:
                e, b, _ = R.hl_error(key, var, got[entry], ref)
                _fig(entry, key + (pad,), "out", e, b)
            if len(entries) == 2:
                assert torch.equal(_bits(got["hct_head_linear"]), _bits(got["hct_head_linear_x"])), key


def test_head_linear_refusals(lib, cuda):
    key, inp, var = next(iter(R.hl_runs(65)))
    rows, n_out, nq, D = key[1], key[3], 3, 65
    d = {k: inp[k].contiguous().to(cuda) for k in ("W", "bias", "mean", "var", "dlogits")}
    d["x"] = torch.zeros(rows, nq * D + 8, device=cuda)
    for entry in ("hct_head_linear", "hct_head_linear_x"):
        for kw in (dict(ldx=nq * D - 1), dict(stats=(True, False)), dict(stats=(False, True))) + ((dict(act=HCT_ACT_GELU), dict(act=7)) if entry == "hct_head_linear"
                                                                                                   else (dict(x_code=HCT_F16), dict(x_code=7))):
            rc, outs = _hl_call(lib, d, var, rows, D, n_out, nq, kw.pop("ldx", nq * D), cuda, entry, **kw)
            _refused(rc, outs, lib, entry, HCT_E_BADARG)
    for ldx, stats, code in ((nq * D - 1, (True, True), HCT_F32), (nq * D, (True, False), HCT_F32), (nq * D, (False, True), HCT_F32), (nq * D, (True, True), HCT_F16)):
        outs = dict(dW=_Out((n_out, D), F32, cuda), db=_Out((n_out,), F32, cuda))
        rc = lib.hct_head_linear_bwd(d["x"].data_ptr(), code, ldx, nq, d["mean"].data_ptr() if stats[0] else None, d["var"].data_ptr() if stats[1] else None, EPS,
                                     d["dlogits"].data_ptr(), rows, D, n_out, outs["dW"].ptr, outs["db"].ptr, _st())
        _refused(rc, outs, lib, "hct_head_linear_bwd", HCT_E_BADARG)


# ---- hct_head_linear_bwd / _wgrad ------------------------------------------------------------------------------------------------------
# one thread per (c, k), rows in index order: n_out x D = 1 ... 3840 = fifteen blocks; 2 x 130 = 260 a second block of four threads
@pytest.mark.parametrize("B,D,n_out", R.HL_BWD_CASES)
def test_head_linear_bwd(lib, cuda, B, D, n_out):
    for key, inp, var in R.hl_bwd_runs(B, D, n_out):
        nq, xdt, stats = var["nq"], var["xdt"], var["stats"]
        dW_ref, db_ref = R.hl_bwd_ref(inp, var)
        (dW_bound, db_bound), exact = R.hl_bwd_limits(inp, var)
        for pad in R.HL_PAD:
            ldx = nq * D + pad
            d = {k: inp[k].contiguous().to(cuda) for k in ("mean", "var", "dlogits")}
            d["x"] = R.strided(inp["x"].reshape(B, nq * D), ldx).to(cuda)
            mean, v = (d["mean"].data_ptr(), d["var"].data_ptr()) if stats else (None, None)
            plain = nq == 1 and xdt == F32 and pad == 0

            def run():
                outs = dict(dW=_Out((n_out, D), F32, cuda), db=_Out((n_out,), F32, cuda), dW_alone=_Out((n_out, D), F32, cuda))
                _lib.check(lib.hct_head_linear_bwd(d["x"].data_ptr(), _code(xdt), ldx, nq, mean, v, EPS, d["dlogits"].data_ptr(), B, D, n_out, outs["dW"].ptr,
                                                   outs["db"].ptr, _st()), "hct_head_linear_bwd")
                _lib.check(lib.hct_head_linear_bwd(d["x"].data_ptr(), _code(xdt), ldx, nq, mean, v, EPS, d["dlogits"].data_ptr(), B, D, n_out, outs["dW_alone"].ptr,
                                                   None, _st()), "hct_head_linear_bwd (db NULL)")
                if plain:
                    outs.update(dW_wgrad=_Out((n_out, D), F32, cuda), db_wgrad=_Out((n_out,), F32, cuda))
                    _lib.check(lib.hct_head_linear_wgrad(d["x"].data_ptr(), mean, v, EPS, d["dlogits"].data_ptr(), B, D, n_out, outs["dW_wgrad"].ptr,
                                                         outs["db_wgrad"].ptr, _st()), "hct_head_linear_wgrad")
                return outs
            got = _twice(run)
            _within(got["dW"], dW_ref, dW_bound, exact, f"hct_head_linear_bwd dW {key} pad={pad}")
            _within(got["db"], db_ref, db_bound, var["kind"] == "int", f"hct_head_linear_bwd db {key} pad={pad}")
            assert torch.equal(_bits(got["dW_alone"]), _bits(got["dW"])), key
            if plain:
                assert torch.equal(_bits(got["dW_wgrad"]), _bits(got["dW"])) and torch.equal(_bits(got["db_wgrad"]), _bits(got["db"])), key


# ---- hct_channel_norm ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,C", R.CN_CASES)
def test_channel_norm(lib, cuda, rows, C):
    for key, inp, var in R.cn_runs(rows, C):
        odt = var["odt"]
        d = {k: inp[k].contiguous().to(cuda) for k in ("x", "mean", "var")}

        def run():
            outs = dict(out=_Out((rows, C), odt, cuda), bn=_Out((rows, C), odt, cuda))
            _lib.check(lib.hct_channel_norm(d["x"].data_ptr(), d["mean"].data_ptr(), d["var"].data_ptr(), EPS, outs["out"].ptr, _code(odt), rows, C, _st()),
                       "hct_channel_norm")
            _lib.check(lib.hct_bn_norm(d["x"].data_ptr(), HCT_F32, C, rows, C, d["mean"].data_ptr(), d["var"].data_ptr(), EPS, outs["bn"].ptr, _code(odt), _st()),
                       "hct_bn_norm")
            return outs
        got = _twice(run)
        assert torch.equal(_bits(got["out"]), _bits(got["bn"])), key
        _, default = H.norm_spec(var)["out"]
        _fig("hct_channel_norm", key, "out", H.worst_row(got["out"], H.norm_ref(inp, var)["out"]), R.bar(key + ("out",), default))
    x = torch.zeros(rows, R.CN_REFUSED_C, device=cuda)
    for odt, code in ((F32, HCT_F32), (BF16, HCT_BF16), (F32, HCT_F16)):
        outs = dict(out=_Out((rows, R.CN_REFUSED_C if code != HCT_F16 else 8), odt, cuda))
        rc = lib.hct_channel_norm(x.data_ptr(), x.data_ptr(), x.data_ptr(), EPS, outs["out"].ptr, code, rows, R.CN_REFUSED_C if code != HCT_F16 else 4, _st())
        _refused(rc, outs, lib, "hct_channel_norm", HCT_E_BADARG)


# ---- hct_cast / hct_transpose_cast ----------------------------------------------------------------------------------------------------
# cast: a quad per thread, at most 2048 blocks of 256: n = 2048 x 1024 + 5 takes the grid-stride loop a second time, with a scalar tail
@pytest.mark.parametrize("sdt,ddt", R.DTYPE_PAIRS)
def test_cast(lib, cuda, sdt, ddt):
    for n in R.CAST_N:
        src = R.cast_values(n, sdt, 45)
        sd = src.to(cuda)

        def run():
            dst = _Out((n,), ddt, cuda)
            _lib.check(lib.hct_cast(sd.data_ptr(), _code(sdt), dst.ptr, _code(ddt), n, _st()), "hct_cast")
            return dict(dst=dst)
        assert torch.equal(_bits(_twice(run)["dst"]), _bits(R.cast(src, ddt))), n
    dst = _Out((8,), ddt, cuda)
    rc = lib.hct_cast(sd.data_ptr(), _code(sdt), dst.ptr, _code(ddt), 0, _st())   # n = 0: nothing is written
    torch.cuda.synchronize()
    dst.result()
    assert rc == 0 and dst.untouched()
    for codes in ((HCT_F16, _code(ddt)), (_code(sdt), HCT_F16), (7, _code(ddt)), (_code(sdt), -1)):
        outs = dict(dst=_Out((8,), ddt, cuda))
        _refused(lib.hct_cast(sd.data_ptr(), codes[0], outs["dst"].ptr, codes[1], 8, _st()), outs, lib, "hct_cast", HCT_E_BADARG)
        outs = dict(dst=_Out((4, 2), ddt, cuda))
        _refused(lib.hct_transpose_cast(sd.data_ptr(), codes[0], outs["dst"].ptr, codes[1], 2, 4, _st()), outs, lib, "hct_transpose_cast", HCT_E_BADARG)


@pytest.mark.parametrize("sdt,ddt", R.DTYPE_PAIRS)
def test_transpose_cast(lib, cuda, sdt, ddt):
    for rows, cols in R.TRANSPOSE_CASES:   # 64 x 64 tiles: one element; ragged both ways; one whole tile; 2 x 3 and 5 x 3 tiles, ragged
        src = R.cast_values(rows * cols, sdt, 46).reshape(rows, cols)
        sd = src.to(cuda)

        def run():
            dst = _Out((cols, rows), ddt, cuda)
            _lib.check(lib.hct_transpose_cast(sd.data_ptr(), _code(sdt), dst.ptr, _code(ddt), rows, cols, _st()), "hct_transpose_cast")
            return dict(dst=dst)
        assert torch.equal(_bits(_twice(run)["dst"]), _bits(R.transpose_cast(src, ddt))), (rows, cols)


# ---- hct_colsum ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", R.COLSUM_COLS_LIST)
def test_colsum(lib, cuda, cols):
    for rows in R.colsum_rows(cols):
        need = lib.hct_colsum_workspace_bytes(rows, cols)
        assert need == R.colsum_chunks(rows, cols) * cols * 4
        ws = _ws(need, cuda)
        for dt in (F32, BF16):
            for kind in ("int", "normal"):
                x = H.values((rows, cols), kind, H.gen(rows, cols, 44)).to(dt)
                ref, mag = x.double().sum(0), x.double().abs().sum(0)
                for pad in R.COLSUM_PAD:
                    xd = R.strided(x, cols + pad).to(cuda)

                    def run(short=0, checked=True):
                        out = _Out((cols,), F32, cuda)
                        rc = lib.hct_colsum(xd.data_ptr(), _code(dt), rows, cols, cols + pad, out.ptr, ws.data_ptr(), need - short, _st())
                        if checked:
                            _lib.check(rc, "hct_colsum")
                            return dict(out=out)
                        return rc, dict(out=out)
                    _check_sum(_twice(run)["out"], ref, torch.full((cols,), rows), mag, kind, f"hct_colsum {rows}x{cols} ld={cols + pad} {dt} {kind}")
        _refused(*run(short=1, checked=False), lib, "hct_colsum", HCT_E_WORKSPACE)


# ---- hct_gather_rows -------------------------------------------------------------------------------------------------------------------
# a 16-byte piece per thread, at most 8192 blocks of 256: 21846 rows of 96 pieces are 64 pieces past one trip of the whole grid
@pytest.mark.parametrize("n_rows,row_bytes", [(37, b) for b in R.GATHER_ROW_BYTES] + [R.GATHER_BIG])
def test_gather_rows(lib, cuda, n_rows, row_bytes):
    n_src, w = 11 if n_rows < 100 else 64, row_bytes // 4
    src = torch.randint(-2 ** 31, 2 ** 31 - 1, (n_src, w), generator=H.gen(n_rows, row_bytes, 47), dtype=torch.int64).to(torch.int32)
    idx = R.gather_index(n_rows, n_src, 48)
    sd, idd = src.to(cuda), idx.to(cuda)

    def run():
        dst = _Out((n_rows, w), torch.int32, cuda)
        _lib.check(lib.hct_gather_rows(sd.data_ptr(), idd.data_ptr(), n_rows, row_bytes, dst.ptr, _st()), "hct_gather_rows")
        return dict(dst=dst)
    got = _twice(run)["dst"]
    assert torch.equal(got, R.gather_rows(src, idx)) and bool((got[idx < 0] == 0).all()) and int((idx < 0).sum()) >= 2
    if n_rows < 100:
        dst = _Out((n_rows, w), torch.int32, cuda)
        rc = lib.hct_gather_rows(sd.data_ptr(), idd.data_ptr(), 0, row_bytes, dst.ptr, _st())   # no rows: nothing is written
        torch.cuda.synchronize()
        dst.result()
        assert rc == 0 and dst.untouched()
        outs = dict(dst=_Out((n_rows, 6), torch.int32, cuda))
        _refused(lib.hct_gather_rows(sd.data_ptr(), idd.data_ptr(), 4, R.GATHER_REFUSED_BYTES, outs["dst"].ptr, _st()), outs, lib, "hct_gather_rows", HCT_E_BADARG)
