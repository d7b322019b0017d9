"""The LoRA kernels of csrc/lora.hip (lora_rmw_mfma_kernel at its six instances, lora_rmw_generic_kernel, lora_gather_kernel) and the
host code of hct_lora_qv_fwd / hct_lora_qv_bwd, through the C ABI, against tests/lora_kernel_ref.py: the float64 value of the
header's formulas, a derived per-element bound, and integer inputs for which every output must be bit-equal.

Every buffer a call writes (T, qkv, the four gradients, dx1) is a view inside a larger NaN-filled allocation whose margins must
come back NaN; T and the gradients are NaN beforehand (they are overwritten); the workspace is followed by a pattern that must
survive.  Which kernel instance a case reaches is restated in lora_kernel_ref.instance and asserted on the CPU
(tests/test_lora_kernel_ref_cpu.py); this file names it in its reports."""
import dataclasses
import json
import time

import pytest
import torch

from headct_foundation_amd import _lib
from tests import lora_kernel_ref as K

pytestmark = pytest.mark.gpu

PAD = 256          # elements of margin on either side (a multiple of 16 bytes in both dtypes)
NAN = float("nan")
GRADS = ("dAq", "dAv", "dBq", "dBv")
STATS = {}         # (instance, output) -> [worst |err| / bound, integer outputs bit-equal, integer outputs checked]


def _st():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.view({2: torch.int16, 4: torch.int32, 1: torch.uint8}[t.element_size()])


def _name(inst):
    return "generic" if inst[0] == "generic" else f"mfma<KS={inst[1]},pairs={inst[2]}>"


@pytest.fixture(scope="module", autouse=True)
def summary():
    t0 = time.time()
    yield
    rows = {f"{k[0]} {k[1]}": dict(worst_ratio=round(v[0], 4), int_equal=v[1], int_checked=v[2]) for k, v in sorted(STATS.items())}
    print("\nLORA_KERNEL_SUMMARY " + json.dumps(dict(seconds=round(time.time() - t0, 1), rows=rows)))


class Framed:
    """A contiguous tensor of `shape` inside a flat NaN-filled allocation, `off` elements past a 16-byte boundary."""

    def __init__(self, shape, dtype, dev, fill=None, off=0):
        n = 1
        for s in shape:
            n *= s
        self.start, self.n = PAD + off, n
        self.flat = torch.full((PAD + off + n + PAD,), NAN, dtype=dtype, device=dev)
        self.view = self.flat[self.start:self.start + n].view(shape)
        if fill is not None:
            self.view.copy_(fill.view(shape))

    @property
    def ptr(self):
        return self.view.data_ptr()

    def margins_intact(self):
        return bool(torch.isnan(self.flat[:self.start]).all()) and bool(torch.isnan(self.flat[self.start + self.n:]).all())


class Call:
    """The device operands of one case and generator, and the two entries."""

    def __init__(self, lib, dev, case, d):
        self.lib, self.dev, self.case, self.d = lib, dev, case, d
        self.td = K.torch_dtype(case)
        self.code = _lib.HCT_BF16 if case.dtype == "bf16" else _lib.HCT_F32
        put = lambda v: v.to(dev, self.td).contiguous()
        self.inp = {k: put(d[k]) for k in ("x1", "Aq", "Av", "Bq", "Bv", "T")}
        self.tr = {k: (put(d[k].t()) if use else None) for k, use in (("Aq", case.at), ("Av", case.at), ("Bq", case.bt), ("Bv", case.bt))}
        self.dqkv = Framed((case.B, case.N, 3, case.H, case.dh), self.td, dev, fill=d["dqkv"], off=case.qkv_off)
        self.ws_bytes = lib.hct_lora_qv_bwd_workspace_bytes(case.M, case.D, case.r, self.code)
        self.ws = torch.full((self.ws_bytes + 1024,), 0xA5, dtype=torch.uint8, device=dev)

    def forward(self):
        c, i = self.case, self.inp
        out = dict(T=Framed((c.M, 2 * c.r), self.td, self.dev),
                   qkv=Framed((c.B, c.N, 3, c.H, c.dh), self.td, self.dev, fill=self.d["qkv"], off=c.qkv_off))
        rc = self.lib.hct_lora_qv_fwd(i["x1"].data_ptr(), i["Aq"].data_ptr(), i["Av"].data_ptr(), i["Bq"].data_ptr(), i["Bv"].data_ptr(), c.B, c.N,
                                      c.H, c.dh, c.r, self.code, out["T"].ptr, out["qkv"].ptr, _st())
        _lib.check(rc, "hct_lora_qv_fwd " + c.name)
        torch.cuda.synchronize()
        return out

    def backward(self, base):
        c, i = self.case, self.inp
        out = {k: Framed((c.r, c.D) if k[1] == "A" else (c.D, c.r), torch.float32, self.dev) for k in GRADS}
        out["dx1"] = Framed((c.M, c.D), self.td, self.dev, fill=base)
        ptr = lambda v: None if v is None else v.data_ptr()
        rc = self.lib.hct_lora_qv_bwd(self.dqkv.ptr, i["x1"].data_ptr(), i["T"].data_ptr(), i["Aq"].data_ptr(), i["Av"].data_ptr(), i["Bq"].data_ptr(),
                                      i["Bv"].data_ptr(), ptr(self.tr["Aq"]), ptr(self.tr["Av"]), ptr(self.tr["Bq"]), ptr(self.tr["Bv"]), c.B, c.N, c.H,
                                      c.dh, c.r, self.code, out["dAq"].ptr, out["dAv"].ptr, out["dBq"].ptr, out["dBv"].ptr, out["dx1"].ptr,
                                      self.ws.data_ptr(), self.ws_bytes, _st())
        _lib.check(rc, "hct_lora_qv_bwd " + c.name)
        torch.cuda.synchronize()
        assert bool((self.ws[self.ws_bytes:] == 0xA5).all()), f"{c.name}: the bytes after the workspace were written"
        return out


def _check(case, gen, inst, name, framed, want64, allow, bf16_out, fails, report):
    """Margins, finiteness, bit equality (integers) or the per-element bound (gaussian).  Appends texts to `fails`."""
    if not framed.margins_intact():
        fails.append(f"{case.name}/{gen}: {name}: an element outside the buffer was written")
    got = framed.view.cpu()
    want64 = want64.reshape(got.shape)
    flat = lambda t: t.reshape(-1, t.shape[-1])
    s = STATS.setdefault((_name(inst), name), [0.0, 0, 0])
    if not bool(torch.isfinite(got).all()):
        fails.append(f"{case.name}/{gen}: {name}: not finite at {(~torch.isfinite(got)).nonzero()[0].tolist()} ({_name(inst)})")
        return
    if gen == "integers":
        want = K.stored(want64, 1 if bf16_out else 0)
        equal = torch.equal(got, want)
        s[1] += int(equal)
        s[2] += 1
        if not equal:
            at = (got != want).nonzero()[0].tolist()
            fails.append(f"{case.name}/integers: {name} differs in {int((got != want).sum())} elements, first at {at} ({_name(inst)}): "
                         f"got {float(got[tuple(at)])}, exact {float(want64[tuple(at)])}")
    else:
        ratio, row, col = K.worst(flat(got.double()), flat(want64), flat(allow.reshape(got.shape)))
        s[0] = max(s[0], ratio)
        report[name] = max(report.get(name, 0.0), ratio)
        if not ratio <= 1.0:
            fails.append(f"{case.name}/gaussian: {name} |err| / bound = {ratio:.3f} at flat row {row}, column {col} ({_name(inst)}): "
                         f"got {float(flat(got)[row, col])!r}, exact {float(flat(want64)[row, col])!r}")


def _check_forward(case, gen, d, out, fails, report):
    """T against exact and its bound; qkv against the value and the bound that follow from the DEVICE's T; the k slot bit for bit."""
    ex = K.exact(case, d)
    bf16 = case.dtype == "bf16"
    T_dev = out["T"].view.cpu().double()
    _check(case, gen, case.fwd_instance, "T", out["T"], ex["T"], K.bound(case, d, ex)["T"] if gen == "gaussian" else None, bf16, fails, report)
    if not bool(torch.isfinite(T_dev).all()):
        return
    _check(case, gen, case.fwd_instance, "qkv", out["qkv"], K.scatter(case, d, T_dev), K.bound_qkv(case, d, T_dev) if gen == "gaussian" else None,
           bf16, fails, report)
    if not torch.equal(_bits(out["qkv"].view[:, :, 1].cpu().contiguous()), _bits(d["qkv"][:, :, 1].to(K.torch_dtype(case)).contiguous())):
        fails.append(f"{case.name}/{gen}: the k slot changed")


@pytest.mark.parametrize("gen", ["integers", "gaussian"])
@pytest.mark.parametrize("case", K.CASES, ids=lambda c: c.name)
def test_forward(lib, cuda, case, gen):
    """hct_lora_qv_fwd: T per element, the q and v slots per element from the device's own T, the k slot bit-equal to its input,
    margins untouched; on `integers` everything bit-equal to exact.  The case whose qkv base is 8 bytes off a 16-byte boundary also
    runs aligned: same T bits, the aligned qkv inside the same bound, and on `integers` the same bits."""
    d = K.make_data(case, gen)
    fails, report = [], {}
    out = Call(lib, cuda, case, d).forward()
    _check_forward(case, gen, d, out, fails, report)
    if case.qkv_off:
        twin = dataclasses.replace(case, qkv_off=0)
        assert twin.fwd_instance[0] == "mfma" and case.fwd_instance == ("generic",)
        out2 = Call(lib, cuda, twin, d).forward()
        _check_forward(twin, gen, d, out2, fails, report)
        if not torch.equal(_bits(out["T"].view), _bits(out2["T"].view)):
            fails.append(f"{case.name}/{gen}: T differs between the aligned and the unaligned call")
        if gen == "integers" and not torch.equal(_bits(out["qkv"].view), _bits(out2["qkv"].view)):
            fails.append(f"{case.name}/integers: qkv differs between the aligned and the unaligned call")
    print(f"lora fwd {case.name}/{gen} {_name(case.fwd_instance)}: worst |err| / bound", {k: round(v, 4) for k, v in report.items()})
    assert not fails, f"{len(fails)} failures:\n" + "\n".join(fails[:20])


@pytest.mark.parametrize("gen", ["integers", "gaussian"])
@pytest.mark.parametrize("case", K.CASES, ids=lambda c: c.name)
def test_backward(lib, cuda, case, gen):
    """hct_lora_qv_bwd on two dx1 bases (zeros, dx0): dAq, dAv, dBq, dBv and dx1 per element against the float64 chain (dU and dT
    are never read out of the workspace); gradients NaN beforehand; on `integers` everything bit-equal."""
    d = K.make_data(case, gen)
    ex = K.exact(case, d)
    allow = K.bound(case, d, ex) if gen == "gaussian" else None
    call = Call(lib, cuda, case, d)
    fails, report = [], {}
    for base, key in ((torch.zeros_like(d["dx0"]), "inc"), (d["dx0"], "dx1")):
        out = call.backward(base)
        for k in GRADS:
            _check(case, gen, case.bwd_instance, k, out[k], ex[k], allow[k] if allow else None, False, fails, report)
        _check(case, gen, case.bwd_instance, "dx1", out["dx1"], ex[key], allow[key] if allow else None, case.dtype == "bf16", fails, report)
    print(f"lora bwd {case.name}/{gen} {_name(case.bwd_instance)}: worst |err| / bound", {k: round(v, 4) for k, v in report.items()})
    assert not fails, f"{len(fails)} failures:\n" + "\n".join(fails[:20])


GATHER_CASES = (K.Case("gather-2x37x3x64", 2, 37, 3, 64, 128), K.Case("gather-1x300x4x16", 1, 300, 4, 16, 128),
                K.Case("gather-2x5x16x4", 2, 5, 16, 4, 128), K.Case("gather-3x1x1x64", 3, 1, 1, 64, 128),
                K.Case("gather-fp32-2x9x3x16", 2, 9, 3, 16, 128, dtype="fp32"), K.Case("gather-fp32-1x131x2x4", 1, 131, 2, 4, 128, dtype="fp32"))


@pytest.mark.parametrize("case", GATHER_CASES, ids=lambda c: c.name)
def test_gather_places_every_block(lib, cuda, case):
    """lora_gather_kernel on its own, shown through dB with a one-hot T: with T[m, j] = 1 exactly where m = m0 + j (in both pairs'
    halves), dB = dU^T . T holds row m0 + j of dU in its column j, as a sum of one term and zeros: exact in any order, so every
    element of dU is compared BIT for bit, with Gaussian dqkv (no two blocks alike), in chunks of r = 128 rows."""
    d = dict(K.make_data(case, "gaussian"))
    M, D, r = case.M, case.D, case.r
    dU = K.gather(case, d["dqkv"].double()).view(M, 2, D)
    for m0 in range(0, M, r):
        rows = min(r, M - m0)
        T = torch.zeros(M, 2 * r)
        for z in range(2):
            T[m0:m0 + rows, z * r:z * r + rows] = torch.eye(rows)
        d["T"] = T
        out = Call(lib, cuda, case, d).backward(d["dx0"])
        for z, k in enumerate(("dBq", "dBv")):
            want = torch.zeros(D, r, dtype=torch.float64)
            want[:, :rows] = dU[m0:m0 + rows, z].t()
            got = out[k].view.cpu()
            assert out[k].margins_intact()
            assert torch.equal(got, want.float()), (case.name, k, m0, (got != want.float()).nonzero()[0].tolist())


INSTANCES = [("fwd", ("mfma", ks, 1)) for ks in (1, 2, 4)] + [("bwd", ("mfma", ks, 2)) for ks in (1, 2, 4)] + [("fwd", ("generic",)), ("bwd", ("generic",))]


@pytest.mark.parametrize("which,inst", INSTANCES, ids=lambda v: v if isinstance(v, str) else _name(v).replace(",", "-"))
def test_second_call_is_bit_identical(lib, cuda, which, inst):
    """Two calls on the same inputs: every output (and every margin) has the same bits.  Once per instance, at the first case of the
    table past one workgroup's rows that reaches it (the generic kernel: the first that reaches it)."""
    pick = [c for c in K.CASES if (c.fwd_instance if which == "fwd" else c.bwd_instance) == inst]
    case = next((c for c in pick if c.M > K.KROWS_WG), pick[0])
    d = K.make_data(case, "gaussian")
    call = Call(lib, cuda, case, d)
    a, b = (call.forward(), call.forward()) if which == "fwd" else (call.backward(d["dx0"]), call.backward(d["dx0"]))
    for k in a:
        assert torch.equal(_bits(a[k].flat), _bits(b[k].flat)), (case.name, k)


def test_refusals_touch_nothing(lib, cuda):
    """Each returns non-zero, names its reason in hct_last_error_string and leaves every output buffer bit-unchanged."""
    case = K.Case("refuse", 2, 9, 2, 64, 64)
    d = K.make_data(case, "gaussian")
    call = Call(lib, cuda, case, d)
    i, tr, c = call.inp, call.tr, case
    p = lambda t: t.data_ptr()

    def outputs():
        o = {k: Framed((c.r, c.D) if k[1] == "A" else (c.D, c.r), torch.float32, cuda) for k in GRADS}
        o["dx1"] = Framed((c.M, c.D), call.td, cuda, fill=d["dx0"])
        o["T"] = Framed((c.M, 2 * c.r), call.td, cuda)
        o["qkv"] = Framed((c.B, c.N, 3, c.H, c.dh), call.td, cuda, fill=d["qkv"])
        return o

    def fwd_args(o, **over):
        a = dict(x1=p(i["x1"]), Aq=p(i["Aq"]), Av=p(i["Av"]), Bq=p(i["Bq"]), Bv=p(i["Bv"]), B=c.B, N=c.N, H=c.H, dh=c.dh, r=c.r, dtype=call.code,
                 T=o["T"].ptr, qkv=o["qkv"].ptr)
        a.update(over)
        return list(a.values()) + [_st()]

    def bwd_args(o, **over):
        a = dict(dqkv=call.dqkv.ptr, x1=p(i["x1"]), T=p(i["T"]), Aq=p(i["Aq"]), Av=p(i["Av"]), Bq=p(i["Bq"]), Bv=p(i["Bv"]), AqT=p(tr["Aq"]),
                 AvT=p(tr["Av"]), BqT=p(tr["Bq"]), BvT=p(tr["Bv"]), B=c.B, N=c.N, H=c.H, dh=c.dh, r=c.r, dtype=call.code, dAq=o["dAq"].ptr,
                 dAv=o["dAv"].ptr, dBq=o["dBq"].ptr, dBv=o["dBv"].ptr, dx1=o["dx1"].ptr, workspace=p(call.ws), workspace_bytes=call.ws_bytes)
        a.update(over)
        return list(a.values()) + [_st()]

    refusals = [("fwd", f"null {k}", {k: None}, b"null argument") for k in ("x1", "Aq", "Av", "Bq", "Bv", "T", "qkv")]
    refusals += [("bwd", f"null {k}", {k: None}, b"null argument")
                 for k in ("dqkv", "x1", "T", "Aq", "Av", "Bq", "Bv", "dAq", "dAv", "dBq", "dBv", "dx1", "workspace")]
    refusals += [("bwd", "a short workspace", dict(workspace_bytes=call.ws_bytes - 1), b"workspace too small"),
                 ("bwd", "no workspace bytes", dict(workspace_bytes=0), b"workspace too small"),
                 ("bwd", "AqT without AvT", dict(AvT=None), b"come in pairs"), ("bwd", "AvT without AqT", dict(AqT=None), b"come in pairs"),
                 ("bwd", "BqT without BvT", dict(BvT=None), b"come in pairs"), ("bwd", "BvT without BqT", dict(BqT=None), b"come in pairs")]
    for which in ("fwd", "bwd"):
        refusals += [(which, "dh % 4 != 0", dict(dh=6), b"multiple of 4"), (which, "r = 0", dict(r=0), b"multiple of 32"),
                     (which, "r = 48", dict(r=48), b"multiple of 32")]
    assert call.ws_bytes > 0
    for which, what, over, reason in refusals:
        o = outputs()
        before = {k: _bits(f.flat).clone() for k, f in o.items()}
        rc = lib.hct_lora_qv_fwd(*fwd_args(o, **over)) if which == "fwd" else lib.hct_lora_qv_bwd(*bwd_args(o, **over))
        torch.cuda.synchronize()
        assert rc != 0, (which, what)
        assert reason in lib.hct_last_error_string(), (which, what, lib.hct_last_error_string())
        for k, f in o.items():
            assert torch.equal(_bits(f.flat), before[k]), f"{which}: {what}: {k} was written"
    assert bool((call.ws == 0xA5).all()), "a refused call wrote into the workspace"
