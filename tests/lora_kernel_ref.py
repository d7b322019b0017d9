"""CPU-only reference, error bound, generators, dispatch restatement, planted defects and case table for the LoRA kernel tests
(csrc/lora.hip through hct_lora_qv_fwd / hct_lora_qv_bwd_workspace_bytes / hct_lora_qv_bwd).  Imported by
tests/test_lora_kernel_ref_cpu.py (which pins this file to tests/lora_ref.py, to autograd and to its own claims) and
tests/test_lora_kernels_gpu.py (which runs the kernels against it).  Nothing here touches a device.

exact(case, data)   the operations of include/headct_hip.h (the LoRA entries) in float64 on the operands as stored:
                      T = x1 . [Aq; Av]^T;  qkv after the call = old + U at the permuted position (U = T . B^T, k slot unchanged);
                      dU = the inverse gather of dqkv;  dB = dU^T . T;  dT = dU . B;  dA = dT^T . x1;  dx1 = dx0 + dT . A.
                    The permutation is written with explicit indices (`positions`, as tests/lora_ref.lora_positions): block
                    r = n' H + h' of a volume goes to (head r // N, token r % N).  T is an INPUT of the scatter and of the backward
                    (data["T"]: the exact product rounded to the storage dtype; the GPU forward test passes the device's own T).
bound(case, data)   a per-element allowance |got - exact| <= bound, derived term by term from gemm_ref's constants (U23 = 2^-23,
                    U8 = 2^-8), never tuned to a kernel.  With acc(K) = K 2^-23 (K + 1 for fp32 operands, whose products are
                    rounded once more; gemm_ref's accumulation term: K u doubled because the summation order is unspecified) and
                    st = 2^-8 for bf16 storage, 0 for fp32:
                      T      acc(D) |x1||A|^T + st (|T| + that)
                      qkv    from the T it is given: acc(r) |T||B|^T + 2^-23 |old + U| (the one fp32 add) + st (|old + U| + those),
                             at the permuted position; the k slot has no allowance at all (it must be bit-equal to its input)
                      dB     acc(M) |dU|^T |T|                       (fp32 out)
                      dT     (in the workspace, never read here)  bT = acc(D) |dU||B| + st (|dT| + that)
                      dx1    sum_k bT[m, k] |A[k, n]|  +  acc(2r) (|dT| + bT) |A|  +  2^-23 |dx0 + dT A|  +  st (|dx0 + dT A| + those)
                      dA     sum_m bT[m, k] |x1[m, n]|  +  acc(M) (|dT| + bT)^T |x1|     (fp32 out)
make_data           two seeded generators: `gaussian` (operands rounded to the storage dtype, checked element by element against
                    bound) and `integers` (below: every stored value is an integer of magnitude <= 256, exact in bf16, every
                    partial sum in any order is below 2^24: the device must be BIT-equal to exact).
instance(...)       lora.hip::rmw_launch's choice restated: ("mfma", KS, pairs) or ("generic",).
CASES               the table; DEFECTS the planted faults of the CPU file.

The `integers` construction: x1 and the rows of dU (the q and v slots of dqkv, drawn as dU and placed through the permutation)
have 4 entries of +-1 per row, A is uniform in -2..2, B has 8 entries of +-1 per row, the old qkv values, the k slot of dqkv
and dx0 are uniform in -64..64.  Hence |T| <= 8, |U| <= 64, |dT| <= 4 by construction; |old + U| and |dx0 + dT A| <= 256 is
asserted per case from the float64 reference (largest over the table: 98 and 113), and so is that U and the dx1 increment
are non-zero on >= 90 % of their elements.
"""
import dataclasses
import functools
import zlib

import torch

from tests.gemm_ref import U8, U23, stored, worst  # noqa: F401  (stored, worst: used by the two test files)

KROWS_WAVE, KROWS_WG = 256, 1024   # lora.hip: kRowsPerWave, four waves per workgroup


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    B: int
    N: int
    H: int
    dh: int
    r: int
    dtype: str = "bf16"      # "bf16" | "fp32"
    at: bool = True          # the backward gets AqT / AvT
    bt: bool = True          # the backward gets BqT / BvT
    qkv_off: int = 0         # qkv's (and dqkv's) first element past a 16-byte boundary, in elements

    @property
    def M(self):
        return self.B * self.N

    @property
    def D(self):
        return self.H * self.dh

    @property
    def fwd_instance(self):
        return instance(self.dtype, self.D, self.dh, self.r, True, self.qkv_off * (2 if self.dtype == "bf16" else 4) % 16 == 0, scatter=True)

    @property
    def bwd_instance(self):
        return instance(self.dtype, self.D, self.dh, self.r, self.at, True, scatter=False)


def torch_dtype(case):
    return torch.bfloat16 if case.dtype == "bf16" else torch.float32


# ---- the dispatch -----------------------------------------------------------------------------------------------------------------------
def generic_reasons(dtype, D, dh, r, transposed, aligned, scatter=True):
    """Why rmw_launch (lora.hip) would NOT take lora_rmw_mfma_kernel: () means it does.  scatter: U into qkv (PERM, one pair per
    z of the grid; the small matrix B [D, r] is row-major whatever the caller passes, and eight consecutive columns must stay in
    one dh block); otherwise dx1 += dT . A (two pairs; the small matrix has ldb_k = 1 only through the transposed copies, which
    the entry uses for bf16 alone).  `aligned`: the read-modify-written buffer's base is on a 16-byte boundary.  The strides the
    launch also tests (lda = 2r, ldb_n = r, ldc = D multiples of 8) follow from r % 32 == 0 and D % 64 == 0."""
    why = []
    if dtype != "bf16":
        why.append("fp32")
    if D % 64:
        why.append("D % 64")
    if r not in (32, 64, 128):
        why.append("rank")
    if not aligned:
        why.append("alignment")
    if scatter and dh % 8:
        why.append("dh % 8")
    if not scatter and not transposed:
        why.append("no transposed copy")
    return tuple(why)


def instance(dtype, D, dh, r, transposed, aligned, scatter=True):
    if generic_reasons(dtype, D, dh, r, transposed, aligned, scatter):
        return ("generic",)
    return ("mfma", r // 32, 1 if scatter else 2)


# ---- the permutation --------------------------------------------------------------------------------------------------------------------
def positions(N, H):
    """(head, token) that block (n', h') of a volume's U lands on: two [N, H] index tensors, r = n' H + h' -> (r // N, r % N)."""
    head, tok = torch.empty(N, H, dtype=torch.long), torch.empty(N, H, dtype=torch.long)
    for n in range(N):
        for h in range(H):
            r = n * H + h
            head[n, h], tok[n, h] = r // N, r % N
    return head, tok


@functools.lru_cache(maxsize=8)
def _positions(N, H):
    return positions(N, H)


def place(case, V):
    """[B, N, 2, D] in source order (row n', columns h' dh ..) -> [B, N, 3, H, dh] with V at the permuted q / v positions."""
    head, tok = _positions(case.N, case.H)
    out = torch.zeros(case.B, case.N, 3, case.H, case.dh, dtype=V.dtype)
    for z in range(2):
        out[:, tok, 2 * z, head] = V[:, :, z].reshape(case.B, case.N, case.H, case.dh)
    return out


def gather(case, G):
    """The inverse: [B, N, 3, H, dh] -> dU [B, N, 2, D]."""
    head, tok = _positions(case.N, case.H)
    return torch.stack([G[:, tok, 2 * z, head].reshape(case.B, case.N, case.D) for z in range(2)], dim=2)


# ---- generators -------------------------------------------------------------------------------------------------------------------------
def _sparse_pm1(rows, cols, k, g):
    idx = torch.rand(rows, cols, generator=g).argsort(dim=1)[:, :k]
    sign = (torch.randint(0, 2, (rows, k), generator=g) * 2 - 1).float()
    return torch.zeros(rows, cols).scatter_(1, idx, sign)


@functools.lru_cache(maxsize=2)
def _shape_data(gen, B, N, H, dh, r, dtype):
    g = torch.Generator(device="cpu").manual_seed(zlib.crc32(repr((gen, B, N, H, dh, r, dtype)).encode()))
    M, D = B * N, H * dh
    geo = Case("geo", B, N, H, dh, r, dtype)
    if gen == "integers":
        ri = lambda lim, *s: torch.randint(-lim, lim + 1, s, generator=g).float()
        x1 = _sparse_pm1(M, D, 4, g).view(B, N, D)
        dU = _sparse_pm1(M * 2, D, 4, g).view(B, N, 2, D)
        dqkv = place(geo, dU)
        dqkv[:, :, 1] = ri(64, B, N, H, dh)
        t = dict(x1=x1, qkv=ri(64, B, N, 3, H, dh), dqkv=dqkv, dx0=ri(64, B, N, D), Aq=ri(2, r, D), Av=ri(2, r, D),
                 Bq=_sparse_pm1(D, r, 8, g), Bv=_sparse_pm1(D, r, 8, g))
    else:
        rn = lambda *s: torch.randn(*s, generator=g)
        t = dict(x1=rn(B, N, D), qkv=rn(B, N, 3, H, dh), dqkv=rn(B, N, 3, H, dh), dx0=rn(B, N, D), Aq=rn(r, D), Av=rn(r, D),
                 Bq=rn(D, r) * 0.05, Bv=rn(D, r) * 0.05)
    td = torch.bfloat16 if dtype == "bf16" else torch.float32
    t = {k: v.to(td).float() for k, v in t.items()}  # as stored
    T64 = t["x1"].double().view(M, D) @ torch.cat([t["Aq"], t["Av"]]).double().t()
    t["T"] = T64.float().to(td).float()
    t["gen"] = gen
    return t


def make_data(case, gen):
    """Seeded by the geometry, rank and dtype only: a case and its unaligned / untransposed twins share their operands."""
    return _shape_data(gen, case.B, case.N, case.H, case.dh, case.r, case.dtype)


# ---- planted defects --------------------------------------------------------------------------------------------------------------------
# name -> (what it is, outputs that must show it).  "qkv" is asked wherever the forward is an MFMA instance, "dx1" wherever the dx1
# product is, "grads" (any of dAq, dAv, dBq, dBv, dx1) wherever either is.  `applies` states the exclusions.
DEFECTS = {
    "kstep":  ("one k-step of 32 dropped in one 64-column tile", ("qkv", "dx1")),
    "halves": ("the two 4-column halves of one lane's 8 columns swapped", ("qkv", "dx1")),
    "strip":  ("one 16-row strip of one tile left at its old value", ("qkv", "dx1")),
    "tail":   ("the rows of the last partial strip not stored", ("qkv", "dx1")),
    "pairB":  ("pair q's B used for v", ("qkv",)),
    "swap":   ("head and token swapped in the destination for one row (r = h' N + n': the block stays at token n', head h')", ("qkv",)),
    "pair2":  ("the second pair omitted from dx1", ("dx1",)),
    "gather": ("one dh block of dU gathered from the neighbouring block", ("grads",)),
}


def applies(case, defect):
    """False only where the defect changes nothing: no partial strip (M % 16 == 0); H = 1 or N = 1, where r = h' N + n' is r itself;
    one block per volume (N H = 1), which has no neighbour."""
    if defect == "tail":
        return case.M % 16 != 0
    if defect == "swap":
        return case.H > 1 and case.N > 1
    if defect == "gather":
        return case.N * case.H > 1
    return True


def _seed(case, what):
    return zlib.crc32((what + case.name).encode())


def _first(start, n, ok):
    """The first index from a seeded start (cyclically) at which the defect changes something; the place is drawn, not chosen."""
    return next((start + k) % n for k in range(n) if ok((start + k) % n))


def _plant_rmw(case, defect, inc, term):
    """Plant `defect` in an [M, D] increment of a read-modify-write product.  term(cols, ks) is pair 0's contribution of k-step ks
    to the columns `cols`."""
    M, D = inc.shape
    inc = inc.clone()
    tiles, strips = D // 64, (M + 15) // 16
    if defect == "kstep":
        t, s = _seed(case, "kstep-t") % tiles, _seed(case, "kstep-s") % (case.r // 32)
        cols = slice(64 * t, 64 * t + 64)
        inc[:, cols] -= term(cols, s)
    elif defect == "halves":
        n8 = D // 8
        differs = lambda i: bool((inc[i // n8, 8 * (i % n8):8 * (i % n8) + 4] != inc[i // n8, 8 * (i % n8) + 4:8 * (i % n8) + 8]).any())
        i = _first(_seed(case, "halves") % (M * n8), M * n8, differs)
        m, c = i // n8, 8 * (i % n8)
        inc[m, c:c + 8] = torch.cat([inc[m, c + 4:c + 8], inc[m, c:c + 4]])
    elif defect == "strip":
        live = lambda i: bool((inc[16 * (i // tiles):16 * (i // tiles) + 16, 64 * (i % tiles):64 * (i % tiles) + 64] != 0).any())
        i = _first(_seed(case, "strip") % (strips * tiles), strips * tiles, live)
        inc[16 * (i // tiles):16 * (i // tiles) + 16, 64 * (i % tiles):64 * (i % tiles) + 64] = 0.0
    elif defect == "tail":
        inc[M - M % 16:] = 0.0
    return inc


# ---- exact ------------------------------------------------------------------------------------------------------------------------------
def scatter(case, d, T64, defect=None):
    """qkv after the forward, in float64, from the T it is given ([M, 2r])."""
    B, N, H, dh, r, M, D = case.B, case.N, case.H, case.dh, case.r, case.M, case.D
    Bm = [d["Bq"].double(), d["Bv"].double()]
    Tz = [T64[:, :r], T64[:, r:]]
    U = [Tz[z] @ Bm[z].t() for z in range(2)]
    if defect == "pairB":
        U[1] = Tz[1] @ Bm[0].t()
    if defect in ("kstep", "halves", "strip"):  # in pair q
        U[0] = _plant_rmw(case, defect, U[0], lambda cols, s: Tz[0][:, 32 * s:32 * s + 32] @ Bm[0][cols, 32 * s:32 * s + 32].t())
    if defect == "tail":
        U = [_plant_rmw(case, defect, u, None) for u in U]
    U = torch.stack(U, dim=1).view(B, N, 2, D)
    out = d["qkv"].double()
    if defect == "swap":
        # one source row (b0, n0 >= 1) of pair q: its H blocks stay at (token n0, head h') instead of going to (r % N, r // N)
        b0, n0 = _seed(case, "swap-b") % B, 1 + _seed(case, "swap-n") % (N - 1)
        moved = U[b0, n0, 0].clone()
        U = U.clone()
        U[b0, n0, 0] = 0.0
        out = out + place(case, U)
        out[b0, n0, 0] += moved.view(H, dh)
        return out
    return out + place(case, U)


def exact(case, d, defect=None):
    """dict(T [M, 2r], qkv [B, N, 3, H, dh], dAq, dAv [r, D], dBq, dBv [D, r], inc [M, D] = dT . A summed over the pairs,
    dx1 = dx0 + inc) in float64.  `defect` plants one of DEFECTS."""
    assert defect is None or defect in DEFECTS
    B, N, H, dh, r, M, D = case.B, case.N, case.H, case.dh, case.r, case.M, case.D
    x1 = d["x1"].double().view(M, D)
    A = [d["Aq"].double(), d["Av"].double()]
    Bm = [d["Bq"].double(), d["Bv"].double()]
    T = x1 @ torch.cat(A).t()
    Tin = d["T"].double()
    qkv = scatter(case, d, Tin, defect)
    dU = gather(case, d["dqkv"].double())  # [B, N, 2, D]
    if defect == "gather":
        # block (b, n, h) of pair z takes the values of the NEXT block of its volume (the last one: the one before it)
        z = _seed(case, "gather-z") % 2
        blocks = dU[:, :, z].reshape(B, N * H, dh)
        nb = torch.arange(1, N * H + 1)
        nb[-1] = N * H - 2
        differs = (blocks != blocks[:, nb]).any(dim=2).flatten()
        i = _first(_seed(case, "gather") % (B * N * H), B * N * H, lambda j: bool(differs[j]))
        blocks = blocks.clone()
        blocks[i // (N * H), i % (N * H)] = blocks[i // (N * H), nb[i % (N * H)]]
        dU = dU.clone()
        dU[:, :, z] = blocks.view(B, N, D)
    dU = dU.view(M, 2, D)
    dBm = [dU[:, z].t() @ Tin[:, z * r:(z + 1) * r] for z in range(2)]
    dT = [dU[:, z] @ Bm[z] for z in range(2)]
    dA = [dT[z].t() @ x1 for z in range(2)]
    inc = dT[0] @ A[0] + (0.0 if defect == "pair2" else dT[1] @ A[1])
    if defect in ("kstep", "halves", "strip", "tail"):
        inc = _plant_rmw(case, defect, inc, lambda cols, s: dT[0][:, 32 * s:32 * s + 32] @ A[0][32 * s:32 * s + 32, cols])
    return dict(T=T, qkv=qkv, dAq=dA[0], dAv=dA[1], dBq=dBm[0], dBv=dBm[1], inc=inc, dx1=d["dx0"].double().view(M, D) + inc,
                U=qkv - d["qkv"].double(), dT=torch.cat(dT, dim=1))


# ---- bound ------------------------------------------------------------------------------------------------------------------------------
def _acc(case, K):
    return (K + (1 if case.dtype == "fp32" else 0)) * U23


def bound_qkv(case, d, T64):
    """[B, N, 3, H, dh] allowance of the forward's qkv for the T it was computed from; 0 in the k slot."""
    r, st = case.r, U8 if case.dtype == "bf16" else 0.0
    absU = torch.stack([T64[:, z * r:(z + 1) * r].abs() @ d[k].double().abs().t() for z, k in enumerate(("Bq", "Bv"))], dim=1)
    acc = place(case, (_acc(case, r) * absU).view(case.B, case.N, 2, case.D))
    val = scatter(case, d, T64).abs()
    err = acc + U23 * val
    err = err + st * (val + err)
    err[:, :, 1] = 0.0
    return err


def bound(case, d, ex=None):
    """Per-element allowance for T, qkv (for T = data["T"]), dAq, dAv, dBq, dBv, dx1 (base dx0) and inc (base zero)."""
    ex = ex if ex is not None else exact(case, d)
    r, M, D, st = case.r, case.M, case.D, U8 if case.dtype == "bf16" else 0.0
    x1 = d["x1"].double().view(M, D).abs()
    A = [d["Aq"].double().abs(), d["Av"].double().abs()]
    Bm = [d["Bq"].double().abs(), d["Bv"].double().abs()]
    Tin = d["T"].double().abs()
    bT = _acc(case, D) * (x1 @ torch.cat(A).t())
    out = dict(T=bT + st * (ex["T"].abs() + bT), qkv=bound_qkv(case, d, d["T"].double()))
    dU = gather(case, d["dqkv"].double()).view(M, 2, D).abs()
    prop = 0.0      # dT's allowance through dT . A, summed over the pairs
    mag = 0.0       # (|dT| + bdT) |A|
    for z, k in enumerate(("q", "v")):
        out["dB" + k] = _acc(case, M) * (dU[:, z].t() @ Tin[:, z * r:(z + 1) * r])
        dT = ex["dT"][:, z * r:(z + 1) * r].abs()
        bdT = _acc(case, D) * (dU[:, z] @ Bm[z])
        bdT = bdT + st * (dT + bdT)
        out["dA" + k] = bdT.t() @ x1 + _acc(case, M) * ((dT + bdT).t() @ x1)
        prop = prop + bdT @ A[z]
        mag = mag + (dT + bdT) @ A[z]
    for name, base in (("dx1", d["dx0"].double().view(M, D)), ("inc", 0.0)):
        val = (base + ex["inc"]).abs()
        err = prop + _acc(case, 2 * r) * mag + U23 * val
        out[name] = err + st * (val + err)
    return out


OUTPUTS = ("T", "qkv", "dAq", "dAv", "dBq", "dBv", "dx1")


# ---- the case table ---------------------------------------------------------------------------------------------------------------------
# M = B N at the edges of lora_rmw_mfma_kernel: a wave's 16-row strips (1, 15, 16, 17), a wave's 256 rows and a workgroup's 1024
M_EDGES = {1: (1, 1), 15: (3, 5), 16: (2, 8), 17: (1, 17), 255: (3, 85), 256: (1, 256), 257: (1, 257), 1023: (3, 341), 1024: (2, 512),
           1025: (1, 1025)}
EDGE_GEOMETRY = {32: (8, 8), 64: (2, 64), 128: (4, 16)}  # r -> (H, dh): D = 64 (one column tile), 128 (two), 64
# the raw-reshape permutation on the MFMA path (D % 64 == 0): per (H, dh), N = 1, N < H, N > H coprime to H, N a multiple of H, N > H neither
GEOMETRY_N = {(8, 8): (1, 3, 9, 16, 12), (4, 16): (1, 3, 9, 8, 6), (4, 48): (1, 3, 9, 8, 6), (2, 64): (1, 3, 4, 7), (1, 64): (1, 5),
              (1, 128): (1, 5), (3, 64): (1, 2, 4, 6, 7)}


def _cases():
    out = []
    for r, (H, dh) in EDGE_GEOMETRY.items():  # both MFMA instances of KS = r / 32 at every edge
        for M, (B, N) in M_EDGES.items():
            out.append(Case(f"edge-r{r}-M{M}-{B}x{N}x{H}x{dh}", B, N, H, dh, r))
    i = 0
    for (H, dh), Ns in GEOMETRY_N.items():
        for N in Ns:
            r = (32, 64, 128)[i % 3]
            i += 1
            out.append(Case(f"geo-{2}x{N}x{H}x{dh}-r{r}", 2, N, H, dh, r))
    out.append(Case("vitb-2x513x12x64-r128", 2, 513, 12, 64, 128))  # the old test's D = 768 shape
    # the generic kernel, reason by reason
    for r, (B, N, H, dh) in {32: (3, 9, 3, 16), 64: (2, 37, 2, 64), 96: (1, 17, 2, 32), 128: (2, 11, 3, 16)}.items():
        out.append(Case(f"fp32-r{r}-{B}x{N}x{H}x{dh}", B, N, H, dh, r, dtype="fp32"))
    out.append(Case("bf16-D48-3x9x3x16-r32", 3, 9, 3, 16, 32))
    out.append(Case("bf16-D48-2x11x3x16-r128", 2, 11, 3, 16, 128))
    out.append(Case("bf16-r96-2x37x2x64", 2, 37, 2, 64, 96))
    out.append(Case("bf16-dh4-2x5x16x4-r32", 2, 5, 16, 4, 32))  # dh % 8 != 0: the scatter is generic, the dx1 product is not
    out.append(Case("bf16-noAT-3x37x2x64-r64", 3, 37, 2, 64, 64, at=False))             # dx1 product with ldb_k = D
    out.append(Case("bf16-noBT-3x37x2x64-r64", 3, 37, 2, 64, 64, bt=False))             # dt_product with transB = 0
    out.append(Case("bf16-noT-3x37x2x64-r64", 3, 37, 2, 64, 64, at=False, bt=False))
    out.append(Case("bf16-qkvoff-3x37x2x64-r64", 3, 37, 2, 64, 64, qkv_off=4))          # qkv 8 bytes off a 16-byte boundary
    out.append(Case("bf16-aligned-3x37x2x64-r64", 3, 37, 2, 64, 64))                    # the four above with nothing taken away
    return tuple(out)


CASES = _cases()  # (make_data ignores at / bt / qkv_off: the last five share their operands)


def mfma_cases():
    return [c for c in CASES if c.fwd_instance[0] == "mfma" or c.bwd_instance[0] == "mfma"]
