"""Reference for the native-grid segmentation path (headct_foundation_amd/native.py, csrc/native.hip): the per-axis tables and
blend + arg-max restated in float64 from their definition (issue text / include/headct_hip.h), the geometries and inputs of the
tests, and the bound on the fp32 blend's error.  Nothing here needs a GPU, and nothing here calls native.native_tables.

The bound E.  The kernel blends with 7 lerps, three deep: r = fl(a + fl(w * fl(b - a))), fp32, no contraction, w in [0, 1] exact
(the table's own fp32 value, which the reference widens), |a|, |b| <= M.  With u = 2^-24:
    d = fl(b - a):  |d| <= 2 M,               rounding error <= 2 M u
    p = fl(w d):    |p| <= 2 M,               rounding error <= 2 M u, plus w * (error of d) <= 2 M u
    r = fl(a + p):  |r| <= M (1 + 5 u),       rounding error <= M u (1 + 5 u)
so one lerp of exact inputs errs by at most 5 M u (1 + u), and since a lerp is a convex combination, input errors e pass through as at
most e.  Three levels: 15 M u (1 + O(u)); the inputs themselves are exact (fp32, or bf16 widened).  E = 16 M u covers it with the
growth of M by (1 + 5 u) per level.  The arg-max can differ from float64's only where the top-2 margin is at most 2 E.
"""
import itertools

import numpy as np
import torch

from headct_foundation_amd import nifti
from headct_foundation_amd.native import ScanGeometry
from tests import seg_ref

U = 2.0 ** -24
NEAR_TIE_CAP = 1e-3  # share of a case's voxels the test may leave out as near-ties
P, G = 2, 3
S = P * G
CLASSES = (2, 3, 5, 16)


def blend_error_bound(max_abs: float) -> float:
    return 16.0 * U * float(max_abs)


# ---- geometries -----------------------------------------------------------------------------------------------------------------------
def make_geom(file_shape, perm, flip, zooms, box="inner") -> ScanGeometry:
    """A geometry from the file shape (ni, nj, nk), perm / flip to RAS, the voxel size per RAS axis and a box: "full" (the volume),
    "inner" (one resampled voxel off every face: outside voxels on both sides of every axis), "one0" .. "one2" (size 1 on that RAS axis,
    inner elsewhere)."""
    d = [file_shape[perm[o]] for o in range(3)]
    gm = [nifti.spacing_geometry(d[o], zooms[o]) for o in range(3)]
    m, steps = [g[0] for g in gm], [g[1] for g in gm]
    if box == "full":
        start, size = [0, 0, 0], list(m)
    else:
        start = [1 if m[o] > 2 else 0 for o in range(3)]
        size = [m[o] - 2 if m[o] > 2 else m[o] for o in range(3)]
        if box.startswith("one"):
            o = int(box[3])
            start[o], size[o] = m[o] // 2, 1
    affine = np.eye(4)
    return ScanGeometry(tuple(file_shape), tuple(perm), tuple(flip), d, m, steps, affine, start, size)


def identity_geom(n: int = S) -> ScanGeometry:
    return make_geom((n, n, n), (0, 1, 2), (False, False, False), (1.0, 1.0, 1.0), "full")


ZOOMS = (0.45, 1.0, 5.0)  # steps 2.2 (a 0.45 mm axis), 1, 0.2 (a 5 mm axis)


def geometries() -> dict:
    """name -> ScanGeometry: each of the 6 perms with some flip, all 8 flip patterns on one perm, file shapes (13, 9, 7) and (7, 13, 9),
    boxes inner / full / size one on an axis."""
    out = {}
    boxes = ("inner", "full", "one0", "one1", "one2")
    for n, perm in enumerate(itertools.permutations(range(3))):
        flip = tuple(bool((n + 1) >> o & 1) for o in range(3))
        shape = (13, 9, 7) if n % 2 == 0 else (7, 13, 9)
        zooms = tuple(ZOOMS[(o + n) % 3] for o in range(3))
        out[f"perm{''.join(map(str, perm))}"] = make_geom(shape, perm, flip, zooms, boxes[n % len(boxes)])
    for code in range(8):
        flip = tuple(bool(code >> o & 1) for o in range(3))
        out[f"flip{code}"] = make_geom((13, 9, 7), (1, 2, 0), flip, ZOOMS, boxes[(code + 1) % len(boxes)])
    return out


def long_geometries() -> dict:
    """A row past any one block's trip, 1024 slices of one voxel pair, and 40 rows j in a slice: the kernel hands 16 consecutive rows of a
    slice to a workgroup, so these are three of them, the last one partial, under a flip on j (item rows met in descending order)."""
    return {"long_i": make_geom((1024, 2, 2), (0, 1, 2), (True, False, False), (0.45, 1.0, 1.0), "inner"),
            "long_k": make_geom((2, 2, 1024), (2, 1, 0), (False, False, True), (0.45, 1.0, 1.0), "inner"),
            "wide_j": make_geom((5, 40, 3), (1, 0, 2), (True, False, False), (0.45, 1.0, 1.0), "inner")}


def dyadic_geometries() -> dict:
    """Geometries whose linear weights are dyadic (exact in fp32, and exact blends of small integers): steps 1 with a full box of n
    voxels onto R = 6: t = (f + 0.5) * 6 / n - 0.5 with n = 12 (weights k/4), n = 3 (k/2), n = 6 (0) and n = 24 (k/8)."""
    return {"dy_12_3_6": make_geom((12, 3, 6), (0, 1, 2), (False, True, False), (1.0, 1.0, 1.0), "full"),
            "dy_24_6_12": make_geom((6, 12, 24), (2, 0, 1), (True, False, True), (1.0, 1.0, 1.0), "full")}


# ---- tables, from the definition -------------------------------------------------------------------------------------------------------
def axis_coordinate(geom, a: int, R: int, fault=None):
    """(t float64 [n_a], inside bool [n_a]) of file axis a: the item coordinate before any clamp.  `fault` plants one: "no_flip" leaves
    the flip out, "no_half" drops the + 0.5, "no_start" ignores the box start."""
    o = list(geom.perm).index(a)
    n = geom.file_shape[a]
    t, inside = np.empty(n, np.float64), np.empty(n, bool)
    for f in range(n):
        r = geom.d[o] - 1 - f if (geom.flip[o] and fault != "no_flip") else f
        u = np.float64(r) / np.float64(geom.steps[o])
        c = u - (0 if fault == "no_start" else geom.start[o])
        inside[f] = -0.5 <= c < geom.size[o] - 0.5
        t[f] = (c + (0.0 if fault == "no_half" else 0.5)) * R / geom.size[o] - 0.5
    return t, inside


def tables(geom, R=S, interp: str = "linear", fault=None) -> list:
    """R: the item's side, or its three sides by RAS axis."""
    R3 = [R] * 3 if isinstance(R, int) else list(R)
    out = []
    for a in range(3):
        R = R3[list(geom.perm).index(a)]
        t, inside = axis_coordinate(geom, a, R, fault)
        if interp == "linear":
            t = np.minimum(np.maximum(t, 0.0), R - 1.0)
            i0 = np.floor(t)
            i1 = np.minimum(i0 + 1, R - 1)
            w = (t - i0).astype(np.float32)
        else:
            i0 = i1 = np.minimum(np.maximum(np.floor(t + 0.5), 0), R - 1)
            w = np.zeros(t.size, np.float32)
        out.append({"i0": i0.astype(np.int32), "i1": i1.astype(np.int32), "w": w, "inside": inside.astype(np.uint8)})
    return out


def tables_equal(a, b) -> bool:
    return all(np.array_equal(x[k], y[k]) and x[k].dtype == y[k].dtype for x, y in zip(a, b) for k in ("i0", "i1", "w", "inside"))


# ---- blend + arg-max ---------------------------------------------------------------------------------------------------------------------
def blend(vol: np.ndarray, tabs, perm) -> tuple:
    """(values float64 [K, nk, nj, ni], inside bool [nk, nj, ni]): vol float64 [K, R, R, R] (item axes = RAS axes) blended at every
    file voxel with the tables' own weights (fp32, widened)."""
    x = np.asarray(vol, np.float64)
    inv = [list(perm).index(a) for a in range(3)]
    for o in range(3):
        t = tabs[perm[o]]
        a, b = np.take(x, t["i0"], axis=1 + o), np.take(x, t["i1"], axis=1 + o)
        shape = [1, 1, 1, 1]
        shape[1 + o] = -1
        x = a + t["w"].astype(np.float64).reshape(shape) * (b - a)
    order = (0, 1 + inv[2], 1 + inv[1], 1 + inv[0])  # [K, RAS axes] -> [K, k, j, i]
    ins = [tabs[a]["inside"].astype(bool) for a in range(3)]
    inside = ins[2][:, None, None] & ins[1][None, :, None] & ins[0][None, None, :]
    return np.ascontiguousarray(x.transpose(order)), inside


def predict(values: np.ndarray, inside: np.ndarray) -> np.ndarray:
    """int16 [nk, nj, ni]: the arg-max (numpy's: the first maximum, so the lowest class wins a tie) inside, 0 outside."""
    return np.where(inside, np.argmax(values, axis=0), 0).astype(np.int16)


def near_ties(values: np.ndarray, inside: np.ndarray, max_abs: float) -> np.ndarray:
    """bool [nk, nj, ni]: inside voxels whose float64 top-2 margin is at most 2 E."""
    top = np.sort(values, axis=0)
    return inside & ((top[-1] - top[-2]) <= 2.0 * blend_error_bound(max_abs))


def counts(pred: np.ndarray, y: np.ndarray, K: int) -> np.ndarray:
    """int64 [K, 3] = TP, FP, FN over the valid voxels (seg_ref.counts for one sample)."""
    return seg_ref.counts(torch.from_numpy(pred.astype(np.int64))[None], torch.from_numpy(y.astype(np.int64))[None], K)[0]


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
def gaussian_volume(K: int, seed: int, bf16: bool) -> torch.Tensor:
    """float64 [K, S, S, S], std 1; rounded to bf16 for the bf16 cases, so that the stored logits are the reference's inputs."""
    v = torch.randn(K, S, S, S, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)
    return (v.to(torch.bfloat16) if bf16 else v).to(torch.float64)


def integer_volume(K: int, seed: int) -> torch.Tensor:
    """float64 [K, S, S, S] of integers in [-2, 2] (ties everywhere) with one item row where every class ties."""
    v = torch.randint(-2, 3, (K, S, S, S), generator=torch.Generator().manual_seed(seed)).to(torch.float64)
    v[:, 0, 0, :] = 1.0
    return v


def token_rows(vol: torch.Tensor, first: int, pad: int, dtype) -> torch.Tensor:
    """[T, K * P^3 + pad] of `dtype`: the volume in token layout, NaN in the leading rows and the pad columns."""
    K = vol.shape[0]
    T, N = first + G ** 3, K * P ** 3
    tok = torch.full((T, N + pad), float("nan"), dtype=torch.float64)
    tok[:, :N] = seg_ref.patchify(vol[None], first, T, G, P)[0]
    tok[:first] = float("nan")
    return tok.to(dtype)


def case_params(index: int) -> dict:
    """K, first and pad of the index-th geometry: K through {2, 3, 5, 16}, first through {0, 2}, ld above K * P^3 always."""
    return {"K": CLASSES[index % 4], "first": (0, 2)[(index // 2) % 2], "pad": (3, 8)[index % 2]}


def gaussian_cases() -> list:
    """(name, geom, K, first, pad, bf16, seed) of the Gaussian-logit cases: every geometry, fp32 and bf16."""
    out = []
    named = list(geometries().items()) + list(long_geometries().items())
    for n, (name, geom) in enumerate(named):
        for bf16 in (False, True):
            p = case_params(n + int(bf16))
            out.append((f"{name}-{'bf16' if bf16 else 'fp32'}", geom, p["K"], p["first"], p["pad"], bf16, 100 + 2 * n + int(bf16)))
    return out


def planted_labels(shape, K: int, seed: int) -> np.ndarray:
    """uint8 labels in file order with 255 planted at about 15 % of the voxels."""
    gen = np.random.default_rng(seed)
    y = gen.integers(0, K, shape).astype(np.uint8)
    y[gen.random(shape) < 0.15] = 255
    return y
