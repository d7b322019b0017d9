"""float64 numpy restatement of hct_affine_labels (include/headct_hip.h) and the set of voxels where fp32 may decide otherwise.

Conventions are those of tests/affine_ref.py: mat [B, 12] = rows of [A | t], the map from output to input voxel coordinates about
c = (S - 1) / 2; for output index i (axis 0 slowest) p = i - c and q = A p + t + c.  The label at i is labels[n] with
n_a = floor(q_a + 0.5) (a tie goes up) where every axis has -0.5 <= q_a < S - 0.5, and `outside` elsewhere.  A sample with fire 0 is
flips(labels) with flip's bits (bit a = spatial axis a); where it fires the flips are folded into A and `flip` is not looked at.

`delta(mat, S)`: how far the kernel's fp32 coordinate can lie from the float64 one.  The header fixes
q_a = fma(A_a2, p_2, fma(A_a1, p_1, fma(A_a0, p_0, t_a + c))) with p exact: 4 roundings (the sum t_a + c and three fused
multiply-adds), each at most u = 2^-24 times a partial sum, and every partial sum is at most m_a = sum_k |A_ak| |p_k| + |t_a| + c in
magnitude up to a factor (1 + u)^3.  One more unit covers those second-order terms, as in affine_ref: KQ = 4 + 1 = 5, the same count.
Everything the kernel does after q is exact on the fp32 value: floor(q), the fraction q - floor(q) for q >= 0 (for q in [-0.5, 0) the
answer is voxel 0 however q + 1 rounds), the two comparisons of the inside test.  So the kernel's index can differ from the float64
one only where q + 0.5 is within delta_a = KQ u m_a of an integer, and its inside test only where q is within delta_a of -0.5 or of
S - 0.5 (both are such integers of q + 0.5: the second set is part of the first).  `near_tie` is that mask; `candidates` lists what
the kernel may then give."""
import itertools

import numpy as np

from tests.affine_ref import KQ, U


def coords(mat, S):
    """q [B, S, S, S, 3] float64 and m [B, S, S, S, 3] = sum_k |A_ak| |p_k| + |t_a| + c (affine_ref._coords in numpy)."""
    m = np.asarray(mat, dtype=np.float64).reshape(-1, 3, 4)
    A, t = m[:, :, :3], m[:, :, 3]
    c = (S - 1) / 2
    r = np.arange(S, dtype=np.float64) - c
    p = np.stack(np.meshgrid(r, r, r, indexing="ij"), axis=-1)  # [S, S, S, 3]
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.einsum("bak,xyzk->bxyza", A, p) + (t + c)[:, None, None, None, :]
        mag = np.einsum("bak,xyzk->bxyza", np.abs(A), np.abs(p)) + (np.abs(t) + c)[:, None, None, None, :]
    return q, mag


def delta(mat, S):
    """[B, S, S, S, 3]: the distance the kernel's fp32 q_a may have from the float64 one (the derivation is in the module text)."""
    return KQ * U * coords(mat, S)[1]


def flip_plain(labels, flip):
    out = np.array(labels, copy=True)
    for b in range(out.shape[0]):
        axes = [a for a in range(3) if flip is not None and (int(flip[b]) >> a) & 1]
        if axes:
            out[b] = np.flip(out[b], axis=axes)
    return out


def nearest(q, S):
    """(n int64 clamped to [0, S - 1], inside bool over the three axes) of q [..., 3]; a NaN is outside."""
    with np.errstate(invalid="ignore"):
        ok = (q >= -0.5) & (q < S - 0.5)
    n = np.floor(np.where(ok, q, 0.0) + 0.5).astype(np.int64)
    return np.clip(n, 0, S - 1), ok.all(axis=-1)


def affine_labels_ref(labels, mat, fire=None, flip=None, outside=0):
    """labels uint8 [B, S, S, S] (the batch after the gather), mat [B, 12] or None, fire / flip [B] or None -> uint8 [B, S, S, S]."""
    labels = np.asarray(labels, dtype=np.uint8)
    B, S = labels.shape[0], labels.shape[1]
    out = flip_plain(labels, flip)
    if mat is None:
        return out
    mat = np.asarray(mat, dtype=np.float64).reshape(B, 12)
    for b in range(B):
        if fire is not None and not int(fire[b]):
            continue
        n, inside = nearest(coords(mat[b:b + 1], S)[0][0], S)
        out[b] = np.where(inside, labels[b][n[..., 0], n[..., 1], n[..., 2]], np.uint8(outside))
    return out


def near_tie(mat, S, delta):
    """bool [B, S, S, S]: some axis has q + 0.5 within `delta` (a number or [B, S, S, S, 3]) of an integer, or q within `delta` of
    -0.5 or S - 0.5 (which are such integers; stated for the record).  A non-finite q is no tie: it is outside on either side."""
    q, _ = coords(mat, S)
    with np.errstate(invalid="ignore"):
        h = q + 0.5
        tie = np.abs(h - np.round(h)) <= delta
        tie |= (np.abs(q + 0.5) <= delta) | (np.abs(q - (S - 0.5)) <= delta)
    return (tie & np.isfinite(q)).any(axis=-1)


def candidates(labels_b, mat_b, S, delta_b, outside):
    """The values hct_affine_labels may give at each voxel of ONE firing sample: bool [256, S, S, S], entry [v] set where v is
    `outside` or the label at one of the indices floor(q_a + 0.5 -+ delta_a) per axis (the two candidates; 2^3 combinations) that
    lie in the volume."""
    q = coords(np.asarray(mat_b).reshape(1, 12), S)[0][0]
    d = np.broadcast_to(delta_b, q.shape)
    with np.errstate(invalid="ignore"):
        lo, hi = np.floor(q + 0.5 - d), np.floor(q + 0.5 + d)
    ok = np.zeros((256, S, S, S), dtype=bool)
    ok[int(outside)] = True
    grid = np.indices((S, S, S))
    for pick in itertools.product((0, 1), repeat=3):
        n = np.stack([np.where(pick[a], hi[..., a], lo[..., a]) for a in range(3)], axis=-1)
        valid = (np.isfinite(n) & (n >= 0) & (n <= S - 1)).all(axis=-1)
        idx = np.clip(np.nan_to_num(n), 0, S - 1).astype(np.int64)
        v = labels_b[idx[..., 0], idx[..., 1], idx[..., 2]]
        ok[v[valid], grid[0][valid], grid[1][valid], grid[2][valid]] = True
    return ok
