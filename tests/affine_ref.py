"""float64 restatement of hct_affine_augment (include/headct_hip.h) and a derived per-element bound on the fp32 kernel's error.

`affine_sample(x, mat, shift)`: x [B, C, S, S, S], mat [B, 12] = rows of [A | t], the map from output to input voxel coordinates about
c = (S - 1) / 2: for output index i (axis 0 slowest) p = i - c, q = A p + t + c; trilinear interpolation from the eight voxels around
q, a tap outside [0, S) on any axis contributing zero (grid_sample with align_corners=True and padding_mode="zeros"); + shift[b].

`bound(x, mat, shift)`: |kernel - affine_sample| <= bound per element, with u = 2^-24 (fp32 unit roundoff).  Two parts.

1. Coordinates.  The header fixes q_a = fma(A_a2, p_2, fma(A_a1, p_1, fma(A_a0, p_0, t_a + c))) with p exact: 4 roundings (the sum
   t_a + c and three fused multiply-adds), each at most u times a partial sum, and every partial sum is at most
   m_a = sum_k |A_ak p_k| + |t_a| + c in magnitude (up to a factor (1 + u)^3).  The weight w1 = q - floor(q) is exact except for q in
   (-1/2, 0), where q + 1 rounds by at most 2^-25 <= u c / 3 (c >= 3/2 as S >= 4); this is the same as moving q by that much, and its
   slack covers the second-order terms of the four roundings.  So the kernel interpolates at a point q' with
       |q'_a - q_a| <= d_a = KQ u m_a,   KQ = 4 + 1 = 5.
   The trilinear interpolant of the zero-padded volume is continuous everywhere -- across cell borders and across the volume's
   border -- and inside a cell its derivative along axis a is a convex combination of differences between voxels adjacent along a.
   With d_a < 1 the segment from q to q' stays within the cell of q and its neighbours, voxels [f - 1, f + 2] per axis (f = floor(q)),
   so the value moves by at most sum_a L_a d_a, L_a = the largest |difference| of voxels adjacent along a in that zero-padded block.
   A `floor` that lands on the other side of an integer therefore does not break the bound.  (d_a >= 1, a translation of 1e6 voxels
   and more, gives an infinite bound: such samples are held to exact values by their own test.)
2. Weights and sum.  w0 = 1 - w1 rounds once per axis (w1 is exact as a function of q'): 3 roundings in a tap's weight; the two
   products (w_d0 w_d1) w_d2: 2; acc = fma(w, v, acc) over eight taps from acc = 0: a term goes through at most 8 roundings.  Each is
   relative, so the error is at most g sum_i w_i |v_i|, g = KS u / (1 - KS u), KS = 3 + 2 + 8 = 13, with the weights of the exact
   interpolation at q' -- which is within sum_a L_a d_a of the one at q (| |v| | has the Lipschitz constants of v), hence the factor
   (1 + g) on part 1.  Taps outside the volume are not loaded and add exactly nothing.
The final out = acc + shift[b] rounds once more: u (|ref| + E) with E the sum of parts 1 and 2 (no term where shift is None).
Input voxels (fp16, bf16, fp32) widen to fp32 exactly."""
import itertools

import torch
import torch.nn.functional as F

U = 2.0 ** -24
KQ = 5   # roundings of a coordinate: t + c, three fma, and the rounding of w1 = q - floor(q) counted as a move of q
KS = 13  # roundings of a tap's term: 3 (w0 per axis) + 2 (weight products) + 8 (fma chain)


def _coords(mat, S):
    """q [B, S, S, S, 3] float64 and m [B, S, S, S, 3] = sum_k |A_ak p_k| + |t_a| + c."""
    m64 = mat.double().view(-1, 3, 4)
    A, t = m64[:, :, :3], m64[:, :, 3]
    c = (S - 1) / 2
    r = torch.arange(S, dtype=torch.float64) - c
    p = torch.stack(torch.meshgrid(r, r, r, indexing="ij"), dim=-1)  # [S, S, S, 3]
    q = torch.einsum("bak,xyzk->bxyza", A, p) + (t + c).view(-1, 1, 1, 1, 3)
    mag = torch.einsum("bak,xyzk->bxyza", A.abs(), p.abs()) + (t.abs() + c).view(-1, 1, 1, 1, 3)
    return q, mag


def _cells(q, S):
    """inside [B, S, S, S, 3] (the kernel's test, `q > -1 && q < S`, which a NaN fails), f = floor(q) as int64 (0 where not inside),
    w1 = q - f."""
    inside = (q > -1) & (q < S)
    qs = torch.where(inside, q, torch.zeros_like(q))
    f = qs.floor()
    return inside, f.long(), qs - f


def _taps(x, mat):
    """Yields (weight [B, 1, S, S, S], value [B, C, S, S, S]) for the eight taps; value and weight are 0 where the tap is outside."""
    x = x.double()
    B, C, S = x.shape[:3]
    q, _ = _coords(mat, S)
    inside, f, w1 = _cells(q, S)
    flat = x.reshape(B, C, S * S * S)
    for d in itertools.product((0, 1), repeat=3):
        idx = f + torch.tensor(d)
        ok = (inside & (idx >= 0) & (idx < S)).all(dim=-1)
        w = torch.ones_like(w1[..., 0])
        for a in range(3):
            w = w * (w1[..., a] if d[a] else 1 - w1[..., a])
        idx = idx.clamp(0, S - 1)
        lin = ((idx[..., 0] * S + idx[..., 1]) * S + idx[..., 2]).view(B, 1, -1).expand(B, C, -1)
        v = torch.gather(flat, 2, lin).view(B, C, S, S, S)
        okc = ok.view(B, 1, S, S, S)
        yield torch.where(okc, w.view(B, 1, S, S, S), torch.zeros(())).double(), torch.where(okc, v, torch.zeros((), dtype=torch.float64))


def affine_sample(x, mat, shift=None):
    out = sum(w * v for w, v in _taps(x, mat))
    if shift is not None:
        out = out + shift.double().view(-1, 1, 1, 1, 1)
    return out


def bound(x, mat, shift=None):
    x64 = x.double()
    B, C, S = x64.shape[:3]
    q, mag = _coords(mat, S)
    d = KQ * U * mag                                            # [B, S, S, S, 3]
    far = (d >= 1).any(dim=-1) | ~torch.isfinite(q).all(dim=-1)  # [B, S, S, S]
    # block of the cell: voxels [f - 1, f + 2] per axis of the zero-padded volume; f outside [-2, S]: no voxel within reach
    f = q.nan_to_num(nan=-3.0).clamp(-3, S + 1).floor().long()
    reach = ((f >= -2) & (f <= S)).all(dim=-1)
    fc = f.clamp(-2, S) + 2                                     # start of the block in the volume padded by 3 on every side
    pad = F.pad(x64.reshape(B * C, 1, S, S, S), (3,) * 6)
    part1 = torch.zeros_like(x64)
    lin = ((fc[..., 0] * (S + 3) + fc[..., 1]) * (S + 3) + fc[..., 2]).view(B, 1, -1).expand(B, C, -1)
    for a in range(3):
        diff = pad.diff(dim=2 + a).abs()                        # pair (i, i + 1) along a at index i
        kernel = [4, 4, 4]
        kernel[a] = 3
        La = F.max_pool3d(diff, kernel, stride=1).view(B, C, -1)  # [S + 3]^3 per volume
        La = torch.gather(La, 2, lin).view(B, C, S, S, S)
        part1 += torch.where(reach.view(B, 1, S, S, S), La, torch.zeros(())) * d[..., a].view(B, 1, S, S, S)
    g = KS * U / (1 - KS * U)
    absum = sum(w * v.abs() for w, v in _taps(x, mat))
    err = (1 + g) * part1 + g * absum
    if shift is not None:
        err = err + U * (affine_sample(x, mat, shift).abs() + err)
    return torch.where(far.view(B, 1, S, S, S), torch.full((), float("inf"), dtype=torch.float64), err)


def plain(x, flip=None, shift=None):
    """The arithmetic of hct_gather_augment / hct_augment_volume as fp32: (float)x[flips(i)] + shift[b]."""
    out = x.float().clone()
    for b in range(out.shape[0]):
        dims = [a + 1 for a in range(3) if flip is not None and (int(flip[b]) >> a) & 1]
        if dims:
            out[b] = out[b].flip(dims)
        if shift is not None:
            out[b] = out[b] + shift[b].float()
    return out


def lattice(x, perm, sign, t, shift=None):
    """out[i] = x[q] with q_a = c + sign[a] (i[perm[a]] - c) + t[a] (integers), zero where q leaves the volume: torch indexing on the
    fp32 cast.  x [C, S, S, S]."""
    S = x.shape[-1]
    r = torch.arange(S)
    i = torch.meshgrid(r, r, r, indexing="ij")
    q = [(i[perm[a]] if sign[a] > 0 else S - 1 - i[perm[a]]) + int(t[a]) for a in range(3)]
    ok = (q[0] >= 0) & (q[0] < S) & (q[1] >= 0) & (q[1] < S) & (q[2] >= 0) & (q[2] < S)
    v = x.float()[:, q[0].clamp(0, S - 1), q[1].clamp(0, S - 1), q[2].clamp(0, S - 1)]
    out = torch.where(ok, v, torch.zeros(()))
    return out if shift is None else out + shift


def rotations():
    """The 24 signed axis permutations of determinant +1 as (perm, sign): A[a, perm[a]] = sign[a]."""
    out = []
    for perm in itertools.permutations(range(3)):
        for sign in itertools.product((1, -1), repeat=3):
            A = torch.zeros(3, 3)
            for a in range(3):
                A[a, perm[a]] = sign[a]
            if round(float(torch.det(A))) == 1:
                out.append((perm, sign))
    assert len(out) == 24
    return out


def lattice_mat(perm, sign, t):
    m = torch.zeros(3, 4)
    for a in range(3):
        m[a, perm[a]] = sign[a]
        m[a, 3] = t[a]
    return m.reshape(12)
