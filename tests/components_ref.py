"""Oracle of the connected-component kernels (csrc/components.hip, headct_foundation_amd/components.py): scipy.ndimage.label with
generate_binary_structure(3, 1 | 2 | 3), numpy restatements of sizes, overlap, small-component removal, recount and lesion_metrics, a
vectorised numpy union-find labeller with switches for planted faults (what a wrong kernel would do), and the case builders of both
test files.  Volumes are [nk, nj, ni]; a tile T = (tk, tj, ti) is what one workgroup would label locally (hct_cc_tile_dims)."""
import itertools

import numpy as np
from scipy import ndimage

RANK = {6: 1, 18: 2, 26: 3}
DIRECTIONS = [d for d in itertools.product((-1, 0, 1), repeat=3) if d > (0, 0, 0)]  # the 13 neighbours that come later in memory
AXIS_LIMIT = 32768


def allowed(d, connectivity) -> bool:
    return sum(1 for x in d if x) <= RANK[connectivity]


def label_ref(mask, connectivity):
    lab, n = ndimage.label(np.asarray(mask, bool), structure=ndimage.generate_binary_structure(3, RANK[connectivity]))
    return lab.astype(np.int32), int(n)


def root_form(mask, connectivity):
    """0 off the mask, 1 + the smallest linear index of the voxel's component on it: hct_cc_label's output."""
    lab, n = label_ref(mask, connectivity)
    first = np.zeros(n + 1, np.int64)
    flat = lab.reshape(-1)
    idx = np.flatnonzero(flat)
    first[flat[idx][::-1]] = idx[::-1]  # the last write of a label is its first voxel
    return np.where(lab > 0, first[lab] + 1, 0).astype(np.int32)


def masks(pred, labels, c):
    if labels is None:
        return pred == c, np.zeros(pred.shape, bool)
    return (pred == c) & (labels != 255), labels == c


def flags_of(pred, labels, c):
    P, G = masks(pred, labels, c)
    return P.astype(np.uint8) | (G.astype(np.uint8) << 1)


def sizes_ref(lab, n):
    return np.bincount(lab.reshape(-1), minlength=n + 1).astype(np.int64) * (np.arange(n + 1) > 0)


def overlap_ref(lab, n, other):
    return np.bincount(lab.reshape(-1), weights=np.asarray(other, bool).reshape(-1), minlength=n + 1).astype(np.int64) * (np.arange(n + 1) > 0)


def recount_ref(pred, labels, K):
    """class_voxels [K] over the whole grid; counts [K, 3] = TP, FP, FN over the voxels whose label is < K (None without labels)."""
    cv = np.array([(pred == c).sum() for c in range(K)], np.int64)
    if labels is None:
        return cv, None
    ok = labels < K
    cn = np.array([[((pred == c) & (labels == c) & ok).sum(), ((pred == c) & (labels != c) & ok).sum(), ((pred != c) & (labels == c) & ok).sum()]
                   for c in range(K)], np.int64)
    return cv, cn


def remove_small_ref(pred, K, min_voxels, connectivity, labels=None):
    out, removed = pred.copy(), np.zeros(K, np.int64)
    if min_voxels > 1:
        for c in range(1, K):
            lab, n = label_ref(out == c, connectivity)  # the annotation plays no part
            small = sizes_ref(lab, n) < min_voxels
            small[0] = False
            out[small[lab]] = 0
            removed[c] = int(small.sum())
    cv, cn = recount_ref(out, labels, K)
    return {"pred": out, "class_voxels": cv, "counts": cn, "removed": removed}


def lesion_metrics_ref(pred, labels, K, connectivity):
    out = {k: np.zeros(K, np.int64) for k in ("n_gt", "n_pred", "gt_detected", "pred_matched")}
    lesions = []
    for c in range(1, K):
        P, G = masks(pred, labels, c)
        for side, own, other, n_key, hit_key in (("gt", G, P, "n_gt", "gt_detected"), ("pred", P, G, "n_pred", "pred_matched")):
            lab, n = label_ref(own, connectivity)
            size, over = sizes_ref(lab, n), overlap_ref(lab, n, other)
            out[n_key][c], out[hit_key][c] = n, int((over[1:] > 0).sum())
            lesions.extend((c, side, m, int(size[m]), int(over[m])) for m in range(1, n + 1))
    out["lesions"] = lesions
    return out


def smallest_component_ml(pred, K, connectivity, voxel_ml):
    s = [sizes_ref(*label_ref(pred == c, connectivity))[1:] for c in range(1, K)]
    s = np.concatenate(s) if s else np.zeros(0)
    return float(s.min()) * voxel_ml if s.size else float("inf")


# ---- a union-find labeller whose faults can be switched on ---------------------------------------------------------------------------------
FAULTS = ("skip_seam_k", "skip_seam_j", "skip_seam_i", "conn18_for_26", "row_wrap", "discovery_order", "no_flatten", "counter16")


def _edges(mask, connectivity, tile, fault):
    nk, nj, ni = mask.shape
    idx = np.arange(mask.size, dtype=np.int64).reshape(mask.shape)
    conn = 18 if (fault == "conn18_for_26" and connectivity == 26) else connectivity
    a_all, b_all = [], []
    for d in DIRECTIONS:
        if not allowed(d, conn):
            continue
        src = tuple(slice(max(0, -x), n - max(0, x)) for x, n in zip(d, mask.shape))
        dst = tuple(slice(max(0, x), n - max(0, -x)) for x, n in zip(d, mask.shape))
        both = mask[src] & mask[dst]
        a, b = idx[src][both], idx[dst][both]
        if fault and fault.startswith("skip_seam_"):
            ax = "kji".index(fault[-1])
            stride = (nj * ni, ni, 1)[ax]
            size = mask.shape[ax]
            keep = ((a // stride) % size) // tile[ax] == ((b // stride) % size) // tile[ax]
            a, b = a[keep], b[keep]
        a_all.append(a)
        b_all.append(b)
    if fault == "row_wrap":  # memory neighbours across the end of a row
        flat = mask.reshape(-1)
        v = np.arange(ni - 1, mask.size - 1, ni)
        v = v[flat[v] & flat[v + 1]]
        a_all.append(v)
        b_all.append(v + 1)
    return np.concatenate(a_all), np.concatenate(b_all)


def _jump(p):
    while True:
        q = p[p]
        if np.array_equal(q, p):
            return p
        p = q


def label_uf(mask, connectivity, tile=(AXIS_LIMIT,) * 3, fault=None):
    """(labels int32, n) by union-find over the edge list: roots hook below the smaller root, pointer jumping in between.  With
    fault=None it restates label_ref; each fault of FAULTS is a mistake a kernel could make."""
    mask = np.asarray(mask, bool)
    a, b = _edges(mask, connectivity, tile, fault)
    parent = np.arange(mask.size, dtype=np.int64)
    first_hook = None
    while True:
        pa, pb = parent[a], parent[b]
        new = parent.copy()
        np.minimum.at(new, np.maximum(pa, pb), np.minimum(pa, pb))
        if first_hook is None:
            first_hook = new.copy()
        new = _jump(new)
        if np.array_equal(new, parent):
            break
        parent = new
    flat = mask.reshape(-1)
    if fault == "no_flatten":
        parent = first_hook  # every voxel still points at what it was first hooked below
    is_root = flat & (parent == np.arange(mask.size))
    roots = np.flatnonzero(is_root)
    if fault == "discovery_order":  # numbered as a column-major sweep would meet them
        k, j, i = np.unravel_index(roots, mask.shape)
        roots = roots[np.lexsort((k, j, i))]
    number = np.zeros(mask.size, np.int64)
    number[roots] = np.arange(1, roots.size + 1)
    if fault == "counter16":
        number &= 0xFFFF
    lab = np.where(flat, number[parent], 0)
    return lab.reshape(mask.shape).astype(np.int32), int(roots.size if fault != "counter16" else roots.size & 0xFFFF)


# ---- cases -----------------------------------------------------------------------------------------------------------------------------------
SEAM_CAP = (35, 69, 135)  # 2 T + (3, 5, 7) at T = (16, 32, 64); a larger tile is cut to this, about 0.33 M voxels


def seam_shape(tile):
    return tuple(min(2 * t + e, cap) for t, e, cap in zip(tile, (3, 5, 7), SEAM_CAP))


def seam_corner(tile):
    """The tile corner the seam cases straddle: T itself, or the middle of the capped shape where the tile is larger."""
    return tuple(t if 2 * t + e <= cap else s // 2 for t, e, cap, s in zip(tile, (3, 5, 7), SEAM_CAP, seam_shape(tile)))


def ellipsoid(shape, centre, radii):
    g = np.ogrid[tuple(slice(0, s) for s in shape)]
    return sum(((x - c) / r) ** 2 for x, c, r in zip(g, centre, radii)) <= 1.0


def bernoulli(shape, p, seed=0):
    return np.random.default_rng(seed).random(shape) < p


def serpentine(shape):
    """One voxel wide: every other row of every other plane, rows joined at alternating ends, planes joined at alternating corners."""
    nk, nj, ni = shape
    m = np.zeros(shape, bool)
    rows = list(range(0, nj, 2))
    at_end = False  # where the walk stands along i
    for pk, k in enumerate(range(0, nk, 2)):
        order = rows if pk % 2 == 0 else rows[::-1]
        for n, j in enumerate(order):
            m[k, j, :] = True
            if n + 1 < len(order):
                at_end = not at_end
                m[k, min(j, order[n + 1]):max(j, order[n + 1]) + 1, ni - 1 if at_end else 0] = True
        if k + 2 < nk:
            at_end = not at_end
            m[k:k + 3, order[-1], ni - 1 if at_end else 0] = True
    return m


def comb(shape):
    """Teeth along k on every other (j, i) column of every other row, joined only by the full last plane."""
    m = np.zeros(shape, bool)
    m[:, ::2, ::2] = True
    m[-1] = True
    return m


def corners(shape):
    m = np.zeros(shape, bool)
    for c in itertools.product((0, -1), repeat=3):
        m[c] = True
    return m


def alternating(shape):
    m = np.zeros(shape, bool)
    m.reshape(-1)[np.arange(m.size) % 5 < 3] = True  # runs of three, gaps of two
    return m


def seam_pair(tile, d):
    shape, c = seam_shape(tile), seam_corner(tile)
    m = np.zeros(shape, bool)
    x = tuple(ci - (1 if di > 0 else 0) for ci, di in zip(c, d))  # x and x + d straddle the corner on every axis d moves along
    m[x] = True
    m[tuple(xi + di for xi, di in zip(x, d))] = True
    return m


def seam_blobs(tile, d):
    m = seam_pair(tile, d)
    x = np.argwhere(m)
    lo, hi = x[0], x[1]
    for p, sign in ((lo, -1), (hi, 1)):  # a 10^3 blob with each voxel of the pair as the corner that faces the other blob
        sl = []
        for a in range(3):
            step = d[a] * sign if d[a] else sign
            a0, a1 = (p[a] - 9, p[a] + 1) if step < 0 else (p[a], p[a] + 10)
            sl.append(slice(max(a0, 0), min(a1, m.shape[a])))
        m[tuple(sl)] = True
    return m


def no_wrap_cases(shape=(4, 6, 9)):
    nk, nj, ni = shape
    a, b = np.zeros(shape, bool), np.zeros(shape, bool)
    a[1, 2, ni - 1] = a[1, 3, 0] = True
    b[1, nj - 1, ni - 1] = b[2, 0, 0] = True
    return {"wrap_j": a, "wrap_k": b}


def diagonal(n, body):
    m = np.zeros((n, n, n), bool)
    r = np.arange(n)
    m[r if body else 0, r, r] = True
    return m


def checkerboard(n):
    k, j, i = np.ogrid[0:n, 0:n, 0:n]
    return (k + j + i) % 2 == 0


def lattice(shape=(64, 96, 96)):
    m = np.zeros(shape, bool)
    m[::2, ::2, ::2] = True
    return m


def small_cases(tile):
    """name -> mask: the cases cheap enough for the numpy labeller too (the CPU test runs every planted fault against them)."""
    shape = seam_shape(tile)
    out = {"empty": np.zeros(shape, bool), "full": np.ones(shape, bool), "corners": corners(shape), "one": np.ones((1, 1, 1), bool)}
    for s in ((1, 1, 300), (1, 300, 1), (300, 1, 1)):
        out["alt_" + "x".join(map(str, s))] = alternating(s)
    for p in (0.08, 0.2, 0.31, 0.5):
        out[f"bernoulli_{p}"] = bernoulli((37, 45, 70), p)
    out["checkerboard"] = checkerboard(24)
    out["face_diagonal"], out["body_diagonal"] = diagonal(40, False), diagonal(40, True)
    for d in DIRECTIONS:
        out["seam_" + "".join("-0+"[x + 1] for x in d)] = seam_pair(tile, d)
    for d in ((0, 0, 1), (0, 1, 1), (1, 1, 1), (1, -1, 1)):
        out["blobs_" + "".join("-0+"[x + 1] for x in d)] = seam_blobs(tile, d)
    out.update(no_wrap_cases())
    out["serpentine"] = serpentine(shape)
    out["comb"] = comb(shape)
    return out


# scipy on bernoulli((37, 45, 70), p, seed 0), p = 0.08, 0.2, 0.31, 0.5: from thousands of components to a handful
BERNOULLI_COUNTS = {6: (7201, 10155, 6871, 1234), 26: (2420, 165, 14, 3)}


def removal_case(min_voxels=12):
    """K = 3 on (20, 30, 40): per class cuboids of min_voxels - 1, min_voxels and min_voxels + 1 voxels (min_voxels = 12: 1 x 1 x 11,
    2 x 2 x 3, 1 x 1 x 13), two of the small ones 26-adjacent (through a corner) to a cuboid of the OTHER class, ignore voxels inside a
    cuboid of every size, and labels that agree in part.  -> pred int16, labels uint8."""
    assert min_voxels == 12
    pred, labels = np.zeros((20, 30, 40), np.int16), np.zeros((20, 30, 40), np.uint8)
    for c, k0 in ((1, 1), (2, 11)):
        o = 3 - c
        pred[k0, 2, 2:13] = c            # 11 voxels: removed
        pred[k0 + 1, 3, 13:18] = o       # the other class touches its end through a corner: 5 voxels, removed, and must not save it
        pred[k0:k0 + 2, 8:10, 2:5] = c   # 12 voxels: kept
        pred[k0 + 2, 10, 5:16] = o       # 11 voxels of the other class at the kept cuboid's corner: removed
        pred[k0, 14, 2:15] = c           # 13 voxels: kept
        pred[k0 + 4, 20:23, 20:24] = c   # 12 voxels with ignore voxels inside: kept, the filter does not look at labels
        labels[k0 + 4, 21, 21:23] = 255
        pred[k0 + 6, 25, 20:31] = c      # 11 voxels with an ignore voxel inside: removed
        labels[k0 + 6, 25, 25] = 255
        labels[k0:k0 + 2, 8:10, 2:6][labels[k0:k0 + 2, 8:10, 2:6] == 0] = c
        labels[k0, 2, 2:8] = c
        labels[k0, 14, 4:20] = c
    return pred, labels


def lesion_scene():
    """K = 2 on (16, 40, 48).  Truth: A missed, B touched by a single predicted voxel, C covered by two predicted components.
    Prediction: p1 (one voxel of it in B), p2 and p3 (in C), p4 a false alarm, p5 whose only overlap with the annotated A lies
    under label 255: those voxels belong to neither mask, so p5 counts as unmatched and A stays missed.  Recall 2 / 3, precision 3 / 5."""
    pred, labels = np.zeros((16, 40, 48), np.int16), np.zeros((16, 40, 48), np.uint8)
    labels[2:5, 3:9, 3:8] = 1                                  # A ...
    labels[2:5, 7:9, 3:8] = 255                                # ... whose rim towards p5 is not to be scored
    pred[2:5, 8:12, 3:8] = 1                                   # p5 meets A only at j = 8, under the ignore label
    labels[2:5, 20:24, 3:8] = 1                                # B
    pred[4:7, 23:26, 7:12] = 1                                 # p1: (4, 23, 7) is its only voxel in B
    labels[9:13, 4:16, 20:40] = 1                              # C
    pred[10:12, 5:9, 22:28] = 1                                # p2
    pred[10:12, 11:15, 30:38] = 1                              # p3
    pred[2:4, 30:33, 30:35] = 1                                # p4
    return pred, labels
