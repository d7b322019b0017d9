"""Float64 oracle of the surface-distance metrics (headct_foundation_amd/surface.py, csrc/surface.hip): MONAI's voxel-based
definitions restated with scipy.

For class c: P = (pred == c), G = (label == c), a voxel labelled 255 background in both.  E(M) = M & ~binary_erosion(M) with
scipy's defaults: the 6-neighbourhood, everything outside the volume background.  d(p -> G) is the value of
distance_transform_edt(~E(G), sampling=spacing) at p, spacing in array order (s_k, s_j, s_i).  HD is the larger of the two directed
maxima, HD95 the larger of the two directed 95th percentiles (numpy's linear one), ASSD the mean of all directed distances, NSD the
share of them within tau.  Both masks empty: all NaN; one empty: NSD 0, the rest NaN.

`faults` plants one wrong reading of the definitions each (test_surface_cpu.py shows that the test inputs tell every one of them
from the oracle).  `edt_direct` restates the arithmetic of hct_edt3d in numpy: three passes (k, j, i), each the direct minimum
over a line's candidates of g[l'] + ((l - l') s)^2, every product and sum rounded once.
"""
import numpy as np
from scipy import ndimage

FAULTS = ("erode26", "no_spacing", "spacing_ijk", "one_directed", "keep_ignore", "higher", "border")
IGNORE = 255


def masks(pred, labels, c, faults=()):
    pred, labels = np.asarray(pred), np.asarray(labels)
    valid = np.ones(labels.shape, bool) if "keep_ignore" in faults else labels != IGNORE
    return (pred == c) & valid, labels == c


def edges(mask, faults=()):
    structure = ndimage.generate_binary_structure(3, 3 if "erode26" in faults else 1)
    return mask & ~ndimage.binary_erosion(mask, structure=structure, border_value=1 if "border" in faults else 0)


def _sampling(spacing, faults=()):
    s = tuple(float(v) for v in spacing)
    if "no_spacing" in faults:
        return (1.0, 1.0, 1.0)
    return s[::-1] if "spacing_ijk" in faults else s


def field(edge, spacing, faults=()):
    """Distance of every voxel to the nearest voxel of `edge` (which must hold one)."""
    return ndimage.distance_transform_edt(~edge, sampling=_sampling(spacing, faults))


def directed(edge_a, edge_b, spacing, faults=()):
    """d(a -> B) for every voxel a of edge_a, in array order."""
    return field(edge_b, spacing, faults)[edge_a]


def q95(d, faults=()):
    return float(np.percentile(d, 95, method="higher" if "higher" in faults else "linear"))


def class_metrics(pred, labels, c, spacing, tau, faults=()):
    """{"HD", "HD95", "ASSD", "NSD", "n_pred", "n_gt", "d_pg", "d_gp"} of one class (the two distance arrays None where undefined)."""
    P, G = masks(pred, labels, c, faults)
    ep, eg = edges(P, faults), edges(G, faults)
    n_p, n_g = int(ep.sum()), int(eg.sum())
    out = {"HD": np.nan, "HD95": np.nan, "ASSD": np.nan, "NSD": np.nan, "n_pred": n_p, "n_gt": n_g, "d_pg": None, "d_gp": None}
    if n_p == 0 and n_g == 0:
        return out
    if n_p == 0 or n_g == 0:
        out["NSD"] = 0.0
        return out
    d_pg, d_gp = directed(ep, eg, spacing, faults), directed(eg, ep, spacing, faults)
    out["HD"] = float(max(d_pg.max(), d_gp.max()))
    out["HD95"] = q95(d_pg, faults) if "one_directed" in faults else max(q95(d_pg, faults), q95(d_gp, faults))
    out["ASSD"] = float((d_pg.sum() + d_gp.sum()) / (n_p + n_g))
    out["NSD"] = float(((d_pg <= tau).sum() + (d_gp <= tau).sum()) / (n_p + n_g))
    out["d_pg"], out["d_gp"] = d_pg, d_gp
    return out


def surface_metrics(pred, labels, num_classes, spacing, tau=2.0, faults=()):
    """Per-class arrays of length K (NaN / 0 at the background's index 0), as headct_foundation_amd.surface.surface_metrics returns."""
    K = int(num_classes)
    out = {k: np.full(K, np.nan) for k in ("HD", "HD95", "ASSD", "NSD")}
    out["n_pred"], out["n_gt"] = np.zeros(K, np.int64), np.zeros(K, np.int64)
    for c in range(1, K):
        m = class_metrics(pred, labels, c, spacing, tau, faults)
        for k in out:
            out[k][c] = m[k]
    return out


def edt_direct(features, spacing):
    """SQUARED distance to the nearest True voxel of `features` by the separable direct minimum, float64, in the kernel's order of
    operations; +inf everywhere where there is none."""
    g = np.where(np.asarray(features, bool), 0.0, np.inf)
    for axis, s in enumerate(float(v) for v in spacing):
        L = g.shape[axis]
        idx = np.arange(L, dtype=np.float64)
        t = (idx[:, None] - idx[None, :]) * np.float64(s)   # [l, l']: (l - l') s, rounded once
        sq = t * t                                          # rounded once
        lines = np.moveaxis(g, axis, -1)                    # [..., l']
        g = np.moveaxis((lines[..., None, :] + sq).min(axis=-1), -1, axis)
    return g


def ellipsoid(shape, centre, radii):
    k, j, i = np.ogrid[:shape[0], :shape[1], :shape[2]]
    return ((k - centre[0]) / radii[0]) ** 2 + ((j - centre[1]) / radii[1]) ** 2 + ((i - centre[2]) / radii[2]) ** 2 <= 1.0


def scan_case(name, shape=(24, 40, 56)):
    """(pred int16, labels uint8, K = 3) of the end-to-end cases: class 1 two overlapping ellipsoids that touch a face of the volume,
    with ignore voxels inside and on the rim; class 2 by `name`: 'both' a shifted pair of plates, 'pred_only' / 'gt_only' one mask
    empty, 'none' both empty."""
    nk, nj, ni = shape
    pred, labels = np.zeros(shape, np.int16), np.zeros(shape, np.uint8)
    labels[ellipsoid(shape, (nk * 0.45, nj * 0.5, ni * 0.4), (nk * 0.3, nj * 0.3, ni * 0.45))] = 1
    pred[ellipsoid(shape, (nk * 0.5, nj * 0.45, ni * 0.45), (nk * 0.28, nj * 0.33, ni * 0.4))] = 1
    plate_p, plate_g = (slice(nk - 4, nk - 3), slice(2, nj // 2), slice(ni - 12, ni)), (slice(nk - 2, nk), slice(4, nj // 2 + 3), slice(ni - 14, ni - 1))
    if name in ("both", "pred_only"):
        pred[plate_p] = 2
    if name in ("both", "gt_only"):
        labels[plate_g] = 2
    gen = np.random.default_rng(len(name))
    ign = gen.random(shape) < 0.01
    ign[nk // 2 - 2:nk // 2 + 2, nj // 2 - 3:nj // 2, 5:9] = True  # a block inside the blob, and one across its rim
    ign[nk // 2, 4:12, ni // 2:ni // 2 + 3] = True
    labels[ign] = IGNORE
    return pred, labels, 3
