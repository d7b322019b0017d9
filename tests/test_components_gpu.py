"""GPU: the connected-component kernels (csrc/components.hip) through the C ABI, then the host layer and the entry point, against
tests/components_ref.py (scipy.ndimage.label and numpy restatements).  Every buffer a kernel writes lies inside a sentinel-filled
guarded allocation, every flag volume inside 0xFF guards (a read past the volume would find mask voxels there).  Everything here is
an integer: labels, counts and tables are compared bit for bit, and every call is repeated with equal results."""
import csv
import gzip
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from headct_foundation_amd import _lib, components
from headct_foundation_amd.metrics import LesionMetrics
from tests import components_ref as R
from tests.test_assembly_kernels_gpu import _st
from tests.test_segmentation_gpu import _vit, _write_pair

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONNS = (6, 18, 26)
BITS = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


class _Guarded:
    """A tensor in the middle of a filled allocation; `result()` checks the guards bit for bit."""

    def __init__(self, shape, dtype, dev, fill, guard=4096):
        n = int(np.prod(shape))
        self.g, self.n = guard, n
        self.buf = torch.full((n + 2 * guard,), fill, dtype=dtype, device=dev)
        self.ref = self.buf.clone()
        self.t = self.buf[guard:guard + n].view(shape)
        self.ptr = self.t.data_ptr()

    def put(self, array):
        self.t.copy_(torch.from_numpy(np.ascontiguousarray(array)))
        return self

    def result(self):
        a, b = self.buf.view(BITS[self.buf.element_size()]), self.ref.view(BITS[self.buf.element_size()])
        assert bool((a[:self.g] == b[:self.g]).all()) and bool((a[self.g + self.n:] == b[self.g + self.n:]).all()), "guard band written"
        return self.t.cpu().numpy()


def _tile(lib):
    return components.tile_dims()


def _ws(lib, dev, nbytes):
    return _Guarded((max(int(nbytes), 16) // 8,), torch.int64, dev, -1, guard=64)


def _flags_of_mask(mask, bit):
    """The mask in `bit`, and the other bit set on a pattern of its own: only the asked-for bit may count."""
    other = 3 - bit
    noise = (np.arange(mask.size).reshape(mask.shape) % 3 == 0)
    return (mask.astype(np.uint8) * bit) | (noise.astype(np.uint8) * other)


def _label(lib, dev, mask, conn, bit=1):
    """(root form, labels 1 .. n, n) of hct_cc_label and hct_cc_compact, guards checked."""
    nk, nj, ni = mask.shape
    f = _Guarded(mask.shape, torch.uint8, dev, 0xFF).put(_flags_of_mask(mask, bit))
    lab = _Guarded(mask.shape, torch.int32, dev, -77)
    n_out = _Guarded((1,), torch.int64, dev, -77, guard=64)
    ws = _ws(lib, dev, max(lib.hct_cc_label_workspace_bytes(nk, nj, ni), lib.hct_cc_compact_workspace_bytes(nk, nj, ni)))
    _lib.check(lib.hct_cc_label(f.ptr, bit, nk, nj, ni, conn, lab.ptr, ws.ptr, ws.n * 8, _st()), "hct_cc_label")
    torch.cuda.synchronize()
    root = lab.result().copy()
    _lib.check(lib.hct_cc_compact(lab.ptr, nk, nj, ni, n_out.ptr, ws.ptr, ws.n * 8, _st()), "hct_cc_compact")
    torch.cuda.synchronize()
    f.result(), ws.result()
    return root, lab.result(), int(n_out.result()[0])


_REF = {}


def _ref(name, mask, conn):
    """scipy's labels of a case: computed once, shared, read only."""
    if (name, conn) not in _REF:
        _REF[name, conn] = (R.root_form(mask, conn),) + R.label_ref(mask, conn)
    return _REF[name, conn]


_CASES = {}


def _cases(lib):
    if not _CASES:
        _CASES.update(R.small_cases(_tile(lib)))
    return _CASES


def _check(lib, cuda, name, mask, conn, bit=1):
    want_root, want, want_n = _ref(name, mask, conn)
    root, lab, n = _label(lib, cuda, mask, conn, bit)
    assert n == want_n, (name, conn, n, want_n)
    assert np.array_equal(root, want_root), (name, conn, "root form")
    assert np.array_equal(lab, want), (name, conn, "numbering")
    root2, lab2, n2 = _label(lib, cuda, mask, conn, bit)
    assert n2 == n and root2.tobytes() == root.tobytes() and lab2.tobytes() == lab.tobytes()
    return want_n


CASE_NAMES = list(R.small_cases((R.AXIS_LIMIT,) * 3))  # the names do not depend on the tile


@pytest.mark.parametrize("conn", CONNS)
@pytest.mark.parametrize("name", CASE_NAMES)
def test_labels_bit_equal_to_scipy(lib, cuda, name, conn):
    """Empty, full and corner masks, degenerate shapes with alternating runs, Bernoulli masks from thousands of components to one,
    the connectivity tells, the 13 seam pairs and the blobs that touch only through one, the row and plane wrap-around, the
    serpentine and the comb: root form and numbering equal scipy's, twice."""
    mask = _cases(lib)[name]
    n = _check(lib, cuda, name, mask, conn, bit=1 if len(name) % 2 else 2)
    if name == "empty":
        assert n == 0
    if name in ("full", "one"):
        assert n == 1
    if name == "corners":
        assert n == 8
    if name.startswith("bernoulli_") and conn in R.BERNOULLI_COUNTS:
        assert n == R.BERNOULLI_COUNTS[conn][(0.08, 0.2, 0.31, 0.5).index(float(name.split("_")[1]))]
    if name == "checkerboard":
        assert n == (6912 if conn == 6 else 1)
    if name == "face_diagonal":
        assert n == (40 if conn == 6 else 1)
    if name == "body_diagonal":
        assert n == (1 if conn == 26 else 40)
    if name.startswith("seam_"):
        d = tuple("-0+".index(ch) - 1 for ch in name[5:])
        assert int(mask.sum()) == 2 and n == (1 if R.allowed(d, conn) else 2)
    if name.startswith("blobs_"):
        d = tuple("-0+".index(ch) - 1 for ch in name[6:])
        assert n == (1 if R.allowed(d, conn) else 2)
    if name.startswith("wrap_"):
        assert n == 2
    if name == "serpentine":
        assert n == 1 and int(mask.sum()) > mask.size // 5


@pytest.mark.parametrize("conn", CONNS)
def test_comb_root_form_is_the_first_voxel(lib, cuda, conn):
    """Teeth that meet only in the last plane: before compaction every mask voxel carries 1 + the index of the first voxel, 0."""
    mask = _cases(lib)["comb"]
    root, lab, n = _label(lib, cuda, mask, conn)
    assert n == 1 and mask[0, 0, 0] and (root[mask] == 1).all() and (root[~mask] == 0).all()


@pytest.mark.parametrize("conn", CONNS)
def test_many_components_pass_65536(lib, cuda, conn):
    """73 728 isolated voxels: more than one workgroup of the second scan level (1024 chunks of 4096 voxels would be 4 M voxels;
    here 144 chunks), and a count past 16 bits."""
    mask = R.lattice()
    assert _check(lib, cuda, "lattice", mask, conn) == 73728


def test_numbering_crosses_the_second_scan_level(lib, cuda):
    """(40, 330, 330) = 4 356 000 voxels = 1064 chunks of 4096: two workgroups at the second level of the prefix sum, roots on
    both sides of the border between them."""
    mask = np.zeros((40, 330, 330), bool)
    mask[::3, ::7, ::5] = True
    mask[38:, :, :] = True
    assert _check(lib, cuda, "two_level", mask, 6) == int(mask[:38].sum()) + 1


# ---- masks, sizes, overlap ------------------------------------------------------------------------------------------------------------------
def _two_ellipsoids():
    shape = (20, 45, 70)
    pred = R.ellipsoid(shape, (9, 20, 30), (6, 12, 20)).astype(np.int16)
    labels = R.ellipsoid(shape, (11, 25, 40), (6, 12, 20)).astype(np.uint8)
    labels[8:12, 20:24, 30:36] = 255
    pred[0:3, 40:45, 60:70] = 2
    return pred, labels


def _masks(lib, dev, pred, labels, c):
    nk, nj, ni = pred.shape
    p = _Guarded(pred.shape, torch.int16, dev, c).put(pred)
    y = _Guarded(pred.shape, torch.uint8, dev, c).put(labels) if labels is not None else None
    flags = _Guarded(pred.shape, torch.uint8, dev, 0xEE)
    _lib.check(lib.hct_cc_masks(p.ptr, y.ptr if y is not None else None, nk, nj, ni, c, flags.ptr, _st()), "hct_cc_masks")
    torch.cuda.synchronize()
    p.result()
    return flags.result()


@pytest.mark.parametrize("with_labels", [True, False])
def test_masks_bit_for_bit(lib, cuda, with_labels):
    pred, labels = _two_ellipsoids()
    for c in (1, 2, 7):
        got = _masks(lib, cuda, pred, labels if with_labels else None, c)
        assert np.array_equal(got, R.flags_of(pred, labels if with_labels else None, c))
    assert ((labels == 255) & (pred == 1)).sum() > 20
    if not with_labels:
        assert not (got & 2).any()


def _tables(lib, dev, lab, n, flags, bit_b):
    nvox = lab.size
    l = _Guarded(lab.shape, torch.int32, dev, n).put(lab)
    f = _Guarded(lab.shape, torch.uint8, dev, 0xFF).put(flags)
    sizes, over = _Guarded((n + 1,), torch.int64, dev, -5, guard=64), _Guarded((n + 1,), torch.int64, dev, -5, guard=64)
    _lib.check(lib.hct_cc_sizes(l.ptr, nvox, n, sizes.ptr, _st()), "hct_cc_sizes")
    _lib.check(lib.hct_cc_overlap(l.ptr, n, f.ptr, bit_b, nvox, over.ptr, _st()), "hct_cc_overlap")
    torch.cuda.synchronize()
    l.result(), f.result()
    return sizes.result(), over.result()


@pytest.mark.parametrize("conn", CONNS)
@pytest.mark.parametrize("name", ["bernoulli_0.08", "bernoulli_0.2", "bernoulli_0.31", "bernoulli_0.5", "ellipsoids"])
def test_sizes_and_overlap_against_bincount(lib, cuda, name, conn):
    if name == "ellipsoids":
        pred, labels = _two_ellipsoids()
        flags = R.flags_of(pred, labels, 1)
    else:
        mask = _cases(lib)[name]
        flags = mask.astype(np.uint8) | (R.bernoulli(mask.shape, 0.4, seed=5).astype(np.uint8) << 1)
    lab, n = R.label_ref((flags & 1) != 0, conn)
    sizes, over = _tables(lib, cuda, lab, n, flags, 2)
    assert np.array_equal(sizes, R.sizes_ref(lab, n)) and np.array_equal(over, R.overlap_ref(lab, n, (flags & 2) != 0))
    assert sizes[1:].sum() == (lab > 0).sum() and 0 < over.sum() < sizes.sum()
    sizes2, over2 = _tables(lib, cuda, lab, n, flags, 2)
    assert sizes2.tobytes() == sizes.tobytes() and over2.tobytes() == over.tobytes()


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 700001])
def test_count_small_against_numpy(lib, cuda, n):
    """How many of the labels 1 .. n lie below the threshold: entry 0 and everything past n (small values both) are not counted; more
    labels than one pass of the grid (2048 x 256) at 700 001."""
    sizes = np.random.default_rng(n).integers(1, 40, n + 1).astype(np.int64)
    sizes[0] = 0
    s = _Guarded((n + 1,), torch.int64, cuda, 0, guard=64).put(sizes)
    for mv in (1, 12, 40):
        out = _Guarded((1,), torch.int64, cuda, -5, guard=64)
        _lib.check(lib.hct_cc_count_small(s.ptr, n, mv, out.ptr, _st()), "hct_cc_count_small")
        torch.cuda.synchronize()
        assert int(out.result()[0]) == int((sizes[1:] < mv).sum()), mv
    s.result()
    assert lib.hct_cc_count_small(s.ptr, -1, 5, out.ptr, _st()) == -1 and lib.hct_cc_count_small(None, 1, 5, out.ptr, _st()) == -1


def test_host_handles_match_the_kernels(cuda):
    mask = R.bernoulli((37, 45, 70), 0.2)
    for conn in CONNS:
        want, want_n = R.label_ref(mask, conn)
        lab, n = components.connected_components(torch.from_numpy(mask.astype(np.uint8) * 2).to(cuda), bit=2, connectivity=conn)
        assert n == want_n and lab.dtype == torch.int32 and np.array_equal(lab.cpu().numpy(), want)
        assert np.array_equal(components.component_sizes(lab, n).cpu().numpy(), R.sizes_ref(want, want_n))


# ---- removal and recount -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("conn", CONNS)
def test_remove_small_components_and_recount(cuda, conn):
    """Cuboids of min_voxels - 1, min_voxels and min_voxels + 1 voxels per class, some at the corner of a cuboid of the other class,
    some with ignore voxels inside: the filtered prediction, the removed counts, class_voxels and TP / FP / FN equal the restatement."""
    K, mv = 3, 12
    pred, labels = R.removal_case(mv)
    want = R.remove_small_ref(pred, K, mv, conn, labels)
    assert want["removed"].tolist() == [0, 4, 4] and (want["pred"] != pred).sum() == 2 * (11 + 5 + 11 + 11)
    pd = torch.from_numpy(pred).to(cuda)
    for run in range(2):
        got = components.remove_small_components(pd, K, mv, conn, labels=torch.from_numpy(labels).to(cuda))
        assert np.array_equal(got["pred"].cpu().numpy(), want["pred"]) and got["pred"].dtype == torch.int16
        assert got["removed"].tolist() == want["removed"].tolist()
        assert got["class_voxels"].cpu().tolist() == want["class_voxels"].tolist()
        assert got["counts"].cpu().tolist() == want["counts"].tolist()
    assert np.array_equal(pd.cpu().numpy(), pred)  # the input is not touched
    got = components.remove_small_components(pd, K, mv, conn)  # without labels: no counts
    assert got["counts"] is None and got["class_voxels"].cpu().tolist() == want["class_voxels"].tolist()
    # every surviving component is at least min_voxels large
    for c in (1, 2):
        lab, n = R.label_ref(want["pred"] == c, conn)
        assert R.sizes_ref(lab, n)[1:].min() >= mv


def test_remove_small_components_below_two_voxels_returns_its_inputs(cuda):
    pred, labels = R.removal_case()
    pd = torch.from_numpy(pred).to(cuda)
    cv, cn = torch.arange(3, device=cuda), torch.arange(9, device=cuda).view(3, 3)
    for mv in (1, 0, -3):
        got = components.remove_small_components(pd, 3, mv, 26, labels=labels, class_voxels=cv, counts=cn)
        assert got["pred"] is pd and got["class_voxels"] is cv and got["counts"] is cn and got["removed"].tolist() == [0, 0, 0]


def test_recount_matches_seg_to_native_conventions(lib, cuda):
    """K = 3 with labels 0 .. 2, 3 (>= K: ignore) and 255: class_voxels over the whole grid, TP / FP / FN over the valid voxels;
    a workspace inside guards; without labels only class_voxels."""
    gen = np.random.default_rng(3)
    shape = (9, 33, 301)
    pred = gen.integers(0, 3, shape).astype(np.int16)
    labels = gen.choice(np.array([0, 1, 2, 3, 255], np.uint8), shape)
    nk, nj, ni = shape
    p, y = _Guarded(shape, torch.int16, cuda, 1).put(pred), _Guarded(shape, torch.uint8, cuda, 1).put(labels)
    cv, cn = _Guarded((3,), torch.int64, cuda, -9, guard=64), _Guarded((3, 3), torch.int64, cuda, -9, guard=64)
    ws = _ws(lib, cuda, lib.hct_seg_recount_workspace_bytes(nk, nj, ni, 3))
    _lib.check(lib.hct_seg_recount(p.ptr, y.ptr, nk, nj, ni, 3, cv.ptr, cn.ptr, ws.ptr, ws.n * 8, _st()), "hct_seg_recount")
    torch.cuda.synchronize()
    want_cv, want_cn = R.recount_ref(pred, labels, 3)
    ws.result(), p.result(), y.result()
    assert cv.result().tolist() == want_cv.tolist() and cn.result().tolist() == want_cn.tolist()
    cv2 = _Guarded((3,), torch.int64, cuda, -9, guard=64)
    _lib.check(lib.hct_seg_recount(p.ptr, None, nk, nj, ni, 3, cv2.ptr, None, ws.ptr, ws.n * 8, _st()), "hct_seg_recount")
    torch.cuda.synchronize()
    assert cv2.result().tolist() == want_cv.tolist()


# ---- lesion metrics -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("conn", CONNS)
def test_lesion_metrics_on_the_planted_scene(cuda, conn):
    pred, labels = R.lesion_scene()
    want = R.lesion_metrics_ref(pred, labels, 2, conn)
    assert (want["n_gt"][1], want["gt_detected"][1], want["n_pred"][1], want["pred_matched"][1]) == (3, 2, 5, 3)
    got = components.lesion_metrics(torch.from_numpy(pred).to(cuda), torch.from_numpy(labels).to(cuda), 2, conn)
    for k in ("n_gt", "n_pred", "gt_detected", "pred_matched"):
        assert got[k].dtype == np.int64 and got[k].tolist() == want[k].tolist(), k
    assert got["lesions"] == want["lesions"] and len(got["lesions"]) == 8
    touched = [r for r in got["lesions"] if r[1] == "gt" and r[4] == 1]
    assert len(touched) == 1  # the lesion a single predicted voxel reaches
    m = LesionMetrics(2)
    m(got)
    out = m.compute()
    assert out["LesionRecall"][1] == 2 / 3 and out["LesionPrecision"][1] == 3 / 5 and np.isnan(out["LesionRecall"][0])
    assert abs(out["LesionF1"][1] - 2 * (2 / 3) * (3 / 5) / (2 / 3 + 3 / 5)) < 1e-15
    again = components.lesion_metrics(torch.from_numpy(pred).to(cuda), labels, 2, conn)  # the mask file's array, as the engine passes it
    assert again["lesions"] == got["lesions"]


def test_lesion_metrics_over_two_emulated_ranks(cuda):
    scans = []
    for n in range(4):
        pred, labels = R.lesion_scene()
        pred, labels = np.roll(pred, n, axis=2), np.roll(labels, 2 * n, axis=1)
        scans.append(components.lesion_metrics(torch.from_numpy(pred).to(cuda), torch.from_numpy(labels).to(cuda), 2, 18))
        want = R.lesion_metrics_ref(pred, labels, 2, 18)
        assert all(scans[-1][k].tolist() == want[k].tolist() for k in LesionMetrics.KEYS) and scans[-1]["lesions"] == want["lesions"]
    one, a, b = LesionMetrics(2), LesionMetrics(2), LesionMetrics(2)
    for n, s in enumerate(scans):
        one(s)
        (a, b)[n % 2](s)
    a.merge(b)
    x, y = one.compute(), a.compute()
    assert all(np.array_equal(np.asarray(x[k]), np.asarray(y[k]), equal_nan=True) for k in x)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(lib, cuda):
    mask = np.ones((2, 3, 4), np.uint8)
    f = _Guarded(mask.shape, torch.uint8, cuda, 0xFF).put(mask)
    lab = _Guarded(mask.shape, torch.int32, cuda, -77)
    n_out = _Guarded((1,), torch.int64, cuda, -77, guard=64)
    ws = _ws(lib, cuda, 4096)
    big = 8 * (1 << 20)
    for conn in (4, 0, 27, 8):
        assert lib.hct_cc_label(f.ptr, 1, 2, 3, 4, conn, lab.ptr, ws.ptr, ws.n * 8, _st()) == -1
    assert "connectivity" in lib.hct_last_error_string().decode()
    for shape in ((0, 3, 4), (2, 0, 4), (2, 3, 0), (32769, 1, 1), (1, 32769, 1), (1, 1, 32769), (2048, 1024, 1024), (32768, 32768, 2)):
        assert lib.hct_cc_label(f.ptr, 1, *shape, 26, lab.ptr, ws.ptr, big, _st()) == -1, shape  # by the arguments alone: nothing that large exists
        assert lib.hct_cc_compact(lab.ptr, *shape, n_out.ptr, ws.ptr, big, _st()) == -1, shape
        assert lib.hct_cc_masks(f.ptr, None, *shape, 1, f.ptr, _st()) == -1, shape
        assert lib.hct_seg_recount(f.ptr, None, *shape, 2, n_out.ptr, None, ws.ptr, big, _st()) == -1, shape
        assert lib.hct_cc_compact_workspace_bytes(*shape) == 0 and lib.hct_seg_recount_workspace_bytes(*shape, 2) == 0
    assert lib.hct_cc_label(f.ptr, 0, 2, 3, 4, 26, lab.ptr, ws.ptr, ws.n * 8, _st()) == -1
    assert lib.hct_cc_masks(f.ptr, None, 2, 3, 4, 255, f.ptr, _st()) == -1
    for nvox in (0, -1, (1 << 31) - 1):
        assert lib.hct_cc_sizes(lab.ptr, nvox, 1, n_out.ptr, _st()) == -1
        assert lib.hct_cc_overlap(lab.ptr, 1, f.ptr, 1, nvox, n_out.ptr, _st()) == -1
        assert lib.hct_cc_remove_small(f.ptr, lab.ptr, n_out.ptr, 2, nvox, _st()) == -1
    assert lib.hct_cc_sizes(lab.ptr, 24, 25, n_out.ptr, _st()) == -1 and lib.hct_cc_sizes(lab.ptr, 24, -1, n_out.ptr, _st()) == -1
    assert lib.hct_seg_recount(f.ptr, None, 2, 3, 4, 17, n_out.ptr, None, ws.ptr, ws.n * 8, _st()) == -1
    assert lib.hct_seg_recount(f.ptr, None, 2, 3, 4, 2, n_out.ptr, n_out.ptr, ws.ptr, ws.n * 8, _st()) == -1  # counts without labels
    # too small a workspace
    assert lib.hct_cc_compact_workspace_bytes(2, 3, 4) == 16 and lib.hct_cc_compact(lab.ptr, 2, 3, 4, n_out.ptr, ws.ptr, 8, _st()) == -3
    assert lib.hct_cc_compact(lab.ptr, 2, 3, 4, n_out.ptr, None, 0, _st()) == -3
    need = lib.hct_seg_recount_workspace_bytes(2, 3, 4, 2)
    assert need == 32 and lib.hct_seg_recount(f.ptr, None, 2, 3, 4, 2, n_out.ptr, None, ws.ptr, need - 1, _st()) == -3
    need = lib.hct_cc_label_workspace_bytes(2, 3, 4)
    if need:
        assert lib.hct_cc_label(f.ptr, 1, 2, 3, 4, 26, lab.ptr, ws.ptr, need - 1, _st()) == -3
    torch.cuda.synchronize()
    assert (lab.result() == -77).all() and (n_out.result() == -77).all() and (f.result() == 1).all() and (ws.result() == -1).all()


def test_host_layer_refuses_mismatched_tensors(cuda):
    p16 = torch.zeros(2, 3, 4, dtype=torch.int16, device=cuda)
    u8 = torch.zeros(2, 3, 4, dtype=torch.uint8, device=cuda)
    with pytest.raises(_lib.HctError, match="cuda"):
        components.connected_components(p16)  # dtype
    with pytest.raises(_lib.HctError, match="cuda"):
        components.connected_components(u8.cpu())
    with pytest.raises(_lib.HctError, match="cuda"):
        components.lesion_metrics(p16, torch.zeros(2, 3, 5, dtype=torch.uint8, device=cuda), 2)  # shape
    with pytest.raises(_lib.HctError, match="cuda"):
        components.lesion_metrics(p16.int(), u8, 2)
    with pytest.raises(_lib.HctError, match="cuda"):
        components.remove_small_components(p16.cpu(), 2, 5)
    with pytest.raises(_lib.HctError, match="cuda"):
        components.component_sizes(u8, 1)
    with pytest.raises(ValueError, match="connectivity"):
        components.connected_components(u8, connectivity=4)
    with pytest.raises(ValueError, match="connectivity"):
        components.lesion_metrics(p16, u8, 2, connectivity=8)


# ---- the entry point ------------------------------------------------------------------------------------------------------------------------
AFF_B = np.array([[0.0, 1.5, 0.0, -10.0], [-0.8, 0.0, 0.0, 12.0], [0.0, 0.0, 2.0, 5.0], [0.0, 0.0, 0.0, 1.0]])  # i -> -y, j -> +x: not RAS, anisotropic


def _logged(log, key, integers=False):
    m = re.search(key + r": \[([^\]]*)\]", log)
    assert m, key
    return [int(v) if integers else float(v) for v in m.group(1).split(",")]


def test_main_segmentation_lesions_end_to_end(lib, cuda, tmp_path):
    """main_segmentation.py --native_preds --lesion_metrics --min_component_ml X --component_connectivity 18 on four tiny anisotropic,
    non-RAS NIfTI pairs: both CSVs and the logged figures equal components_ref applied to the written <name>_native.nii.gz and the mask
    files, no written prediction has a component below X, and native_volumes.csv and the Dice describe the written masks.  With the
    three keys at their defaults (named or not), and with a threshold below one voxel's volume, the native files, native_volumes.csv
    and the logged Dice are byte-identical to the run that never mentions them."""
    from headct_foundation_amd.native import class_volumes_ml
    from headct_foundation_amd.nifti import read_nifti
    vit = _vit("fp32", 0)
    torch.save({"state_dict": {"module." + k: t for k, t in vit.state_dict().items()}, "epoch": 3}, tmp_path / "pre.pt")
    pairs = [_write_pair(tmp_path, f"s{n}", (24, 14, 10), AFF_B, n)[:2] for n in range(4)]
    pairs_csv = tmp_path / "pairs.csv"
    pairs_csv.write_text("img_path,seg_path\n" + "".join(f"{i},{s}\n" for i, s in pairs))
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("MODEL:\n  NAME: vit\n")

    def run(tag, extra):
        opts = ["VIT.INPUT_SIZE", "24", "VIT.PATCH_SIZE", "12", "VIT.HIDDEN_SIZE", "48", "VIT.MLP_DIM", "96", "VIT.NUM_LAYERS", "2", "VIT.NUM_HEADS", "3",
                "MODEL.ROI", "[24, 24, 24]", "TRAIN.VAL_EVERY", "1", "MODEL.DIR", str(tmp_path / tag), "MODEL.SAVE_NAME", "seg.pt", "LOG.OUTPUT_DIR",
                str(tmp_path / (tag + "_log")), "PREDS_SAVE_NAME", "run", "MAE.COMPUTE_DTYPE", "fp32", "DATA.CACHE_DIR", str(tmp_path / "cache"),
                "DATA.NUM_WORKERS", "2"]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nproc-per-node", "1", "--master-port", "29627", os.path.join(ROOT, "main_segmentation.py"),
               "--cfg", str(cfg), "--model_name", "vit", "--model_load_path", str(tmp_path / "pre.pt"), "--seg_classes", "3", "--batch_size", "2",
               "--max_epochs", "1", "--grad_clip", "1.0", "--base_lr", "1e-4", "--train_csv_path", str(pairs_csv), "--val_csv_path",
               str(pairs_csv), "--test_csv_path", str(pairs_csv), "--native_preds"] + extra + ["--opts"] + opts
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
        log = r.stdout + r.stderr
        assert r.returncode == 0, log[-4000:]
        return log, tmp_path / tag / "run_preds"

    def native(out, ip):
        return read_nifti(str(out / (os.path.basename(ip)[:-7] + "_native.nii.gz")))[0]

    K, conn = 3, 18
    voxel_ml = float(class_volumes_ml(np.ones(1), AFF_B)[0])
    assert abs(voxel_ml - 0.0024) < 1e-15
    log_off, out_off = run("off", [])
    raw = [native(out_off, ip).astype(np.int16) for ip, _ in pairs]
    sizes = np.sort(np.concatenate([R.sizes_ref(*R.label_ref(p == c, conn))[1:] for p in raw for c in range(1, K)]))
    assert sizes.size >= 1, "the barely trained head predicts some foreground"
    # the median component size where that removes the smaller half, else one voxel more than the smallest (a head this little
    # trained may predict single voxels only): at least two voxels either way, and at least the smallest components go
    cut = int(sizes[sizes.size // 2]) if sizes[sizes.size // 2] > sizes[0] else int(sizes[0]) + 1
    min_ml = (cut - 0.5) * voxel_ml  # between two voxel counts: no rounding can move the threshold
    assert components.min_voxels_for(min_ml, AFF_B) == cut
    log, out = run("on", ["--lesion_metrics", "--min_component_ml", repr(min_ml), "--component_connectivity", str(conn)])
    from headct_foundation_amd.metrics import SegmentationMetrics
    ref, seg, count_rows, lesion_rows, vol_rows = LesionMetrics(K), SegmentationMetrics(K), [], [], []
    for (ip, sp), before in zip(pairs, raw):
        pred = native(out, ip).astype(np.int16)
        mask = read_nifti(sp)[0].astype(np.uint8)
        assert R.smallest_component_ml(pred, K, conn, voxel_ml) >= min_ml
        assert np.array_equal(R.remove_small_ref(pred, K, cut, conn)["pred"], pred)  # filtering what was written changes nothing
        vol_rows.append([ip] + [f"{v:.6f}" for v in class_volumes_ml(R.recount_ref(pred, None, K)[0], AFF_B)])
        seg(R.recount_ref(pred, mask, K)[1][None])
        scan = R.lesion_metrics_ref(pred, mask, K, conn)
        ref(scan)
        count_rows.append([ip] + [str(int(scan[k][c])) for c in range(1, K) for k in LesionMetrics.KEYS])
        lesion_rows += [[ip, str(c), side, str(m), str(v), f"{v * voxel_ml:.6f}", str(o)] for c, side, m, v, o in scan["lesions"]]
    rows =lambda name: list(csv.reader(open(out / name)))
    assert rows("native_lesion_counts.csv") == [["name"] + [f"class_{c}_{k}" for c in range(1, K) for k in LesionMetrics.KEYS]] + count_rows
    assert rows("native_lesions.csv") == [["name", "class", "side", "index", "voxels", "ml", "overlap_voxels"]] + lesion_rows
    assert rows("native_volumes.csv")[1:] == vol_rows
    want = ref.compute()
    for key, k in (("NativeLesionRecall", "LesionRecall"), ("NativeLesionPrecision", "LesionPrecision"), ("NativeLesionF1", "LesionF1")):
        assert np.allclose(_logged(log, key), want[k], rtol=0, atol=1e-4, equal_nan=True), (key, _logged(log, key), want[k])
    assert np.allclose(_logged(log, "NativeDiceGlobal"), seg.compute()["DiceGlobal"], rtol=0, atol=1e-4, equal_nan=True)  # of the written masks
    assert _logged(log, "NativeLesionsGT", True) == want["n_gt"] and _logged(log, "NativeLesionsPred", True) == want["n_pred"]
    # the defaults, named: byte-identical to the run that never mentions them
    # and a threshold below one voxel's volume (0.002 mL of 0.0024 mL voxels: min_voxels = 1), which can remove nothing: the same
    assert components.min_voxels_for(0.002, AFF_B) == 1
    log_def, out_def = run("defaults", ["--min_component_ml", "0", "--component_connectivity", "26"])
    log_sub, out_sub = run("subvoxel", ["--min_component_ml", "0.002"])
    dice = lambda text: re.search(r"NativeDiceGlobal: \[[^\]]*\], NativeIoUGlobal: \[[^\]]*\], NativeDiceScan: \[[^\]]*\]", text).group(0)
    for text, o in ((log_def, out_def), (log_sub, out_sub)):
        for ip, _ in pairs:
            name = os.path.basename(ip)[:-7] + "_native.nii.gz"
            assert gzip.open(o / name, "rb").read() == gzip.open(out_off / name, "rb").read()  # the gzip header carries a time stamp: the content
        assert open(o / "native_volumes.csv", "rb").read() == open(out_off / "native_volumes.csv", "rb").read()
        assert dice(text) == dice(log_off)
    for text, o in ((log_off, out_off), (log_def, out_def), (log_sub, out_sub)):
        assert "NativeLesion" not in text and not os.path.exists(o / "native_lesions.csv") and not os.path.exists(o / "native_lesion_counts.csv")
