"""CPU: the float64 restatement of the affine resampling (tests/affine_ref.py) against torch's grid_sample, the matrix conventions of
`affine_matrices`, the draws of `RandAffine3D`, the inertness of an attached affine on DeviceAugment's own flip / shift stream, and
the TRAIN.AFFINE_* configuration keys with their command-line flags."""
import math
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from headct_foundation_amd.data import DeviceAugment, RandAffine3D, affine_matrices
from tests import affine_ref as R


def _general_mats(B, S, seed, max_deg=30.0):
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(B, 9, generator=g, dtype=torch.float64) * 2 - 1
    return affine_matrices(u[:, :3] * max_deg, 0.8 + (u[:, 3:6] + 1) / 2 * 0.45, u[:, 6:] * S / 4, torch.arange(B) % 8)


# ---- the reference itself ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [4, 5, 12])
def test_affine_sample_is_grid_sample(S):
    """grid_sample in float64 with align_corners=True and zeros padding; its grid is normalised to [-1, 1] and ordered (x, y, z) =
    (axis 2, axis 1, axis 0)."""
    B, C = 3, 2
    x = torch.randn(B, C, S, S, S, generator=torch.Generator().manual_seed(S), dtype=torch.float64)
    mat = _general_mats(B, S, seed=10 + S)
    mat[2, 3] = 0.7 * S  # a sample pushed mostly outside
    shift = torch.tensor([0.0, 0.25, -0.1])
    q, _ = R._coords(mat, S)
    grid = (2 * q / (S - 1) - 1).flip(-1)
    want = F.grid_sample(x, grid, mode="bilinear", padding_mode="zeros", align_corners=True) + shift.double().view(-1, 1, 1, 1, 1)
    got = R.affine_sample(x, mat, shift)
    assert got.dtype == torch.float64 and float((got - want).abs().max()) <= 1e-12
    outside = got[2] == shift[2].double()  # wholly outside: exactly the shift
    assert bool(outside.any()) and not bool(outside.all())


def test_bound_is_small_finite_and_covers_fp32_arithmetic():
    """The bound against a straight fp32 evaluation on the CPU in the documented order: every element inside.  For unit Gaussians at S = 8 the bound is
    of the order 5 u x 18 voxels x 3 axes x a largest neighbour difference of 3 to 4, a few 1e-5: not vacuous."""
    B, C, S = 2, 2, 8
    x = torch.randn(B, C, S, S, S, generator=torch.Generator().manual_seed(1)).half()
    mat = _general_mats(B, S, seed=2)
    bound, ref = R.bound(x, mat), R.affine_sample(x, mat)
    assert bool(torch.isfinite(bound).all()) and float(bound.max()) < 1e-4
    A, t = mat.view(B, 3, 4)[:, :, :3], mat.view(B, 3, 4)[:, :, 3]
    cen = torch.tensor((S - 1) / 2, dtype=torch.float32)
    r = torch.arange(S, dtype=torch.float32) - cen
    fma = lambda a, b, c: (a.double() * b.double() + c.double()).float()  # one rounding: the double product of two floats is exact
    got = torch.zeros(B, C, S, S, S)
    xf = x.float()
    for b in range(B):
        p = torch.meshgrid(r, r, r, indexing="ij")
        q = [fma(A[b, a, 2], p[2], fma(A[b, a, 1], p[1], fma(A[b, a, 0], p[0], t[b, a] + cen))) for a in range(3)]
        ok = [(qa > -1) & (qa < S) for qa in q]
        f = [torch.where(o, qa, torch.zeros(())).floor() for qa, o in zip(q, ok)]
        w1 = [torch.where(o, qa, torch.zeros(())) - fa for qa, o, fa in zip(q, ok, f)]
        w0 = [1 - w for w in w1]
        acc = torch.zeros(C, S, S, S)
        for d0 in (0, 1):
            for d1 in (0, 1):
                for d2 in (0, 1):
                    idx = [f[0].long() + d0, f[1].long() + d1, f[2].long() + d2]
                    valid = ok[0] & ok[1] & ok[2] & (idx[0] >= 0) & (idx[0] < S) & (idx[1] >= 0) & (idx[1] < S) & (idx[2] >= 0) & (idx[2] < S)
                    w = ((w1[0] if d0 else w0[0]) * (w1[1] if d1 else w0[1])) * (w1[2] if d2 else w0[2])
                    v = xf[b][:, idx[0].clamp(0, S - 1), idx[1].clamp(0, S - 1), idx[2].clamp(0, S - 1)]
                    acc = torch.where(valid, fma(w.expand_as(v), v, acc), acc)
        got[b] = acc
    ratio = ((got.double() - ref).abs() / bound.clamp(min=1e-300)).max()
    assert float(ratio) <= 1.0, float(ratio)


# ---- affine_matrices ----------------------------------------------------------------------------------------------------------------------
def test_rotation_is_orthogonal_with_determinant_one():
    g = torch.Generator().manual_seed(0)
    ang = (torch.rand(16, 3, generator=g, dtype=torch.float64) * 2 - 1) * 180
    m = affine_matrices(ang, torch.ones(16, 3), torch.zeros(16, 3)).double().view(16, 3, 4)
    A = m[:, :, :3]
    assert m.dtype == torch.float64 and float((A @ A.transpose(1, 2) - torch.eye(3, dtype=torch.float64)).abs().max()) < 1e-6
    assert float((torch.linalg.det(A) - 1).abs().max()) < 1e-6 and float(m[:, :, 3].abs().max()) == 0.0


def test_quarter_turns_are_signed_permutations():
    one, zero = torch.ones(1, 3), torch.zeros(1, 3)
    A = lambda ang: affine_matrices(torch.tensor([ang]), one, zero).view(3, 4)[:, :3].tolist()
    assert A([90.0, 0.0, 0.0]) == [[1, 0, 0], [0, 0, -1], [0, 1, 0]]
    assert A([0.0, 90.0, 0.0]) == [[0, 0, 1], [0, 1, 0], [-1, 0, 0]]
    assert A([0.0, 0.0, 90.0]) == [[0, -1, 0], [1, 0, 0], [0, 0, 1]]
    assert A([0.0, 0.0, -90.0]) == [[0, 1, 0], [-1, 0, 0], [0, 0, 1]]
    assert A([180.0, 0.0, 0.0]) == [[1, 0, 0], [0, -1, 0], [0, 0, -1]]
    # R = R2 R1 R0: axis 0 first.  R1(90) R0(90) maps e1 -> R0 e1 = e2 -> R1 e2 = e0
    assert A([90.0, 90.0, 0.0]) == [[0, 1, 0], [0, 0, -1], [-1, 0, 0]]


def test_identity_scale_translation_and_flips():
    one, zero = torch.ones(2, 3), torch.zeros(2, 3)
    eye = torch.tensor([[1.0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]] * 2)
    assert torch.equal(affine_matrices(zero, one, zero), eye) and affine_matrices(zero, one, zero).dtype == torch.float32
    m = affine_matrices(zero, torch.tensor([[2.0, 3.0, 0.5]] * 2), torch.tensor([[1.0, -2.0, 0.25]] * 2), torch.tensor([0, 5])).view(2, 3, 4)
    assert m[0].tolist() == [[2, 0, 0, 1], [0, 3, 0, -2], [0, 0, 0.5, 0.25]]
    assert m[1].tolist() == [[-2, 0, 0, 1], [0, 3, 0, -2], [0, 0, -0.5, 0.25]]  # bits 0 and 2; the translation is not flipped


@pytest.mark.parametrize("S", [4, 5])
def test_flips_compose_on_the_output_side(S):
    """A = R diag(s) F: the result is the flip of the resampled volume, not the resampling of the flipped one."""
    B = 8
    x = torch.randn(B, 1, S, S, S, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    ang, sc, tr = torch.tensor([[20.0, -10.0, 35.0]] * B), torch.tensor([[0.9, 1.1, 1.2]] * B), torch.tensor([[0.5, -0.25, 1.0]] * B)
    flip = torch.arange(B)
    unflipped = R.affine_sample(x, affine_matrices(ang, sc, tr))
    got = R.affine_sample(x, affine_matrices(ang, sc, tr, flip))
    for b in range(B):
        dims = [a + 1 for a in range(3) if (b >> a) & 1]
        want = unflipped[b].flip(dims) if dims else unflipped[b]
        assert float((got[b] - want).abs().max()) <= 1e-6  # the matrices are rounded to fp32 separately
    pre = R.affine_sample(x[7:].flip([2, 3, 4]), affine_matrices(ang[:1], sc[:1], tr[:1]))
    assert float((got[7] - pre[0]).abs().max()) > 1e-3


def test_non_finite_input_raises():
    one, zero = torch.ones(1, 3), torch.zeros(1, 3)
    for bad in (float("nan"), float("inf"), -float("inf")):
        v = torch.tensor([[0.0, bad, 0.0]])
        for args in ((v, one, zero), (zero, v, zero), (zero, one, v)):
            with pytest.raises(ValueError, match="non-finite"):
                affine_matrices(*args)
    with pytest.raises(ValueError):
        affine_matrices(torch.zeros(2, 3), one, zero)


# ---- RandAffine3D -------------------------------------------------------------------------------------------------------------------------
def test_rand_affine_ranges_and_isotropy():
    S, B = 96, 4096
    r = RandAffine3D(rotate_deg=(10.0, 5.0, 0.0), scale=0.1, translate=(0.05, 0.0, 0.02), prob=0.3, isotropic_scale=True, seed=1)
    d = r.draw(B, S)
    assert d is r.last_draw and d["fire"].dtype == torch.bool and tuple(d["angles_deg"].shape) == (B, 3)
    for a, lim in enumerate((10.0, 5.0, 0.0)):
        col = d["angles_deg"][:, a]
        assert float(col.abs().max()) <= lim and (lim == 0 or (float(col.min()) < -0.9 * lim and float(col.max()) > 0.9 * lim))
    for a, lim in enumerate((0.05 * S, 0.0, 0.02 * S)):
        col = d["translate_vox"][:, a]
        assert float(col.abs().max()) <= lim and (lim == 0 or (float(col.min()) < -0.9 * lim and float(col.max()) > 0.9 * lim))
    sc = d["scale"]
    assert float(sc.min()) >= 0.9 and float(sc.max()) <= 1.1 and float(sc.min()) < 0.91 and float(sc.max()) > 1.09
    assert torch.equal(sc[:, 0], sc[:, 1]) and torch.equal(sc[:, 0], sc[:, 2])
    assert abs(float(d["fire"].double().mean()) - 0.3) < 0.03
    aniso = RandAffine3D(10.0, 0.1, 0.05, 0.3, isotropic_scale=False, seed=1).draw(B, S)
    assert not torch.equal(aniso["scale"][:, 0], aniso["scale"][:, 1]) and float(aniso["scale"].min()) >= 0.9 and float(aniso["scale"].max()) <= 1.1
    assert torch.equal(aniso["angles_deg"][:, 0], d["angles_deg"][:, 0]) and torch.equal(aniso["fire"], d["fire"])  # the same stream
    m = r.matrices(d, torch.zeros(B, dtype=torch.uint8))
    assert tuple(m.shape) == (B, 12) and m.dtype == torch.float32 and bool(torch.isfinite(m).all())


def test_rand_affine_prob_extremes_seed_and_refusals():
    assert not bool(RandAffine3D(10.0, 0.1, 0.05, prob=0.0, seed=2).draw(512, 24)["fire"].any())
    assert bool(RandAffine3D(10.0, 0.1, 0.05, prob=1.0, seed=2).draw(512, 24)["fire"].all())
    a, b, c = (RandAffine3D(10.0, 0.1, 0.05, 0.5, seed=s) for s in (7, 7, 8))
    for _ in range(3):
        da, db, dc = a.draw(5, 24), b.draw(5, 24), c.draw(5, 24)
        assert all(torch.equal(da[k], db[k]) for k in da) and not torch.equal(da["angles_deg"], dc["angles_deg"])
    first = a.draw(5, 24)["angles_deg"].clone()
    assert not torch.equal(first, a.draw(5, 24)["angles_deg"])  # a new draw per batch
    for kw in (dict(rotate_deg=181.0), dict(rotate_deg=-1.0), dict(scale=1.0), dict(scale=-0.1), dict(translate=1.0), dict(prob=1.5),
               dict(rotate_deg=(1.0, 2.0)), dict(scale=float("nan"))):
        with pytest.raises(ValueError):
            RandAffine3D(**{**dict(rotate_deg=10.0, scale=0.1, translate=0.05, prob=0.5), **kw})


# ---- inertness ------------------------------------------------------------------------------------------------------------------------------
def test_an_attached_affine_leaves_the_flip_and_shift_stream_alone():
    plain = DeviceAugment(flip_prob=0.3, shift_offsets=0.1, shift_prob=0.5, seed=11)
    with_affine = DeviceAugment(flip_prob=0.3, shift_offsets=0.1, shift_prob=0.5, seed=11, affine=RandAffine3D(10.0, 0.1, 0.05, 0.5, seed=11))
    assert plain.draw_affine(4, 24, torch.zeros(4, dtype=torch.uint8)) == (None, None)
    for B in (4, 4, 3, 7, 1):
        (f0, s0), (f1, s1) = plain.draw(B), with_affine.draw(B)
        mat, fire = with_affine.draw_affine(B, 24, f1)
        assert torch.equal(f0, f1) and torch.equal(s0, s1)
        assert tuple(mat.shape) == (B, 12) and fire.dtype == torch.uint8 and tuple(fire.shape) == (B,)
        d = with_affine.affine.last_draw
        assert torch.equal(mat, affine_matrices(d["angles_deg"], d["scale"], d["translate_vox"], f1))  # the batch's flips are folded in


# ---- configuration and arguments ------------------------------------------------------------------------------------------------------------
def _parse(monkeypatch, tmp_path, *extra, yaml="MODEL:\n  NAME: vit\n"):
    import main_downstream
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(yaml)
    monkeypatch.setattr(sys, "argv", ["main_downstream.py", "--cfg", str(cfg), "--model_name", "vit", *extra])
    return main_downstream.parse_option()[1]


def test_config_defaults_flags_and_refusals(monkeypatch, tmp_path):
    import config as cfgmod
    t = cfgmod._C.TRAIN
    assert t.AFFINE_PROB == 0.0 and t.AFFINE_ISOTROPIC is True and 0 <= t.AFFINE_SCALE < 1 and 0 <= t.AFFINE_TRANSLATE < 1  # off by default
    assert _parse(monkeypatch, tmp_path).TRAIN.AFFINE_PROB == 0.0
    t = _parse(monkeypatch, tmp_path, "--affine_prob", "0.5", "--affine_rotate", "10", "--affine_scale", "0.1", "--affine_translate", "0.05").TRAIN
    assert (t.AFFINE_PROB, list(t.AFFINE_ROTATE), t.AFFINE_SCALE, t.AFFINE_TRANSLATE) == (0.5, [10.0], 0.1, 0.05)
    t = _parse(monkeypatch, tmp_path, "--affine_rotate", "10", "5", "0").TRAIN
    assert list(t.AFFINE_ROTATE) == [10.0, 5.0, 0.0]
    on = "TRAIN:\n  AFFINE_PROB: 0.5\n  AFFINE_ROTATE: [20, 20, 5]\n  AFFINE_SCALE: 0.2\n  AFFINE_TRANSLATE: 0.1\n  AFFINE_ISOTROPIC: False\nMODEL:\n  NAME: vit\n"
    t = _parse(monkeypatch, tmp_path, yaml=on).TRAIN
    assert (t.AFFINE_PROB, list(t.AFFINE_ROTATE), t.AFFINE_SCALE, t.AFFINE_TRANSLATE, t.AFFINE_ISOTROPIC) == (0.5, [20, 20, 5], 0.2, 0.1, False)
    # an explicit 0 on the command line reaches the config (it overrides the file), as --drop_path 0 does
    t = _parse(monkeypatch, tmp_path, "--affine_prob", "0", "--affine_rotate", "0", "--affine_scale", "0", "--affine_translate", "0", yaml=on).TRAIN
    assert (t.AFFINE_PROB, list(t.AFFINE_ROTATE), t.AFFINE_SCALE, t.AFFINE_TRANSLATE) == (0.0, [0.0], 0.0, 0.0)
    for flags, key in ((("--affine_prob", "1.5"), "AFFINE_PROB"), (("--affine_prob", "-0.1"), "AFFINE_PROB"), (("--affine_prob", "nan"), "AFFINE_PROB"),
                       (("--affine_rotate", "181"), "AFFINE_ROTATE"), (("--affine_rotate", "-1"), "AFFINE_ROTATE"),
                       (("--affine_rotate", "10", "10"), "AFFINE_ROTATE"), (("--affine_scale", "1"), "AFFINE_SCALE"),
                       (("--affine_scale", "-0.5"), "AFFINE_SCALE"), (("--affine_translate", "1"), "AFFINE_TRANSLATE"),
                       (("--affine_translate", "-0.01"), "AFFINE_TRANSLATE"), (("--opts", "TRAIN.AFFINE_ISOTROPIC", "None"), "AFFINE_ISOTROPIC")):
        with pytest.raises(ValueError, match=f"TRAIN.{key}"):
            _parse(monkeypatch, tmp_path, *flags)
