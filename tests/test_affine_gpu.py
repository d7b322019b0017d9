"""GPU: hct_affine_augment through the C ABI against tests/affine_ref.py, the loader paths that carry it, and main_downstream.py end
to end.

Held to equality wherever the arithmetic is exact: `mat == NULL` and `fire == 0` against hct_gather_augment / hct_augment_volume
themselves (all eight flip patterns), lattice maps (identity, folded flips, the 24 signed permutations of determinant +1, integer
translations that push part or all of the volume outside) against torch indexing on the fp32 cast, and integer-valued inputs under
translations by multiples of 1/4 voxel against float64 (weights are multiples of 1/64, products of them with integers up to 1024
and their sums fit in 24 bits: nothing rounds).  General maps -- Gaussian inputs, an outlier voxel, a constant volume; rotations up to 30
degrees, scale 0.8 to 1.25, translations up to S / 4, a different matrix per sample -- are held element by element to
`affine_ref.bound`, which is derived from the header's order of operations (its docstring counts the roundings); no element is left out.

Measured on an MI355X: worst |got - ref| / bound over every general-map case 0.451 (kernel; the constant volume), 0.135 (loader paths).

Every kernel call writes into a NaN-filled output between guard bands that must come back untouched and is made twice on fresh
outputs that must agree bit for bit.  Pool slots the batch does not use hold NaN, so a tap read outside a sample's own volume shows up
even at weight zero.  Shapes: S 8 takes 16-byte loads where the call is hct_gather_augment, 12 and 20 the 8-byte ones, 4 has one store
per row; all of them are one trip of the kernel's grid-stride loop, so `test_more_than_one_trip` adds [48, 1, 48^3]."""
import os
import socket
import subprocess
import sys

import pytest
import torch

from headct_foundation_amd import _lib
from headct_foundation_amd._lib import HCT_BF16, HCT_F16, HCT_F32
from headct_foundation_amd.data import (DeviceAugment, DevicePool, LabelledVolumes, RandAffine3D, VolumeCache, affine_augment, affine_matrices,
                                        gather_augment, get_finetune_dataloaders)
from tests import affine_ref as R
from tests.test_assembly_kernels_gpu import _Out, _p, _st, _twice
from tests.test_labelled_gpu import _DeviceLoader, _label_csvs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
CODE = {F16: HCT_F16, BF16: HCT_BF16, F32: HCT_F32}
HCT_E_BADARG = -1
N_SLOTS = 4
SLOTS = {1: [[2], [-1]], 3: [[1, -1, 1], [3, 99, 0]]}  # repeats, the placeholder, a slot out of range
MODES = [("pool", F16), ("stack", F16), ("stack", BF16), ("stack", F32)]
SHAPES = [(S, C, B) for S in (4, 8, 12, 20) for C in (1, 3) for B in (1, 3)]
WORST = {"kernel": 0.0, "loader": 0.0}


def _bits(t):
    return t.contiguous().view(torch.int32)


class _Case:
    """The input of one call: a pool whose unused slots are NaN (mode "pool") or a stacked batch, and the batch it stands for on
    the CPU (`x` [B, C, S, S, S] in the input dtype, zeros for a placeholder)."""

    def __init__(self, mode, dtype, x, slots, dev):
        B = x.shape[0]
        self.mode, self.dtype, self.B, self.C, self.S = mode, dtype, B, x.shape[1], x.shape[2]
        if mode == "pool":
            pool = torch.full((N_SLOTS,) + tuple(x.shape[1:]), float("nan"), dtype=dtype)
            self.x = x.clone()
            for b, s in enumerate(slots):
                if 0 <= s < N_SLOTS:
                    pool[s] = x[slots.index(s)]  # a repeated slot serves the first sample's volume to every sample that names it
                    self.x[b] = pool[s]
                else:
                    self.x[b] = 0
            self.dev_in, self.slot = pool.to(dev), torch.tensor(slots, dtype=torch.int32, device=dev)
        else:
            self.x, self.dev_in, self.slot = x, x.to(dev), None

    def call(self, lib, mat=None, fire=None, flip=None, shift=None):
        o = _Out((self.B, self.C, self.S, self.S, self.S), F32, self.dev_in.device)
        up = lambda t, dt: None if t is None else t.to(device=self.dev_in.device, dtype=dt).contiguous()
        tabs = [up(mat, F32), up(fire, torch.uint8), up(flip, torch.uint8), up(shift, F32)]
        rc = lib.hct_affine_augment(self.dev_in.data_ptr(), CODE[self.dtype], _p(self.slot), N_SLOTS, o.ptr, self.B, self.C, self.S, *[_p(t) for t in tabs],
                                    _st())
        assert rc == 0, lib.hct_last_error_string()
        o.keep = tabs
        return {"out": o}

    def run(self, lib, **kw):
        return _twice(lambda: self.call(lib, **kw))["out"]


def _cases(x_of, S, C, B, dev, modes=MODES):
    """One case per mode and slot pattern; x_of(dtype) -> [B, C, S, S, S] of that dtype on the CPU."""
    for mode, dtype in modes:
        for slots in (SLOTS[B] if mode == "pool" else [None]):
            yield _Case(mode, dtype, x_of(dtype), slots, dev)


def _gauss(S, C, B, seed):
    x = torch.randn(B, C, S, S, S, generator=torch.Generator().manual_seed(seed))
    return lambda dtype: x.to(dtype)


# ---- 1. the plain arithmetic ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,C,B", SHAPES)
def test_without_a_matrix_or_a_firing_sample_it_is_the_plain_kernel(lib, cuda, S, C, B):
    garbage = torch.tensor([[3.0, -1e4, 0.5, 7.0, 1e20, 2.0, -3.0, 1.5, 0.25, 9.0, -1e-30, 123.0]]).expand(B, 12)  # never read where fire is 0
    for case in _cases(_gauss(S, C, B, 1), S, C, B, cuda):
        for r in range(8):
            flip = torch.tensor([(r + 3 * b) % 8 for b in range(B)], dtype=torch.uint8)
            shift = torch.tensor([0.05, -0.1, 0.0][:B])
            for f, s in [(flip, shift), (flip, None)] + ([(None, shift), (None, None)] if r == 0 else []):
                def parent():
                    o = _Out((B, C, S, S, S), F32, cuda)
                    fd, sd = (None if t is None else t.to(cuda) for t in (f, s))
                    if case.mode == "pool":
                        rc = lib.hct_gather_augment(case.dev_in.data_ptr(), case.slot.data_ptr(), o.ptr, B, C, S, N_SLOTS, _p(fd), _p(sd), _st())
                    else:
                        rc = lib.hct_augment_volume(case.dev_in.data_ptr(), CODE[case.dtype], o.ptr, B, C, S, _p(fd), _p(sd), _st())
                    assert rc == 0
                    o.keep = (fd, sd)
                    return {"out": o}
                want = _twice(parent)["out"]
                assert torch.equal(_bits(want), _bits(R.plain(case.x, f, s)))
                assert torch.equal(_bits(case.run(lib, flip=f, shift=s)), _bits(want)), (case.mode, case.dtype, "mat NULL", r)
                got = case.run(lib, mat=garbage, fire=torch.zeros(B, dtype=torch.uint8), flip=f, shift=s)
                assert torch.equal(_bits(got), _bits(want)), (case.mode, case.dtype, "fire 0", r)


# ---- 2. lattice maps ----------------------------------------------------------------------------------------------------------------------
def _lattice_maps(S):
    maps = [(perm, sign, (0, 0, 0)) for perm, sign in R.rotations()]  # the identity is among them
    maps += [((0, 1, 2), tuple(-1 if (f >> a) & 1 else 1 for a in range(3)), (0, 0, 0)) for f in range(1, 8)]  # flips (determinant -1 too)
    maps += [((0, 1, 2), (1, 1, 1), t) for t in ((1, 0, 0), (0, -2, 0), (0, 0, 3), (-1, 2, -3), (S - 1, 0, 0), (0, 1 - S, 1), (S, 0, 0), (0, 0, -S),
                                                  (2 * S, -3 * S, 5))]
    maps += [((2, 0, 1), (-1, 1, -1), (1, -1, 2)), ((1, 0, 2), (1, -1, -1), (0, 0, S - 2))]
    return maps


@pytest.mark.parametrize("S,C,B", SHAPES)
def test_lattice_maps_are_torch_indexing(lib, cuda, S, C, B):
    maps = _lattice_maps(S)
    shift = torch.tensor([0.0, 0.125, -0.0625][:B])
    for case in _cases(_gauss(S, C, B, 2), S, C, B, cuda):
        for k in range(0, len(maps), B):
            chunk = [maps[(k + b) % len(maps)] for b in range(B)]
            mat = torch.stack([R.lattice_mat(*m) for m in chunk])
            for sh in (None, shift):
                got = case.run(lib, mat=mat, fire=torch.ones(B, dtype=torch.uint8), flip=torch.full((B,), 7, dtype=torch.uint8), shift=sh)  # flip is ignored
                for b, m in enumerate(chunk):
                    want = R.lattice(case.x[b], *m, None if sh is None else sh[b])
                    assert torch.equal(_bits(got[b]), _bits(want)), (case.mode, case.dtype, m)
        # the host's folded flips are the lattice flips, and fire == NULL fires everywhere
        flip = torch.tensor([(5 + b) % 8 for b in range(B)], dtype=torch.uint8)
        zero, one = torch.zeros(B, 3), torch.ones(B, 3)
        got = case.run(lib, mat=affine_matrices(zero, one, zero, flip))
        assert torch.equal(_bits(got), _bits(R.plain(case.x, flip))), (case.mode, case.dtype, "folded flips")
        quarter = case.run(lib, mat=affine_matrices(torch.tensor([[0.0, 0.0, 90.0]] * B), one, zero))
        assert torch.equal(_bits(quarter), _bits(torch.stack([R.lattice(case.x[b], (1, 0, 2), (-1, 1, 1), (0, 0, 0)) for b in range(B)])))


# ---- 3. exact fractions ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,C,B", SHAPES)
def test_quarter_voxel_translations_of_integers_are_exact(lib, cuda, S, C, B):
    g = torch.Generator().manual_seed(3)
    ints = torch.randint(-1024, 1025, (B, C, S, S, S), generator=g)
    x_of = lambda dtype: (ints // 8 * 8 if dtype == BF16 else ints).to(dtype)  # bf16 holds the multiples of 8 up to 1024
    moves = [(0.25, 0.0, 0.0), (0.0, -0.5, 0.75), (1.25, 2.5, -0.25), (-0.75, 0.25, S - 0.5), (0.5 - S, 0.5, 0.5), (0.25, 0.25, 0.25), (S / 4, -S / 2 + 0.25, 1.75)]
    rots = R.rotations()
    for case in _cases(x_of, S, C, B, cuda):
        assert torch.equal(case.x.double(), case.x.double().round())
        for k in range(0, len(moves), B):
            mat = torch.stack([R.lattice_mat(*rots[(5 * (k + b)) % 24], moves[(k + b) % len(moves)]) for b in range(B)])
            for sh in (None, torch.tensor([0.5, -2.0, 0.25][:B])):
                got = case.run(lib, mat=mat, shift=sh)
                assert torch.equal(got.double(), R.affine_sample(case.x, mat, sh)), (case.mode, case.dtype, mat.tolist())


# ---- 4. general maps ------------------------------------------------------------------------------------------------------------------------
def _general_mats(B, S, seed):
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(B, 9, generator=g, dtype=torch.float64) * 2 - 1
    scale = 0.8 + (u[:, 3:6] + 1) / 2 * 0.45
    return affine_matrices(u[:, :3] * 30.0, scale, u[:, 6:] * S / 4, torch.tensor([(seed + b) % 8 for b in range(B)]))


def _within_bound(got, x, mat, shift, fire, flip, what, key="kernel"):
    ref, bound = R.affine_sample(x, mat, shift), R.bound(x, mat, shift)
    err = (got.double() - ref).abs()
    ok = torch.ones(got.shape[0], dtype=torch.bool) if fire is None else fire.bool()
    ratio = float((err[ok] / bound[ok]).nan_to_num(nan=0.0).max()) if bool(ok.any()) else 0.0  # 0 / 0: an exact value where the bound is 0
    WORST[key] = max(WORST[key], ratio)
    print(f"{what}: worst |got - ref| / bound = {ratio:.3f} (worst so far {WORST[key]:.3f})")
    assert bool((err[ok] <= bound[ok]).all()), (what, ratio)
    if not bool(ok.all()):  # samples that did not fire: the plain arithmetic, bit for bit
        assert torch.equal(_bits(got[~ok]), _bits(R.plain(x[~ok], flip[~ok], None if shift is None else shift[~ok]))), what


@pytest.mark.parametrize("S,C,B", SHAPES)
def test_general_maps_within_the_derived_bound(lib, cuda, S, C, B):
    gauss = _gauss(S, C, B, 4)

    def outlier(dtype):
        x = gauss(dtype).clone()
        x[B - 1, C - 1, S // 2, 1, S - 2] = 3.0e4
        return x
    constant = lambda dtype: torch.full((B, C, S, S, S), 0.75, dtype=dtype)
    for name, x_of in (("gaussian", gauss), ("outlier", outlier), ("constant", constant)):
        for i, case in enumerate(_cases(x_of, S, C, B, cuda)):
            mat = _general_mats(B, S, seed=10 * S + i)
            shift = torch.tensor([0.07, -0.1, 0.0][:B])
            what = f"S {S} C {C} B {B} {name} {case.mode} {case.dtype}"
            _within_bound(case.run(lib, mat=mat, shift=shift), case.x, mat, shift, None, None, what)
            fire, flip = torch.tensor([1, 0, 1][:B], dtype=torch.uint8), torch.tensor([6, 3, 5][:B], dtype=torch.uint8)
            _within_bound(case.run(lib, mat=mat, fire=fire, flip=flip), case.x, mat, None, fire, flip, what + " mixed fire")


def test_more_than_one_trip(lib, cuda):
    """A sample gets min(ceil(S^3 / 4 / 256), ceil(4096 / B)) blocks of 256 threads, each thread 4 outputs per trip of its grid-stride
    loop.  Every shape above is one trip; S = 48 with B = 48 has 27648 threads' work per sample for 86 blocks = 22016 threads: a
    second trip for a quarter of them, the path of a fine-tuning batch ([64, 3, 96^3]: 4 trips).  Samples that fire are held to the
    bound, the others bit for bit."""
    S, C, B = 48, 1, 48
    x = torch.randn(B, C, S, S, S, generator=torch.Generator().manual_seed(5)).half()
    case = _Case("stack", F16, x, None, cuda)
    mat = _general_mats(B, S, seed=6)
    fire, flip = (torch.arange(B) % 3 != 0).to(torch.uint8), (torch.arange(B) % 8).to(torch.uint8)
    shift = torch.linspace(-0.1, 0.1, B)
    _within_bound(case.run(lib, mat=mat, fire=fire, flip=flip, shift=shift), x, mat, shift, fire, flip, "two trips")


# ---- 5. far outside -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,C", [(8, 3), (12, 1)])
def test_a_sample_mapped_far_outside_is_its_shift_and_its_neighbours_do_not_notice(lib, cuda, S, C):
    B = 3
    shift = torch.tensor([0.07, -0.1, 0.03])
    for case in _cases(_gauss(S, C, B, 7), S, C, B, cuda, modes=[("pool", F16), ("stack", F32)]):
        near = _general_mats(B, S, seed=8)
        base = case.run(lib, mat=near, shift=shift)
        for b in range(B):
            for col, big in ((3, 1e30), (7, -1e30), (11, 1e30), (0, 1e30), (5, -3e38)):  # translations, and huge entries of A
                mat = near.clone()
                mat[b, col] = big
                got = case.run(lib, mat=mat, shift=shift)
                # a huge entry of A too: |A_ak p_k| >= 5e29 at every voxel (p is a half-integer, S being even), infinite for -3e38
                assert bool((got[b] == shift[b]).all()), (case.mode, b, col)
                others = [o for o in range(B) if o != b]
                assert torch.equal(_bits(got[others]), _bits(base[others])), (case.mode, b, col)


# ---- 6. what is refused ----------------------------------------------------------------------------------------------------------------------
def test_refusals(lib, cuda):
    B, C, S = 2, 1, 8
    x = torch.randn(B, C, S, S, S).half().to(cuda)
    o = _Out((B, C, S, S, S), F32, cuda)
    mat = affine_matrices(torch.zeros(B, 3), torch.ones(B, 3), torch.zeros(B, 3)).to(cuda)
    fire = torch.ones(B, dtype=torch.uint8, device=cuda)
    slot = torch.zeros(B, dtype=torch.int32, device=cuda)
    ok = dict(inp=x.data_ptr(), code=HCT_F16, slot=None, n=0, out=o.ptr, B=B, C=C, S=S, mat=mat.data_ptr(), fire=fire.data_ptr())
    call = lambda **kw: lib.hct_affine_augment(*[{**ok, **kw}[k] for k in ("inp", "code", "slot", "n", "out", "B", "C", "S", "mat", "fire")], None, None, _st())
    for kw in (dict(S=10), dict(S=0), dict(S=1028), dict(mat=None), dict(code=7), dict(out=None), dict(inp=None), dict(B=0), dict(C=40000),
               dict(out=o.ptr + 4), dict(slot=slot.data_ptr(), n=0), dict(slot=slot.data_ptr(), n=2, code=HCT_F32)):
        assert call(**kw) == HCT_E_BADARG, kw
        assert b"hct_affine_augment" in lib.hct_last_error_string(), kw
    torch.cuda.synchronize()
    o.result()
    assert o.untouched()
    assert call() == 0
    # the Python doors refuse a non-finite matrix given on the CPU before anything is launched
    pool = torch.zeros(2, C, S, S, S, dtype=F16, device=cuda)
    for bad in (float("nan"), float("inf"), -float("inf")):
        m = mat.cpu().clone()
        m[1, 5] = bad
        with pytest.raises(ValueError, match="non-finite"):
            affine_augment(x, m)
        with pytest.raises(ValueError, match="non-finite"):
            gather_augment(pool, torch.tensor([0, 1], dtype=torch.int32), mat=m)
    with pytest.raises(ValueError, match="fire without mat"):
        gather_augment(pool, torch.tensor([0, 1], dtype=torch.int32), fire=fire)
    with pytest.raises(ValueError, match="12"):
        affine_augment(x, mat.cpu()[:1])
    assert torch.equal(affine_augment(x, mat.cpu()), x.float())  # the identity through the door


# ---- 7. loader paths ------------------------------------------------------------------------------------------------------------------------
PATHS = [f"/scans/{'bad' if i == 5 else 'ok'}_{i}.nii.gz" for i in range(11)]
ORDER = [0, 5, 3, 3, 10, 7, 5, 1, 2, 9, 4, 8, 6]


def _loader(tmp_path, cuda, sub, pooled, prob):
    cache = VolumeCache(tmp_path / sub, 12, 3, loader=_DeviceLoader())
    pool = DevicePool(cache, 11, cuda, 4, num_workers=3) if pooled else None
    aug = None
    if prob is not None:
        aug = DeviceAugment(flip_prob=0.3, shift_offsets=0.1, shift_prob=0.5, seed=17, affine=RandAffine3D(20.0, 0.15, 0.1, prob, seed=17))
    label_of = {p: i % 2 for i, p in enumerate(PATHS)}
    return LabelledVolumes(PATHS, label_of, ORDER, cache, 4, cuda, aug, pool, num_workers=3), cache


def _with_draws(loader):
    out = []
    for v, t, names in loader:
        draw = None
        if loader.augment is not None:
            draw = (loader.augment.last_draw[0].clone(), loader.augment.last_draw[1].clone(), {k: d.clone() for k, d in loader.augment.affine.last_draw.items()})
        out.append((v, t, names, draw))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("prob", [1.0, 0.5])
def test_pool_path_equals_stacked_path_and_both_the_reference(lib, cuda, tmp_path, prob):
    (on, cache), (off, _) = _loader(tmp_path, cuda, "on", True, prob), _loader(tmp_path, cuda, "off", False, prob)
    fired = 0
    for epoch in range(2):
        a, b = _with_draws(on), _with_draws(off)
        assert len(a) == len(b) == 4
        for k, ((va, ta, na, da), (vb, tb, nb, db)) in enumerate(zip(a, b)):
            assert torch.equal(_bits(va), _bits(vb)) and torch.equal(ta, tb) and na == nb, (epoch, k)
            flip, shift, d = da
            assert torch.equal(flip, db[0]) and torch.equal(shift, db[1]) and all(torch.equal(d[key], db[2][key]) for key in d)
            x = torch.stack([torch.zeros(3, 12, 12, 12, dtype=F16) if n == "None" else cache.get(n, "cpu") for n in na])
            mat = affine_matrices(d["angles_deg"], d["scale"], d["translate_vox"], flip)
            _within_bound(va.cpu(), x, mat, shift, d["fire"], flip, f"loader prob {prob} epoch {epoch} batch {k}", key="loader")
            fired += int(d["fire"].sum())
            assert float(d["angles_deg"].abs().max()) <= 20.0 and float(d["translate_vox"].abs().max()) <= 1.2
    assert (fired == 26) if prob == 1.0 else (0 < fired < 26)


def test_validation_and_test_loaders_keep_the_plain_cast(lib, cuda, tmp_path, capsys):
    for pooled in (True, False):
        loader, cache = _loader(tmp_path, cuda, f"val{pooled}", pooled, None)
        batches = [(v, names) for v, _, names in loader]
        torch.cuda.synchronize()
        for v, names in batches:
            want = torch.stack([torch.zeros(3, 12, 12, 12) if n == "None" else cache.get(n, "cpu").float() for n in names])
            assert torch.equal(_bits(v.cpu()), _bits(want))
    capsys.readouterr()


def _finetune_config(tmp_path, csvs, **train):
    from config import _C
    cfg = _C.clone()
    cfg.defrost()
    cfg.DATA.SYNTHETIC, cfg.DATA.BATCH_SIZE, cfg.DATA.CACHE_DIR = False, 4, str(tmp_path / "cache")
    cfg.DATA.DATASET, cfg.TRAIN.LABEL_NAME, cfg.DATA.TRAIN_SAMPLES_PER_RANK = "rsna", "any", 8
    cfg.MODEL.ROI, cfg.MODEL.IN_CHANS, cfg.VIT.INPUT_SIZE, cfg.VIT.IN_CHANS = [16, 16, 16], 1, 16, 1
    cfg.DATA.TRAIN_CSV_PATH, cfg.DATA.VAL_CSV_PATH, cfg.DATA.TEST_CSV_PATH = csvs
    for k, v in train.items():
        setattr(cfg.TRAIN, k, v)
    return cfg


def _two_epochs(loader):
    out = [[(v, t, names) for v, t, names in loader] for _ in range(2)]
    torch.cuda.synchronize()
    return [(v.cpu(), t.cpu(), names) for epoch in out for v, t, names in epoch]


def test_prob_zero_is_the_loader_without_the_feature(lib, cuda, tmp_path):
    csvs, _ = _label_csvs(tmp_path)
    off = get_finetune_dataloaders(_finetune_config(tmp_path, csvs, AFFINE_PROB=0.0, AFFINE_ROTATE=[30.0], AFFINE_SCALE=0.2), cuda, 0, 1)
    assert off[0].augment.affine is None
    got = _two_epochs(off[0])
    bare = get_finetune_dataloaders(_finetune_config(tmp_path, csvs), cuda, 0, 1)
    bare[0].augment = DeviceAugment(flip_prob=0.1, shift_offsets=0.1, shift_prob=0.5, seed=bare[0].sampler.gen.initial_seed(), affine=None)
    want = _two_epochs(bare[0])
    assert len(got) == len(want) == 4
    for (v, t, names), (w, u, others) in zip(got, want):
        assert torch.equal(_bits(v), _bits(w)) and torch.equal(t, u) and names == others
    # with the affine on: the same scans and labels in the same order, resampled; validation and test untouched
    on = get_finetune_dataloaders(_finetune_config(tmp_path, csvs, AFFINE_PROB=1.0, AFFINE_ROTATE=[30.0], AFFINE_SCALE=0.2), cuda, 0, 1)
    aff = on[0].augment.affine
    assert isinstance(aff, RandAffine3D) and (aff.rotate_deg, aff.scale, aff.translate, aff.prob, aff.isotropic_scale) == ((30.0,) * 3, 0.2, (0.05,) * 3, 1.0, True)
    moved = _two_epochs(on[0])
    for (v, t, names), (w, u, others) in zip(moved, want):
        assert torch.equal(t, u) and names == others and not torch.equal(v, w)
    assert on[1].augment is None and on[2].augment is None
    for k in (1, 2):
        for (v, t, names), (w, u, others) in zip(_two_epochs(on[k]), _two_epochs(off[k])):
            assert torch.equal(_bits(v), _bits(w)) and torch.equal(t, u) and names == others


# ---- 8. main_downstream.py end to end ---------------------------------------------------------------------------------------------------------
def test_main_downstream_with_the_affine(lib, cuda, tmp_path):
    from headct_foundation_amd.dino_model import ViTBackbone
    (train_csv, val_csv, test_csv), _ = _label_csvs(tmp_path)
    torch.manual_seed(0)
    vit = ViTBackbone(in_chans=3, img_size=24, patch_size=12, hidden_size=48, mlp_dim=96, num_layers=2, num_heads=3)
    torch.save({"state_dict": {"module." + k: v for k, v in vit.state_dict().items()}, "epoch": 3}, tmp_path / "pre.pt")
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("MODEL:\n  NAME: vit\n  ROI: [24, 24, 24]\n")
    opts = ["DATA.SYNTHETIC", "False", "DATA.TRAIN_SAMPLES_PER_RANK", "8", "DATA.CACHE_DIR", str(tmp_path / "cache"), "VIT.INPUT_SIZE", "24",
            "VIT.PATCH_SIZE", "12", "VIT.HIDDEN_SIZE", "48", "VIT.MLP_DIM", "96", "VIT.NUM_LAYERS", "2", "VIT.NUM_HEADS", "3",
            "TRAIN.VAL_EVERY", "1", "MODEL.DIR", str(tmp_path / "out"), "MODEL.SAVE_NAME", "ft.pt", "LOG.OUTPUT_DIR", str(tmp_path / "log"),
            "PREDS_SAVE_NAME", "run"]
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = str(sock.getsockname()[1])
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1", "--master-addr", "127.0.0.1", "--master-port", port,
           os.path.join(ROOT, "main_downstream.py"), "--cfg", str(cfg), "--model_name", "vit", "--model_load_path", str(tmp_path / "pre.pt"),
           "--classifier", "linear", "--batch_size", "4", "--max_epochs", "1", "--grad_clip", "1.0", "--base_lr", "1e-4", "--dataset", "rsna",
           "--label_name", "any", "--train_csv_path", train_csv, "--val_csv_path", val_csv, "--test_csv_path", test_csv,
           "--affine_prob", "0.5", "--affine_rotate", "10", "--affine_scale", "0.1", "--affine_translate", "0.05"]
    r = subprocess.run(cmd + ["--opts"] + opts, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600)
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-4000:]
    assert "Random affine: TRAIN.AFFINE_PROB 0.5, TRAIN.AFFINE_ROTATE [10.0] degrees, TRAIN.AFFINE_SCALE 0.1" in log, log[-4000:]
    assert "TRAIN.AFFINE_TRANSLATE 0.05" in log and "Epoch 1/1 [2/2]" in log and "Final test loss" in log and "Error loading" not in log, log[-4000:]
    assert os.path.isfile(tmp_path / "out" / "ft.pt")
