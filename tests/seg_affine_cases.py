"""The cases hct_affine_labels is held to, shared by tests/test_seg_affine_gpu.py (which runs the kernel on them) and
tests/test_seg_affine_cpu.py (which shows that planted faults in the reference do not get through them, and that the excused share
of the general maps stays below the cap).  `verify(case, got)` is the one judgement both files use.

A case: name, kind ("exact": every voxel bit-equal to the reference; "general": bit-equal outside `near_tie`, one of the candidate
values inside it, the excused share of the firing samples' voxels at most CAP), S, pool uint8 [n, S, S, S], slots, mat fp32 [B, 12]
or None, fire / flip uint8 [B] or None, outside.  Label volumes are (7 i + 13 j + 29 k + 31 s) % 251: neighbours along every axis
differ, and so do the volumes of different slots."""
import numpy as np
import torch

from headct_foundation_amd.data import affine_matrices
from tests import affine_ref
from tests import seg_affine_ref as R

CAP = 0.01  # the largest share of voxels a general-map case may excuse as near a tie
N_SLOTS = 3


def volumes(n, S):
    s, i, j, k = np.indices((n, S, S, S))
    return ((7 * i + 13 * j + 29 * k + 31 * s) % 251).astype(np.uint8)


def gathered(case):
    """The batch the slots stand for, [B, S, S, S]; a slot outside the pool reads as 255 (and `expected` keeps it so)."""
    S = case["S"]
    return np.stack([case["pool"][s] if 0 <= s < case["pool"].shape[0] else np.full((S, S, S), 255, np.uint8) for s in case["slots"]])


def expected(case, ref=R.affine_labels_ref):
    out = ref(gathered(case), None if case["mat"] is None else case["mat"].numpy(), case["fire"], case["flip"], case["outside"])
    for b, s in enumerate(case["slots"]):
        if not 0 <= s < case["pool"].shape[0]:
            out[b] = 255  # the placeholder: all-ignore whatever the map and `outside`
    return out


def firing(case):
    B = len(case["slots"])
    if case["mat"] is None:
        return np.zeros(B, dtype=bool)
    return np.ones(B, dtype=bool) if case["fire"] is None else np.asarray(case["fire"]).astype(bool)


def tie_mask(case):
    """near_tie under the derived delta, [B, S, S, S]; False for samples that do not fire or read the placeholder."""
    B, S = len(case["slots"]), case["S"]
    mask = np.zeros((B, S, S, S), dtype=bool)
    for b in np.nonzero(firing(case))[0]:
        if 0 <= case["slots"][b] < case["pool"].shape[0]:
            m = case["mat"][b:b + 1].numpy()
            mask[b] = R.near_tie(m, S, R.delta(m, S))[0]
    return mask


def tie_share(case):
    f = firing(case)
    return float(tie_mask(case)[f].mean()) if f.any() else 0.0


def verify(case, got):
    """(ok, what went wrong or a figure) for an output uint8 [B, S, S, S] of the case."""
    want = expected(case)
    got = np.asarray(got)
    if got.shape != want.shape or got.dtype != np.uint8:
        return False, f"{case['name']}: shape / dtype {got.shape} {got.dtype}"
    if case["kind"] == "exact":
        bad = int((got != want).sum())
        return bad == 0, f"{case['name']}: {bad} voxels differ from the reference"
    tie = tie_mask(case)
    bad = int(((got != want) & ~tie).sum())
    if bad:
        return False, f"{case['name']}: {bad} voxels away from every tie differ from the reference"
    share = tie_share(case)
    if share > CAP:
        return False, f"{case['name']}: {share:.4f} of the voxels excused, cap {CAP}"
    lab = gathered(case)
    for b in np.nonzero(tie.any(axis=(1, 2, 3)))[0]:
        m = case["mat"][b:b + 1].numpy()
        allowed = R.candidates(lab[b], m, case["S"], R.delta(m, case["S"])[0], case["outside"])
        i, j, k = np.nonzero(tie[b])
        if not allowed[got[b][i, j, k], i, j, k].all():
            return False, f"{case['name']}: sample {b} has a value near a tie that is neither candidate nor `outside`"
    return True, f"{case['name']}: excused share {share:.5f}"


# ---- lattice maps: index arithmetic, no floating point -----------------------------------------------------------------------------------
def folded_lattice_mat(perm, sign, t, flip):
    """lattice_mat with the flips folded in as affine_matrices folds them: column k of A times -1 where bit k of `flip` is set."""
    m = affine_ref.lattice_mat(perm, sign, t).view(3, 4).clone()
    for k in range(3):
        if (flip >> k) & 1:
            m[:, k] = -m[:, k]
    return m.reshape(12)


def lattice_index(vol, perm, sign, t, flip, outside):
    """out[i] = vol[q], q_a = i'[perm[a]] (or S - 1 - i'[perm[a]] where sign[a] < 0) + t[a], i' = i with the flipped axes reversed;
    `outside` where q leaves the volume.  Integers only."""
    S = vol.shape[0]
    i = list(np.indices((S, S, S)))
    for k in range(3):
        if (flip >> k) & 1:
            i[k] = S - 1 - i[k]
    q = [(i[perm[a]] if sign[a] > 0 else S - 1 - i[perm[a]]) + int(t[a]) for a in range(3)]
    ok = np.logical_and.reduce([(x >= 0) & (x < S) for x in q])
    v = vol[tuple(np.clip(x, 0, S - 1) for x in q)]
    return np.where(ok, v, np.uint8(outside))


def lattice_maps(S, k):
    """24 (perm, sign, t, flip): every rotation, with translations that push part (or all) of the volume out and a flip code each."""
    moves = [(0, 0, 0), (2, 0, 0), (0, -3, 1), (-1, 2, -3), (S - 1, 0, 0), (0, 1 - S, 1), (S, 0, 0)]
    return [(perm, sign, moves[(b + k) % len(moves)], (3 * b + k) % 8) for b, (perm, sign) in enumerate(affine_ref.rotations())]


def tie_maps():
    """Translations by exactly +-1/2 voxel on one axis, plain and with every flip folded in: (perm, sign, t, flip)."""
    out = []
    for flip in (0, 7):
        for a in range(3):
            for h in (0.5, -0.5):
                t = [0.0, 0.0, 0.0]
                t[a] = h
                out.append(((0, 1, 2), (1, 1, 1), tuple(t), flip))
    return out


def tie_index(vol, t, flip, outside):
    """What the tie rule asks of tie_maps: on the moved axis q = i' + 1/2 takes i' + 1 (outside at i' = S - 1, q = S - 1/2), and
    q = i' - 1/2 takes i' (q = -1/2 is voxel 0)."""
    step = tuple(1 if x > 0 else 0 for x in t)
    return lattice_index(vol, (0, 1, 2), (1, 1, 1), step, flip, outside)


def general_mats(B, S, seed, flip):
    """Rotations of 10 .. 30 degrees about every axis (either sense), anisotropic zoom 0.8 .. 1.25, translations up to S / 6."""
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(B, 12, generator=g, dtype=torch.float64)
    angles = (10.0 + 20.0 * u[:, :3]) * torch.where(u[:, 9:12] < 0.5, -1.0, 1.0)
    scale = 0.8 + 0.45 * u[:, 3:6]
    return affine_matrices(angles, scale, (u[:, 6:9] * 2 - 1) * S / 6, torch.as_tensor(flip))


def _case(name, kind, S, slots, mat, fire, flip, outside, **more):
    u8 = lambda v: None if v is None else np.asarray(v, dtype=np.uint8)
    return dict(name=name, kind=kind, S=S, pool=volumes(N_SLOTS, S), slots=list(slots), mat=mat, fire=u8(fire), flip=u8(flip), outside=outside, **more)


GARBAGE = [3.0, -1e4, 0.5, 7.0, 1e20, 2.0, -3.0, 1.5, 0.25, 9.0, -1e-30, 123.0]  # never read where fire is 0


def plain_cases():
    slots, flip = [0, 1, 2, 0, 1, 2, 0, 1, -1, 1, 1], [0, 1, 2, 3, 4, 5, 6, 7, 5, 7, 7]  # all 8 codes, the placeholder, repeated slots
    for S in (8, 20):
        yield _case(f"plain S{S} mat NULL", "exact", S, slots, None, None, flip, 9)
        yield _case(f"plain S{S} flip NULL", "exact", S, slots, None, None, None, 9)
        yield _case(f"plain S{S} fire 0", "exact", S, slots, torch.tensor([GARBAGE] * len(slots)), [0] * len(slots), flip, 9)


def lattice_cases():
    for S, k, outside in ((8, 0, 0), (8, 1, 255), (12, 2, 7)):
        maps = lattice_maps(S, k)
        mat = torch.stack([folded_lattice_mat(*m) for m in maps])
        slots = [b % N_SLOTS for b in range(len(maps))]
        # flip holds the folded codes: a kernel that looked at it where a sample fires would flip twice
        yield _case(f"lattice S{S} outside {outside}", "exact", S, slots, mat, None, [m[3] for m in maps], outside, maps=maps)


def tie_cases():
    maps = tie_maps()
    for outside in (0, 255):
        mat = torch.stack([folded_lattice_mat(*m) for m in maps])
        yield _case(f"ties outside {outside}", "exact", 8, [b % N_SLOTS for b in range(len(maps))], mat, [1] * len(maps), [m[3] for m in maps], outside,
                    maps=maps)


def general_cases():
    yield _case("general S16", "general", 16, [2, 0, 1, 1], general_mats(4, 16, 11, [6, 3, 5, 0]), [1, 0, 1, 1], [6, 3, 5, 0], 0)
    yield _case("general S20", "general", 20, [2, 0, -1, 1], general_mats(4, 20, 12, [1, 7, 2, 4]), [1, 1, 1, 0], [1, 7, 2, 4], 255)
    yield _case("general S16 fire NULL", "general", 16, [1, 1, 0, 2], general_mats(4, 16, 13, [0, 0, 5, 3]), None, [0, 0, 5, 3], 7)


def multi_trip_case():
    """B = 64, S = 44: a sample has 44 * 44 * 11 = 21296 threads' work and gets min(ceil(21296 / 256), ceil(4096 / 64)) = 64 blocks =
    16384 threads, so 4912 threads take a second trip of the grid-stride loop and the others do not (a partial last trip).  With
    B = 64 it is the smallest S for that: S = 40 has 16000 <= 16384 threads' work, one trip."""
    B, S = 64, 44
    flip = [(5 * b) % 8 for b in range(B)]
    fire = [0 if b % 3 == 0 else 1 for b in range(B)]
    slots = [-1 if b == 17 else b % N_SLOTS for b in range(B)]
    return _case("two trips B64 S44", "general", S, slots, general_mats(B, S, 14, flip), fire, flip, 255)


def small_cases():
    """Every case but the multi-trip one (which is large; the GPU file runs it, the CPU file holds its tie share to the cap)."""
    return list(plain_cases()) + list(lattice_cases()) + list(tie_cases()) + list(general_cases())
