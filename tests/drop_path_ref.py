"""Yardstick of stochastic depth (drop path) on the HIP ViT path: the per-sample decision restated in numpy and a mask object that
plugs into the restatements of tests/dropout_ref.py unchanged.  Nothing here calls the code under test.

Definition (DESIGN.md "Dropout", include/headct_hip.h "Stochastic depth").
    rates      block j of `depth` blocks at rate r (its fp32 value): q_j = r * j / (depth - 1), evaluated in double, cast to fp32;
               q_0 = 0, a one-block model has q = [0].  Both residual branches of block j use q_j.
    decision   sample b (index along the batch axis) at a branch: word b & 3 of Philox4x32-10(counter (b >> 2, 0, 1, site), key = the
               forward's 64-bit seed (low word, high word)); kept iff word >= floor(q * 2^32).  The multiplier s_b is 1 / (1 - q) in fp32
               when kept, 0 otherwise; at q = 0 it is exactly 1.0.
    sites      the branch's streaming site: 1 + 4 j + 1 (attention branch = proj_drop), 1 + 4 j + 3 (MLP branch = drop2).  The third
               counter word is 1 where the element masks have 0.
    block      h_mid = h_in + (proj(o) o Z_proj) * s^attn_b;  h_out = h_mid + (linear2(g) o Z_drop2) * s^mlp_b
"""
import numpy as np
import torch

from tests import dropout_ref as R

MASK32 = 0xFFFFFFFF
ATTN_BRANCH, MLP_BRANCH = 0, 1


def drop_path_rates(rate, depth: int):
    """fp32 values q_j as Python floats."""
    r = float(np.float32(rate))
    if depth == 1:
        return [0.0]
    return [float(np.float32(r * j / (depth - 1))) for j in range(depth)]


def path_site(block: int, branch: int) -> int:
    return 1 + 4 * block + (R.PROJ if branch == ATTN_BRANCH else R.DROP2)


def path_words(seed: int, site: int, B: int) -> np.ndarray:
    g = np.arange((B + 3) // 4, dtype=np.uint64)
    w = R.philox4x32_10(g, 0, 1, site, seed & MASK32, (seed >> 32) & MASK32)
    return np.stack(w, axis=1).reshape(-1)[:B]


def path_keep(seed: int, site: int, q, B: int) -> np.ndarray:
    """bool [B]: the samples a branch keeps.  At q = 0 everything, without a draw."""
    if float(np.float32(q)) == 0.0:
        return np.ones(B, dtype=bool)
    return path_words(seed, site, B) >= R.threshold(q)


def path_scales(seed: int, site: int, q, B: int) -> np.ndarray:
    """fp32 [B]: the multipliers s_b."""
    return path_keep(seed, site, q, B).astype(np.float32) * np.float32(R.scale(q))


def keep_tables(seed: int, rate, depth: int, B: int):
    """[depth][2][B] keep decisions as 0 / 1 lists: per block the attention branch's, then the MLP branch's."""
    q = drop_path_rates(rate, depth)
    return [[path_keep(seed, path_site(j, br), q[j], B).astype(int).tolist() for br in (ATTN_BRANCH, MLP_BRANCH)] for j in range(depth)]


class PathMasks:
    """The interface of dropout_ref.Masks with drop path folded into the proj_drop and drop2 sites: there `.stream` returns Z * s_b, s_b
    broadcast as [B, 1, 1]; everywhere else it is dropout_ref.Masks at p > 0 and dropout_ref.Ones at p = 0."""

    def __init__(self, seed: int, p, rate, depth: int, B: int, dtype=torch.float32):
        self.seed, self.p, self.B, self.dtype = int(seed), p, B, dtype
        self.q = drop_path_rates(rate, depth)
        self.elems = R.Masks(seed, p, dtype) if p > 0 else R.Ones()

    def stream(self, site: int, shape) -> torch.Tensor:
        z = self.elems.stream(site, shape)
        j, kind = (site - 1) // 4, (site - 1) % 4
        if site < 1 or kind not in (R.PROJ, R.DROP2) or j >= len(self.q) or self.q[j] == 0.0:
            return z
        assert shape[0] == self.B
        s = torch.from_numpy(path_scales(self.seed, site, self.q[j], self.B)).to(self.dtype).view(self.B, *([1] * (len(shape) - 1)))
        return z * s  # (fp32: one combined multiplier per element, c = fl(z * s_b))

    def attn(self, site: int, B: int, H: int, N: int) -> torch.Tensor:
        return self.elems.attn(site, B, H, N)


# the model case of the GPU tests: dropout_ref.VIT_CASE with three blocks and four samples, so q = [0, .25, .5] at rate 0.5
PATH_CASE = dict(R.VIT_CASE, num_layers=3, batch=4)
PATH_RATE = 0.5
# Pinned seeds (tests/test_drop_path_cpu.py holds both to the definition above):
#   SEED_MIXED, B = 4, rate 0.5: every branch with q > 0 has kept and dropped samples
#   SEED_ONE, B = 1: keeps everything except the MLP branch of block 2
SEED_MIXED = 20140
KEEP_MIXED = [[[1, 1, 1, 1], [1, 1, 1, 1]], [[1, 0, 1, 1], [1, 1, 0, 1]], [[0, 1, 0, 1], [0, 1, 1, 0]]]
SEED_ONE = 1
KEEP_ONE = [[[1], [1]], [[1], [1]], [[1], [0]]]


def path_case_input(case=PATH_CASE):
    return R.vit_case_input(case)
