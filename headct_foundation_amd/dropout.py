"""Dropout of the HIP models: the site numbering of the native plan and the keep masks as tensors.

Masks are never stored.  The plan draws them from `(seed, site, element)` with Philox4x32-10 wherever a kernel needs them
(csrc/philox.h; DESIGN.md "Dropout"); `keep_mask` materialises one over `hct_dropout_mask`, for tests and debugging.

Stochastic depth (drop path, an addition of this build) draws one decision per (sample, residual branch) from the same seed:
`drop_path_rates` gives the per-block rates, `path_site` the branch's site and `path_scales` the table of per-sample multipliers
over `hct_drop_path_scales`.

Patch dropout (an addition of this build) drops whole patch tokens of the ViT backbone in training mode: `patch_keep_count` is the
number a forward keeps; which ones is decided by ranking noise, as in the MAE (dino_model.ViTBackbone).
"""
from __future__ import annotations

import ctypes as C
from typing import List, Sequence

import numpy as np
import torch

from . import _lib

SITE_EMBEDDING = 0  # dropout(conv(x) + pos) on the patch tokens (patch_embedding.py:160)
ATTN, PROJ, DROP1, DROP2 = 0, 1, 2, 3  # kinds of a block's four sites: attention probabilities, proj_drop, MLP drop1 / drop2


def block_site(block: int, kind: int) -> int:
    """Site of `kind` in block `block`, counting the encoder's blocks first and the MAE decoder's behind them."""
    if block < 0 or kind not in (ATTN, PROJ, DROP1, DROP2):
        raise ValueError(f"no dropout site for block {block}, kind {kind}")
    return 1 + 4 * block + kind


def check_rate(p: float) -> float:
    if not (0 <= p < 1):
        raise ValueError(f"dropout rate {p}: the HIP path takes 0 <= p < 1 (p = 1 drops every value and has no finite scale 1 / (1 - p))")
    return float(p)


def check_path_rate(r: float) -> float:
    if not (0 <= r < 1):
        raise ValueError(f"drop_path_rate {r}: the HIP path takes 0 <= drop_path_rate < 1 (drop_path_rate = 1 drops every sample in the last "
                         "block and has no finite scale 1 / (1 - q))")
    return float(r)


def drop_path_rates(rate: float, depth: int) -> List[float]:
    """Per-block rates q_j = r * j / (depth - 1) of a backbone of `depth` blocks: r is the fp32 value of `rate` (what the plan's config
    carries), the quotient is evaluated in double and cast to fp32.  q_0 = 0; a one-block model has q = [0]."""
    r = float(np.float32(check_path_rate(rate)))
    if depth < 1:
        raise ValueError(f"drop_path_rates: depth {depth}")
    return [float(np.float32(r * j / (depth - 1))) if depth > 1 else 0.0 for j in range(depth)]


def check_patch_rate(r: float) -> float:
    if not (0 <= r < 1):
        raise ValueError(f"patch_dropout {r}: the HIP path takes 0 <= patch_dropout < 1 (the share of patch tokens dropped; 1 drops them all)")
    return float(r)


def patch_keep_count(L: int, rate: float) -> int:
    """Patch tokens a training forward keeps out of `L` at patch-dropout `rate`: K = int(L * (1 - rate)) in double, the rule of the
    MAE's len_keep (mae.py:205) and of the native plan (L = 10: rate 0.1 keeps 9, rate 0.7 keeps 3).  K < 1 is refused."""
    if L < 1:
        raise ValueError(f"patch_keep_count: {L} patches")
    K = int(L * (1 - check_patch_rate(rate)))
    if K < 1:
        raise ValueError(f"patch_dropout {rate} leaves none of the {L} patches: K = int(L * (1 - rate)) must be at least 1")
    return K


def path_site(block: int, branch: int) -> int:
    """Site of a block's residual branch: 0 the attention branch (the proj_drop site), 1 the MLP branch (the drop2 site)."""
    if branch not in (0, 1):
        raise ValueError(f"no residual branch {branch}: 0 attention, 1 MLP")
    return block_site(block, PROJ if branch == 0 else DROP2)


def path_scales(seed: int, sites: Sequence[int], rates: Sequence[float], B: int, device="cuda") -> torch.Tensor:
    """fp32 `[len(sites), B]`: the drop-path multiplier of sample b at each (site, rate) under `seed` -- 1 / (1 - q) where the sample
    is kept, 0 where it is dropped, exactly 1 at q = 0."""
    if len(sites) != len(rates):
        raise ValueError("path_scales: one rate per site")
    for q in rates:
        check_path_rate(q)
    n = len(sites)
    out = torch.empty(n, int(B), dtype=torch.float32, device=device)
    if not out.is_cuda:
        raise _lib.HctError("path_scales (HIP) needs a GPU device: there is no CPU fallback")
    lib = _lib.load()
    with torch.cuda.device(out.device):
        rc = lib.hct_drop_path_scales(int(seed) & 0xFFFFFFFFFFFFFFFF, (C.c_int * n)(*[int(v) for v in sites]),
                                      (C.c_float * n)(*[float(v) for v in rates]), n, int(B), out.data_ptr(), _lib.stream_ptr())
        _lib.check(rc, "hct_drop_path_scales")
    return out


def keep_mask(seed: int, site: int, shape: Sequence[int], p: float, attention: bool = False, device="cuda") -> torch.Tensor:
    """Keep mask (bool, `shape`) of `site` under `seed` at rate `p`: of a streaming tensor of that shape (element index = row-major
    index), or with `attention=True` of the attention probabilities `[B, H, N, N]`."""
    check_rate(p)
    shape = tuple(int(v) for v in shape)
    out = torch.empty(shape, dtype=torch.uint8, device=device)
    if not out.is_cuda:
        raise _lib.HctError("keep_mask (HIP) needs a GPU device: there is no CPU fallback")
    lib = _lib.load()
    with torch.cuda.device(out.device):
        st = _lib.stream_ptr()
        if attention:
            if len(shape) != 4 or shape[2] != shape[3]:
                raise ValueError(f"attention masks are [B, H, N, N], got {shape}")
            rc = lib.hct_dropout_mask(int(seed) & 0xFFFFFFFFFFFFFFFF, site, 1, 0, shape[0] * shape[1], shape[2], float(p), out.data_ptr(), st)
        else:
            rc = lib.hct_dropout_mask(int(seed) & 0xFFFFFFFFFFFFFFFF, site, 0, out.numel(), 0, 0, float(p), out.data_ptr(), st)
        _lib.check(rc, "hct_dropout_mask")
    return out.bool()
