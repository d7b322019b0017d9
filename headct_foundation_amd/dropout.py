"""Dropout of the HIP models: the site numbering of the native plan and the keep masks as tensors.

Masks are never stored.  The plan draws them from `(seed, site, element)` with Philox4x32-10 wherever a kernel needs them
(csrc/philox.h; DESIGN.md "Dropout"); `keep_mask` materialises one over `hct_dropout_mask`, for tests and debugging.
"""
from __future__ import annotations

from typing import Sequence

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
