"""What the multi-label loss tests share: the case list of tests/test_multilabel_gpu.py with the loop constants of
csrc/multilabel.hip it was derived from, the inputs, and the float64 reference -- torch's own
binary_cross_entropy_with_logits with the valid mask as its weight, and its autograd gradient.  Nothing here needs a GPU."""
import functools

import torch
import torch.nn.functional as F

# csrc/multilabel.hip
THREADS = 256          # kBceThreads: threads per block; the gradient pass takes one element per thread and trip
ROW_TRIPS = 4          # kBceRowTrips: rows per thread before a column is shared out over another row block
MAX_ROW_BLOCKS = 64    # kBceMaxRowBlocks: partial (sum, count) pairs per column
GRAD_BLOCKS = 256      # kBceGradBlocks: blocks of the gradient pass, grid-stride beyond THREADS * GRAD_BLOCKS elements
HEAD_BYTES = 16        # kBceHead: the workspace's head (the valid-entry count)

FP32_BAR = 1e-5        # the project's fp32 bar for composite kernels (tests/test_head_kernels_gpu.py)
DLOSS = 0.37


def shape(B: int, T: int) -> dict:
    """bce_shape of csrc/multilabel.hip: cx columns x ry rows of threads per block, column blocks, rows per row block, row blocks."""
    cx = 1
    while cx < T and cx < THREADS:
        cx *= 2
    ry = THREADS // cx
    want = min(MAX_ROW_BLOCKS, -(-B // (ry * ROW_TRIPS)))
    chunk = -(-B // want)
    return {"cx": cx, "ry": ry, "col_blocks": -(-T // cx), "chunk": chunk, "row_blocks": -(-B // chunk)}


def workspace_bytes(B: int, T: int) -> int:
    return HEAD_BYTES + shape(B, T)["row_blocks"] * T * 8


# the issue's grid ...
CASES = [(B, T) for B in (1, 3, 64, 257, 1025) for T in (1, 6, 14, 33)]
# ... and what the kernel's own limits add:
CASES += [(3, 257),     # T > THREADS: a second column block, ending raggedly; the finalize block's second trip over the columns
          (2, 256),     # T == THREADS: cx at its limit, one row of threads (ry = 1)
          (1024, 1),    # T = 1: ry = THREADS rows of threads, exactly ROW_TRIPS trips, one row block
          (2049, 33)]   # B * T > THREADS * GRAD_BLOCKS: the gradient pass's second trip, ending raggedly; MAX_ROW_BLOCKS reached
EXTRA_SHAPE = (64, 14)  # the fine-tuning batch: the degenerate and the NULL-output cases


@functools.lru_cache(maxsize=None)
def inputs(B: int, T: int):
    """(logits, target, pos_weight) fp32 on the CPU: logits 4 * randn with every 7th flat element +100, every 11th (offset 3) -100,
    every 13th (offset 5) 0; targets 0 / 1 with every 5th flat element (offset 2) missing; pos_weight uniform in [0.05, 20]."""
    g = torch.Generator().manual_seed(1000 * B + T)
    x = (4 * torch.randn(B * T, generator=g)).float()
    i = torch.arange(B * T)
    x[i % 7 == 0] = 100.0
    x[i % 11 == 3] = -100.0
    x[i % 13 == 5] = 0.0
    y = (torch.rand(B * T, generator=g) < 0.5).float()
    y[i % 5 == 2] = -1.0
    w = (0.05 + 19.95 * torch.rand(T, generator=g)).float()
    return x.view(B, T), y.view(B, T), w


def reference(x, y, w=None, g=1.0):
    """float64: (loss, label_loss [T], dlogits [B, T], n) of F.binary_cross_entropy_with_logits(x, y.clamp(min=0), weight=valid,
    pos_weight=w, reduction='sum') / max(n, 1) and its autograd gradient times g; label_loss[t] the same over column t alone."""
    x = x.double().clone().requires_grad_(True)
    y = y.double()
    valid = (y >= 0).double()
    n = int(valid.sum())
    pw = None if w is None else w.double()
    terms = F.binary_cross_entropy_with_logits(x, y.clamp(min=0), weight=valid, pos_weight=pw, reduction="none")
    loss = F.binary_cross_entropy_with_logits(x, y.clamp(min=0), weight=valid, pos_weight=pw, reduction="sum") / max(n, 1)
    (grad,) = torch.autograd.grad(loss, x)
    label_loss = terms.sum(dim=0) / valid.sum(dim=0).clamp(min=1)
    return loss.detach(), label_loss.detach(), grad * g, n
