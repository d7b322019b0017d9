"""Volume-to-volume retrieval with a trained encoder (the reference's README: feature extraction, retrieval mAP on RSNA / CQ500):
pooled features, a normalised feature bank searched by the fused similarity + top-k kernel (`hct_topk_dot`, which never forms the
[Q, G] score matrix), retrieval metrics and DINO's weighted k-NN.  The search runs on the GPU only (no CPU fallback exists);
pooling, metrics and k-NN are plain torch.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _lib

POOLINGS = ("cls", "mean", "cls_mean")


def pool_tokens(tokens: torch.Tensor, num_register_tokens: int = 0, pooling: str = "cls") -> torch.Tensor:
    """One feature vector per volume from the encoder's tokens [B, T, D] (token 0 the class token, then `num_register_tokens`
    register tokens, then the patch tokens): 'cls' = token 0, 'mean' = mean over the PATCH tokens only, 'cls_mean' = their
    concatenation [B, 2 D].  What VIT.POOLING / --pooling selects."""
    if tokens.dim() != 3:
        raise ValueError(f"tokens must be [B, T, D], got {tuple(tokens.shape)}")
    first = 1 + num_register_tokens
    if pooling == "cls":
        return tokens[:, 0]
    if pooling not in POOLINGS:
        raise ValueError(f"Pooling {pooling} not supported (one of {POOLINGS})")
    if tokens.shape[1] <= first:
        raise ValueError(f"no patch tokens: T = {tokens.shape[1]} with {num_register_tokens} register tokens")
    mean = tokens[:, first:].mean(dim=1)
    return mean if pooling == "mean" else torch.cat([tokens[:, 0], mean], dim=1)


@torch.no_grad()
def extract_features(model, loader, pooling: str = "cls") -> Tuple[torch.Tensor, torch.Tensor, List[str]]:
    """(feats [n, D'] fp32 on the device, labels [n] int64 on the device, names) of every scan of a labelled loader (batches
    `(volume, target, names)`: SyntheticLabelled, or LabelledVolumes through get_finetune_dataloaders); `model(volume)` returns
    `(tokens [B, T, D], hidden states)`."""
    dev = next(model.parameters()).device
    regs = int(getattr(model, "num_register_tokens", 0))
    feats, labels, names = [], [], []
    for data, target, fname in loader:
        tokens, _ = model(data.to(dev))
        feats.append(pool_tokens(tokens.float(), regs, pooling).clone())
        labels.append(target.to(dev).to(torch.int64).view(-1))
        names += [str(f) for f in fname]
    if not feats:
        raise ValueError("extract_features: the loader is empty")
    return torch.cat(feats), torch.cat(labels), names


def topk_dot(q: torch.Tensor, g: torch.Tensor, k: int, exclude: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """`hct_topk_dot` on two matrices of unit rows (fp32 or bf16, same dtype): (scores [Q, k] fp32, idx [Q, k] int32)."""
    if not (q.is_cuda and g.is_cuda):
        raise _lib.HctError("topk_dot runs on the GPU (no CPU fallback exists)")
    if q.dim() != 2 or g.dim() != 2 or q.shape[1] != g.shape[1] or q.dtype != g.dtype or q.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"q {tuple(q.shape)} {q.dtype} and g {tuple(g.shape)} {g.dtype} must be [Q, D] and [G, D] of one dtype (fp32 or bf16)")
    lib = _lib.load()
    q, g = q.contiguous(), g.contiguous()
    Q, D = q.shape
    G = g.shape[0]
    if exclude is not None:
        exclude = exclude.to(device=q.device, dtype=torch.int32).contiguous()
        if exclude.shape != (Q,):
            raise ValueError(f"exclude must be [Q] = [{Q}], got {tuple(exclude.shape)}")
    with torch.cuda.device(q.device):
        scores = torch.empty(Q, max(k, 0), dtype=torch.float32, device=q.device)
        idx = torch.empty(Q, max(k, 0), dtype=torch.int32, device=q.device)
        ws = torch.empty(max(16, lib.hct_topk_dot_workspace(Q, G, k)), dtype=torch.uint8, device=q.device)
        _lib.check(lib.hct_topk_dot(q.data_ptr(), Q, g.data_ptr(), G, D, _lib.dtype_code(q), _lib.ptr(exclude), k, scores.data_ptr(),
                                    idx.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr()), "hct_topk_dot")
    return scores, idx


def attention_row_probs(qkv: torch.Tensor, B: int, N: int, H: int, dh: int, rows: Sequence[int]) -> torch.Tensor:
    """`hct_attention_row_probs`: probs [B, H, len(rows), N] fp32 of the query rows `rows` (host integers, validated here) from the
    qkv [B, N, 3, H, dh] buffer (fp32 or bf16) that hct_attention_fwd takes."""
    rows = [int(r) for r in rows]
    if not rows or any(r < 0 or r >= N for r in rows):
        raise _lib.HctError(f"attention rows {rows} outside [0, {N})")
    if not qkv.is_cuda:
        raise _lib.HctError("attention_row_probs runs on the GPU (no CPU fallback exists)")
    if qkv.numel() != B * N * 3 * H * dh or not qkv.is_contiguous():
        raise ValueError(f"qkv must be a contiguous [B, N, 3, H, dh] buffer ({qkv.numel()} elements for {(B, N, 3, H, dh)})")
    with torch.cuda.device(qkv.device):
        r = torch.tensor(rows, dtype=torch.int32, device=qkv.device)
        probs = torch.empty(B, H, len(rows), N, dtype=torch.float32, device=qkv.device)
        _lib.check(_lib.load().hct_attention_row_probs(qkv.data_ptr(), B, N, H, dh, _lib.dtype_code(qkv), r.data_ptr(), len(rows),
                                                       probs.data_ptr(), _lib.stream_ptr()), "hct_attention_row_probs")
    return probs


class FeatureBank:
    """A gallery of feature vectors, L2-normalised once (`hct_l2norm_rows_fwd`) into `dtype` ('bf16': half the memory and the MFMA
    search kernel when D % 32 == 0; 'fp32': the plain kernel).  `search(queries, k)` normalises the raw queries the same way and
    returns the k most similar gallery rows per query by cosine, best first, equal scores by ascending row."""

    def __init__(self, feats: torch.Tensor, labels: Optional[torch.Tensor] = None, names: Optional[Sequence[str]] = None, dtype: str = "bf16"):
        if dtype not in ("bf16", "fp32"):
            raise ValueError(f"FeatureBank dtype {dtype} not supported ('bf16' or 'fp32')")
        if feats.dim() != 2 or feats.shape[1] % 4:
            raise ValueError(f"feats must be [n, D] with D a multiple of 4, got {tuple(feats.shape)}")
        if not feats.is_cuda:
            raise _lib.HctError("FeatureBank lives on the GPU (no CPU fallback exists)")
        self.dtype = torch.bfloat16 if dtype == "bf16" else torch.float32
        self.labels = None if labels is None else labels.to(feats.device).to(torch.int64)
        self.names = None if names is None else list(names)
        self.feats = self._normalise(feats)

    def __len__(self) -> int:
        return self.feats.shape[0]

    def _normalise(self, x: torch.Tensor) -> torch.Tensor:
        x = x.detach().to(torch.float32).contiguous()
        M, n = x.shape
        with torch.cuda.device(x.device):
            out = torch.empty(M, n, dtype=self.dtype, device=x.device)
            inv = torch.empty(M, dtype=torch.float32, device=x.device)
            _lib.check(_lib.load().hct_l2norm_rows_fwd(x.data_ptr(), M, n, out.data_ptr(), _lib.dtype_code(self.dtype), inv.data_ptr(),
                                                       _lib.stream_ptr()), "hct_l2norm_rows_fwd")
        return out

    def search(self, queries: Optional[torch.Tensor], k: int, exclude=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """(scores [Q, k] fp32, idx [Q, k] int32).  `exclude`: None, a [Q] tensor with one gallery row to skip per query (-1 = none),
        or 'self' = leave-one-out search of the bank against itself (`queries` is then None, or the bank's own raw features)."""
        if isinstance(exclude, str):
            if exclude != "self":
                raise ValueError(f"exclude {exclude!r} not supported")
            if queries is not None and queries.shape[0] != len(self):
                raise ValueError("exclude='self' searches the bank against itself")
            return topk_dot(self.feats, self.feats, k, torch.arange(len(self), dtype=torch.int32, device=self.feats.device))
        if queries is None:
            raise ValueError("search needs queries unless exclude='self'")
        if queries.dim() != 2 or queries.shape[1] != self.feats.shape[1]:
            raise ValueError(f"queries must be [Q, {self.feats.shape[1]}], got {tuple(queries.shape)}")
        return topk_dot(self._normalise(queries.to(self.feats.device)), self.feats, k, exclude)


def retrieval_metrics(idx, query_labels, gallery_labels, ks: Sequence[int]) -> Dict[str, float]:
    """{'P@k': ..., 'mAP@k': ...} for every k of `ks`, from the neighbour table idx [Q, >= max(ks)] of a search.

    Single-label relevance: gallery item idx[q, i] is relevant (rel_i = 1) when its label equals the query's; an empty slot
    (idx = -1) is a miss.  With P@i = (hits among the first i) / i:
        P@k   = mean over queries of (hits in the top k) / k
        AP@k  = (sum_{i <= k} P@i * rel_i) / max(1, sum_{i <= k} rel_i)
        mAP@k = mean over queries of AP@k
    (The reference reports retrieval mAP as a plot and ships no code for it: this definition is this project's.)"""
    idx = torch.as_tensor(idx).detach().cpu().to(torch.int64)
    ql = torch.as_tensor(query_labels).detach().cpu().to(torch.int64).view(-1)
    gl = torch.as_tensor(gallery_labels).detach().cpu().to(torch.int64).view(-1)
    if idx.dim() != 2 or idx.shape[0] != ql.shape[0]:
        raise ValueError(f"idx {tuple(idx.shape)} does not match {ql.shape[0]} query labels")
    if max(ks) > idx.shape[1] or min(ks) < 1:
        raise ValueError(f"ks {list(ks)} outside [1, {idx.shape[1]}]")
    valid = idx >= 0
    rel = ((gl[idx.clamp(min=0)] == ql.view(-1, 1)) & valid).to(torch.float64)  # [Q, K]
    hits = rel.cumsum(dim=1)
    prec = hits / torch.arange(1, idx.shape[1] + 1, dtype=torch.float64).view(1, -1)
    out = {}
    for k in ks:
        out[f"P@{k}"] = float(prec[:, k - 1].mean())
        ap = (prec[:, :k] * rel[:, :k]).sum(dim=1) / hits[:, k - 1].clamp(min=1.0)
        out[f"mAP@{k}"] = float(ap.mean())
    return out


def knn_predict(scores: torch.Tensor, idx: torch.Tensor, gallery_labels: torch.Tensor, num_classes: int, T: float = 0.07) -> torch.Tensor:
    """DINO's weighted k-NN: neighbour i of a query votes exp(score_i / T) for its class; the votes are normalised to class
    probabilities [Q, num_classes] (fp32; feeds metrics.multiclass_auroc / multiclass_accuracy).  Empty slots (idx = -1) do not
    vote; a query without any neighbour gets the uniform distribution."""
    idx = idx.to(torch.int64)
    valid = idx >= 0
    lab = gallery_labels.to(idx.device).to(torch.int64)[idx.clamp(min=0)]
    s = scores.to(torch.float32)
    # exp((s - max) / T): the common factor cancels in the normalisation and keeps the exponentials finite
    top = torch.where(valid, s, torch.full_like(s, float("-inf"))).max(dim=1, keepdim=True).values
    top = torch.where(torch.isfinite(top), top, torch.zeros_like(top))
    w = torch.where(valid, torch.exp((s - top) / T), torch.zeros_like(s))
    votes = torch.zeros(idx.shape[0], num_classes, dtype=torch.float32, device=idx.device)
    votes.scatter_add_(1, lab, w)
    total = votes.sum(dim=1, keepdim=True)
    return torch.where(total > 0, votes / total.clamp(min=1e-30), torch.full_like(votes, 1.0 / num_classes))
