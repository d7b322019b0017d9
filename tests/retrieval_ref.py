"""fp64 torch / numpy restatements for the retrieval and attention-map tests: cosine scores and their exact ranking, the rank-robust
check of a top-k result, brute-force retrieval metrics, weighted k-NN, token pooling, attention probabilities of a qkv buffer, and a
ViT forward that returns every block's attention probabilities (LayerNorm or RMSNorm trees)."""
import numpy as np
import torch
import torch.nn.functional as F


# ---- top-k over dot products -------------------------------------------------------------------------------------------------
def unit_rows(n, d, seed, dtype=torch.float32):
    """n random unit vectors, rounded to the storage dtype (what the kernel reads)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, d, generator=g, dtype=torch.float64)
    return (x / x.norm(dim=1, keepdim=True)).to(dtype)


def scores_ref(q, g):
    """[Q, G] fp64 dot products of the STORED values."""
    return q.detach().cpu().double() @ g.detach().cpu().double().T


def topk_ref(S, k, exclude=None):
    """Exact ranking of fp64 scores S [Q, G]: score descending, equal scores by ascending row; idx [Q, k] with -1 where the rows run out."""
    Q, G = S.shape
    out = np.full((Q, k), -1, dtype=np.int64)
    Sn = S.numpy()
    for qi in range(Q):
        rows = np.arange(G)
        if exclude is not None and int(exclude[qi]) >= 0:
            rows = rows[rows != int(exclude[qi])]
        order = rows[np.lexsort((rows, -Sn[qi, rows]))][:k]
        out[qi, :len(order)] = order
    return torch.from_numpy(out)


def check_topk(scores, idx, S, k, bar, exclude=None, order_slack=0.0):
    """The rank-robust check.  For every query: the filled slots are unique rows in range, never the excluded row; slots past the rows
    available hold -1 / -inf; scores do not increase; every score is the reference score of its (query, row) pair within `bar`; no row
    left out scores above the last returned score + 2 bar.  `order_slack` loosens the ordering of the scores (for scores that are the reference's own
    at rows another computation ranked).  Returns the largest score error."""
    scores, idx = scores.detach().cpu().double(), idx.detach().cpu().to(torch.int64)
    Q, G = S.shape
    assert scores.shape == (Q, k) and idx.shape == (Q, k)
    ex = torch.full((Q,), -1, dtype=torch.int64) if exclude is None else exclude.detach().cpu().to(torch.int64)
    avail = G - (ex >= 0).to(torch.int64)
    worst = 0.0
    for qi in range(Q):
        n = min(k, int(avail[qi]))
        got, sc = idx[qi, :n], scores[qi, :n]
        assert bool((idx[qi, n:] == -1).all()) and bool(torch.isinf(scores[qi, n:]).all()) and bool((scores[qi, n:] < 0).all()), (qi, idx[qi], scores[qi])
        assert bool(((got >= 0) & (got < G)).all()), (qi, got)
        assert len(set(got.tolist())) == n, (qi, got)
        assert int(ex[qi]) not in got.tolist() or int(ex[qi]) < 0, (qi, got, int(ex[qi]))
        assert bool((sc[1:] <= sc[:-1] + order_slack).all()), (qi, sc)
        err = float((sc - S[qi, got]).abs().max()) if n else 0.0
        assert err <= bar, (qi, err)
        worst = max(worst, err)
        rest = S[qi].clone()
        rest[got] = -np.inf
        if int(ex[qi]) >= 0:
            rest[int(ex[qi])] = -np.inf
        if n:
            assert float(rest.max()) <= float(sc[-1]) + 2 * bar, (qi, float(rest.max()), float(sc[-1]))
    return worst


# ---- metrics, k-NN, pooling ------------------------------------------------------------------------------------------------
def retrieval_metrics_brute(idx, query_labels, gallery_labels, ks):
    idx, ql, gl = np.asarray(idx), np.asarray(query_labels), np.asarray(gallery_labels)
    out = {}
    for k in ks:
        ps, aps = [], []
        for qi in range(idx.shape[0]):
            hits, acc = 0, 0.0
            for i in range(k):
                j = int(idx[qi, i])
                if j >= 0 and gl[j] == ql[qi]:
                    hits += 1
                    acc += hits / (i + 1)
            ps.append(hits / k)
            aps.append(acc / max(1, hits))
        out[f"P@{k}"], out[f"mAP@{k}"] = float(np.mean(ps)), float(np.mean(aps))
    return out


def knn_ref(scores, idx, gallery_labels, num_classes, T):
    scores, idx, gl = np.asarray(scores, dtype=np.float64), np.asarray(idx), np.asarray(gallery_labels)
    out = np.zeros((idx.shape[0], num_classes))
    for qi in range(idx.shape[0]):
        for s, j in zip(scores[qi], idx[qi]):
            if j >= 0:
                out[qi, gl[j]] += np.exp(s / T)
        out[qi] = out[qi] / out[qi].sum() if out[qi].sum() > 0 else 1.0 / num_classes
    return out


def pool_ref(tokens, regs, pooling):
    t = np.asarray(tokens, dtype=np.float64)
    cls, mean = t[:, 0], t[:, 1 + regs:].mean(axis=1)
    return {"cls": cls, "mean": mean, "cls_mean": np.concatenate([cls, mean], axis=1)}[pooling]


# ---- attention -------------------------------------------------------------------------------------------------------------
def attention_ref(qkv, B, N, H, dh):
    """(probs [B, H, N, N], lse [B, H, N], o [B, N, H dh]) in fp64 of the stored qkv [B, N, 3, H, dh]."""
    t = qkv.detach().cpu().double().view(B, N, 3, H, dh).permute(2, 0, 3, 1, 4)
    logits = (t[0] @ t[1].transpose(-1, -2)) * dh ** -0.5
    probs = torch.softmax(logits, dim=-1)
    return probs, torch.logsumexp(logits, dim=-1), (probs @ t[2]).transpose(1, 2).reshape(B, N, H * dh)


def _norm(x, w, b, eps_ln):
    if b is None:  # RMSNorm: eps 1e-6 wherever the model builds one
        return x * torch.rsqrt((x * x).mean(dim=-1, keepdim=True) + 1e-6) * w
    return F.layer_norm(x, (x.shape[-1],), w, b, eps_ln)


def vit_attention(p, x, patch_size, heads, layers, dtype=torch.float64):
    """ViT forward (conv patch embedding + position table, class token, register tokens, blocks, final norm) in `dtype` on the CPU.
    Returns (tokens [B, T, D], [per block: attention probabilities [B, H, T, T]])."""
    p = {k: v.detach().cpu().to(dtype) for k, v in p.items()}
    x = x.detach().cpu().to(dtype)
    B = x.shape[0]
    tok = F.conv3d(x, p["patch_embedding.patch_embeddings.weight"], p["patch_embedding.patch_embeddings.bias"], stride=patch_size)
    tok = tok.flatten(2).transpose(-1, -2)
    if "patch_embedding.position_embeddings" in p:
        tok = tok + p["patch_embedding.position_embeddings"]
    h = torch.cat((p["cls_token"].expand(B, -1, -1), tok), dim=1)
    if "register_tokens" in p:
        h = torch.cat((h[:, :1], p["register_tokens"].expand(B, -1, -1), h[:, 1:]), dim=1)
    D = h.shape[-1]
    atts = []
    for i in range(layers):
        pre = f"blocks.{i}"
        x1 = _norm(h, p[f"{pre}.att_norm.weight"], p.get(f"{pre}.att_norm.bias"), 1e-5)
        qkv = F.linear(x1, p[f"{pre}.attn.qkv.weight"], p.get(f"{pre}.attn.qkv.bias"))
        qkv = qkv.reshape(B, -1, 3, heads, D // heads).permute(2, 0, 3, 1, 4)
        att = torch.softmax((qkv[0] @ qkv[1].transpose(-1, -2)) * (D // heads) ** -0.5, dim=-1)
        atts.append(att)
        y = (att @ qkv[2]).transpose(1, 2).reshape(B, -1, D)
        h = h + F.linear(y, p[f"{pre}.attn.proj.weight"], p[f"{pre}.attn.proj.bias"])
        x2 = _norm(h, p[f"{pre}.ffn_norm.weight"], p.get(f"{pre}.ffn_norm.bias"), 1e-5)
        u = F.gelu(F.linear(x2, p[f"{pre}.mlp.linear1.weight"], p[f"{pre}.mlp.linear1.bias"]))
        h = h + F.linear(u, p[f"{pre}.mlp.linear2.weight"], p[f"{pre}.mlp.linear2.bias"])
    return _norm(h, p["norm.weight"], p.get("norm.bias"), 1e-6), atts
