"""Retrieval and attention maps on the GPU: hct_topk_dot and hct_attention_row_probs through the C ABI against fp64 restatements,
the ViT's attention methods, FeatureBank end to end, and a plumbing run of main_retrieval.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import mae_oracle as O
from tests import retrieval_ref as RR
from tests.lora_ref import CASE
from tests.util import rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}
BAR = 1e-4  # fp32 accumulation of D <= 1024 products with sum |q_i g_i| <= 1: at most D * 2^-24 ~ 6e-5


def _st():
    return torch.cuda.current_stream().cuda_stream


def _topk(lib, q, g, k, exclude=None, Q=None, G=None):
    """hct_topk_dot through the C ABI on the first Q / G rows; (rc, scores, idx)."""
    from headct_foundation_amd import _lib
    Q = q.shape[0] if Q is None else Q
    G = g.shape[0] if G is None else G
    scores = torch.full((Q, max(k, 1)), 7.0, dtype=torch.float32, device=q.device)
    idx = torch.full((Q, max(k, 1)), -7, dtype=torch.int32, device=q.device)
    ws = torch.empty(max(16, lib.hct_topk_dot_workspace(Q, G, k)), dtype=torch.uint8, device=q.device)
    rc = lib.hct_topk_dot(q.data_ptr(), Q, g.data_ptr(), G, q.shape[1], _lib.dtype_code(q), None if exclude is None else exclude.data_ptr(), k,
                          scores.data_ptr(), idx.data_ptr(), ws.data_ptr(), ws.numel(), _st())
    torch.cuda.synchronize()
    return rc, scores[:, :k], idx[:, :k]


_DATA = {}


def _data(dtype, D):
    """(q [70, D], g [5000, D], fp64 scores [70, 5000]) of stored unit vectors: made once, shared, never modified."""
    key = (dtype, D)
    if key not in _DATA:
        q, g = RR.unit_rows(70, D, 11 + D, DTYPES[dtype]), RR.unit_rows(5000, D, 23 + D, DTYPES[dtype])
        _DATA[key] = (q, g, RR.scores_ref(q, g))
    return _DATA[key]


# ---- hct_topk_dot ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("D", [48, 64, 768])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_topk_dot_rank_robust(lib, cuda, dtype, D):
    """Q in {1, 17, 70} x G in {1, 15, 1000, 5000} x k in {1, 10, 64}, with and without excluded rows (D = 64 / 768 in bf16: the MFMA
    kernel; everything else the plain one).  G = 5000 runs five gallery chunks and the merge."""
    q, g, S = _data(dtype, D)
    qd, gd = q.to(cuda), g.to(cuda)
    assert lib.hct_topk_dot_chunks(70, 5000) == 5 and lib.hct_topk_dot_chunks(1, 5000) == 5 and lib.hct_topk_dot_chunks(70, 1000) == 1
    worst = 0.0
    for Q in (1, 17, 70):
        for G in (1, 15, 1000, 5000):
            ex = torch.tensor([(7 * i) % G if i % 2 == 0 else -1 for i in range(Q)], dtype=torch.int32)
            for k in (1, 10, 64):
                assert lib.hct_topk_dot_workspace(Q, G, k) == Q * lib.hct_topk_dot_chunks(Q, G) * k * 8
                for exclude in (None, ex):
                    rc, scores, idx = _topk(lib, qd, gd, k, None if exclude is None else exclude.to(cuda), Q, G)
                    assert rc == 0, lib.hct_last_error_string()
                    worst = max(worst, RR.check_topk(scores, idx, S[:Q, :G], k, BAR, exclude))
    print(f"hct_topk_dot {dtype} D={D}: largest score error {worst:.2e} (bar {BAR:.0e})")


@pytest.mark.gpu
@pytest.mark.parametrize("D", [48, 64])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_topk_dot_exact_order(lib, cuda, dtype, D):
    """Queries e0 against rows (cos t_j, sin t_j, 0, ...) in shuffled order: the score of a row is its stored cosine exactly, adjacent
    cosines are at least 1e-2 apart, so the indices must equal the reference's."""
    G, Q, k = 120, 5, 64
    c = torch.linspace(0.99, -0.99, G, dtype=torch.float64)
    perm = torch.randperm(G, generator=torch.Generator().manual_seed(3))
    g = torch.zeros(G, D, dtype=torch.float64)
    g[perm, 0], g[perm, 1] = c, torch.sqrt(1 - c * c)
    g = g.to(DTYPES[dtype])
    q = torch.zeros(Q, D, dtype=DTYPES[dtype])
    q[:, 0] = 1.0
    stored = g[:, 0].double().sort(descending=True).values
    assert float((stored[:-1] - stored[1:]).min()) >= 1e-2
    S = RR.scores_ref(q, g)
    rc, scores, idx = _topk(lib, q.to(cuda), g.to(cuda), k)
    assert rc == 0, lib.hct_last_error_string()
    want = RR.topk_ref(S, k)
    assert torch.equal(idx.cpu().to(torch.int64), want)
    assert torch.equal(scores.cpu().double(), torch.gather(S, 1, want))  # e0 . row = the stored cosine, no rounding anywhere


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_topk_dot_ties_and_determinism(lib, cuda, dtype):
    """Rows {3, 400, 4999} are bitwise copies of every query's best match: they come first, in that order, with bit-equal scores (they
    sit in different tiles, lanes and chunks).  A second call is bit-identical."""
    D, G, Q, k = 64, 5000, 17, 10
    _, g, _ = _data(dtype, D)
    g = g.clone()
    v = RR.unit_rows(1, D, 99, torch.float64)[0]
    noise = RR.unit_rows(Q, D, 98, torch.float64)
    q = v.view(1, -1) + 0.3 * noise
    q = (q / q.norm(dim=1, keepdim=True)).to(DTYPES[dtype])
    g[[3, 400, 4999]] = v.to(DTYPES[dtype])
    S = RR.scores_ref(q, g)
    others = S.clone()
    others[:, [3, 400, 4999]] = -1.0
    assert float((S[:, 3] - others.max(dim=1).values).min()) > 0.1  # the copies are every query's best match by a wide margin
    rc, scores, idx = _topk(lib, q.to(cuda), g.to(cuda), k)
    assert rc == 0, lib.hct_last_error_string()
    assert idx[:, :3].cpu().tolist() == [[3, 400, 4999]] * Q
    assert torch.equal(scores[:, 0], scores[:, 1]) and torch.equal(scores[:, 1], scores[:, 2])
    RR.check_topk(scores, idx, S, k, BAR)
    rc2, scores2, idx2 = _topk(lib, q.to(cuda), g.to(cuda), k)
    assert rc2 == 0 and torch.equal(scores, scores2) and torch.equal(idx, idx2)


@pytest.mark.gpu
def test_topk_dot_empty_slots_and_refusals(lib, cuda):
    q, g, S = _data("bf16", 64)
    qd, gd = q.to(cuda), g.to(cuda)
    rc, scores, idx = _topk(lib, qd, gd, 64, None, 17, 15)  # G = 15, k = 64: the tail is -1 / -inf
    assert rc == 0
    assert bool((idx[:, 15:] == -1).all()) and bool((scores[:, 15:] == float("-inf")).all()) and bool((idx[:, :15] >= 0).all())
    ex = torch.arange(17, dtype=torch.int32) % 15
    rc, scores, idx = _topk(lib, qd, gd, 15, ex.to(cuda), 17, 15)  # exclude and k = G: exactly one empty slot
    assert rc == 0
    assert bool(((idx == -1).sum(dim=1) == 1).all()) and bool((idx[:, -1] == -1).all()) and bool((scores[:, -1] == float("-inf")).all())
    RR.check_topk(scores, idx, S[:17, :15], 15, BAR, ex)
    for k in (0, 65):
        rc, _, _ = _topk(lib, qd, gd, k, None, 17, 15)
        assert rc == -1 and b"k must be" in lib.hct_last_error_string()
    # the memory condition: the partial lists of a 4096 x 1 000 000 search are below 1 % of its score matrix
    assert 0 < lib.hct_topk_dot_workspace(4096, 1_000_000, 10) < 0.01 * 4096 * 1e6 * 4


# ---- hct_attention_row_probs -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dh", [16, 48, 64])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_attention_row_probs(lib, cuda, dtype, dh):
    """Against the fp64 softmax of the stored qkv (relative L2 <= 1e-3, rows sum to 1 within 1e-5), and tied to hct_attention_fwd:
    probs @ v gives the matching rows of its o, log-sum-exp of the fp64 logits its lse."""
    from headct_foundation_amd import _lib
    from headct_foundation_amd.retrieval import attention_row_probs
    B, H = 2, 3
    tol = 1e-3 if dtype == "fp32" else 2e-2
    worst = 0.0
    for N in (9, 32, 65, 217, 513):
        qkv = torch.randn(B, N, 3, H, dh, generator=torch.Generator().manual_seed(N + dh)).to(DTYPES[dtype])
        p_ref, lse_ref, _ = RR.attention_ref(qkv, B, N, H, dh)
        v = qkv.double().view(B, N, 3, H, dh)[:, :, 2].permute(0, 2, 1, 3)  # [B, H, N, dh]
        qd = qkv.to(cuda)
        o = torch.empty(B, N, H * dh, dtype=DTYPES[dtype], device=cuda)
        lse = torch.empty(B, H, N, dtype=torch.float32, device=cuda)
        _lib.check(lib.hct_attention_fwd(qd.data_ptr(), B, N, H, dh, _lib.dtype_code(qd), o.data_ptr(), lse.data_ptr(), _st()), "hct_attention_fwd")
        for rows in ([0], [0, 5, N - 1]):
            probs = attention_row_probs(qd, B, N, H, dh, rows).cpu()
            assert probs.shape == (B, H, len(rows), N) and probs.dtype == torch.float32
            err = rel_err(probs, p_ref[:, :, rows])
            worst = max(worst, err)
            assert err <= 1e-3, (N, rows, err)
            assert float((probs.double().sum(dim=-1) - 1).abs().max()) <= 1e-5
            pv = (probs.double() @ v).permute(0, 2, 1, 3).reshape(B, len(rows), H * dh)  # rows of o, head-merged
            assert rel_err(o[:, rows].cpu(), pv) <= tol, (N, rows)
            assert float((lse[:, :, rows].cpu().double() - lse_ref[:, :, rows]).abs().max()) <= tol, (N, rows)
    print(f"hct_attention_row_probs {dtype} dh={dh}: largest relative L2 error {worst:.2e}")


@pytest.mark.gpu
def test_attention_row_probs_refuses_rows_out_of_range(lib, cuda):
    from headct_foundation_amd import HctError
    from headct_foundation_amd.retrieval import attention_row_probs
    qkv = torch.zeros(1, 9, 3, 2, 16, device=cuda)
    for rows in ([9], [-1], [0, 100], []):
        with pytest.raises(HctError):
            attention_row_probs(qkv, 1, 9, 2, 16, rows)


# ---- model level -------------------------------------------------------------------------------------------------------------
def _case_vit(dtype, norm, cuda):
    """The tiny ViT of tests/lora_ref.py::CASE with values by seed; the qkv weights are scaled up so that the attention is far from
    uniform (at the fixture's 0.02 every probability is 1 / T to three digits and an error in the logits would not show)."""
    import torch.nn as nn
    from headct_foundation_amd import RMSNorm, ViT
    c = CASE
    vit = ViT(in_chans=c["in_chans"], img_size=c["img_size"], patch_size=c["patch_size"], hidden_size=c["hidden_size"], mlp_dim=c["mlp_dim"],
              num_layers=c["num_layers"], num_heads=c["num_heads"], num_register_tokens=c["num_register_tokens"], qkv_bias=c["qkv_bias"],
              norm_layer=RMSNorm if norm == "rmsnorm" else nn.LayerNorm, compute_dtype=dtype)
    p = O.make_vit_params({k: tuple(v.shape) for k, v in vit.state_dict().items()}, c["seed"])
    for k in p:
        if k.endswith("attn.qkv.weight"):
            p[k] = p[k] * 10.0
    vit.load_state_dict(p)
    n = c["batch"] * c["in_chans"] * c["img_size"] ** 3
    x = torch.from_numpy(O.hash_uniform(n, c["x_seed"]).astype("float32")).view(c["batch"], c["in_chans"], *[c["img_size"]] * 3)
    return vit.to(cuda), p, x


@pytest.mark.gpu
@pytest.mark.parametrize("norm", ["layernorm", "rmsnorm"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_get_selfattention_vs_restatement(lib, cuda, dtype, norm):
    c = CASE
    vit, p, x = _case_vit(dtype, norm, cuda)
    T = 1 + c["num_register_tokens"] + (c["img_size"] // c["patch_size"]) ** 3
    _, atts = RR.vit_attention(p, x, c["patch_size"], c["num_heads"], c["num_layers"], torch.float64 if dtype == "fp32" else torch.float32)
    assert float(atts[0].max()) > 3.0 / T  # the restated attention is not uniform
    tol = 1e-3 if dtype == "fp32" else 5e-2
    rows = [0, 2, T - 1]
    for b in range(c["num_layers"]):
        got = vit.get_selfattention(x.to(cuda), block=b, rows=rows)
        assert got.shape == (c["batch"], c["num_heads"], len(rows), T) and got.dtype == torch.float32
        err = rel_err(got, atts[b][:, :, rows])
        print(f"get_selfattention {dtype} {norm} block {b}: relative L2 error {err:.2e}")
        assert err <= tol, (b, err)
    assert torch.equal(vit.get_selfattention(x.to(cuda), block=-1, rows=rows), got)
    assert torch.equal(vit.get_selfattention(x.to(cuda)), got[:, :, :1])  # defaults: last block, class token


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_forward_is_unchanged_by_attention_calls(lib, cuda, dtype):
    vit, _, x = _case_vit(dtype, "layernorm", cuda)
    xd = x.to(cuda)
    out0, hid0 = vit(xd)
    out0, hid0 = out0.clone(), [h.clone() for h in hid0]
    vit.get_selfattention(xd, block=0, rows=(0, 1))
    vit.attention_map(xd)
    out1, hid1 = vit(xd)
    assert torch.equal(out0, out1) and len(hid0) == len(hid1) and all(torch.equal(a, b) for a, b in zip(hid0, hid1))
    out2, hid2, kept = vit._run(xd)
    assert kept is None and torch.equal(out0, out2) and all(torch.equal(a, b) for a, b in zip(hid0, hid2))


@pytest.mark.gpu
def test_attention_map_layout_and_upsampling(lib, cuda):
    c = CASE
    vit, p, x = _case_vit("fp32", "layernorm", cuda)
    xd = x.to(cuda)
    g, S, R, H, B = c["img_size"] // c["patch_size"], c["img_size"], c["num_register_tokens"], c["num_heads"], c["batch"]
    _, atts = RR.vit_attention(p, x, c["patch_size"], H, c["num_layers"])
    for b in (0, -1):
        m = vit.attention_map(xd, block=b, upsample=None)
        assert m.shape == (B, H, g, g, g)
        # class and register columns dropped, patches in (gh, gw, gd) order: the restated class-token row, reshaped
        want = atts[b][:, :, 0, 1 + R:].reshape(B, H, g, g, g)
        assert rel_err(m, want) <= 1e-3
    assert torch.equal(m.reshape(B, H, -1), vit.get_selfattention(xd)[:, :, 0, 1 + R:])
    near = vit.attention_map(xd, upsample="nearest")
    assert near.shape == (B, H, S, S, S)
    blocks = near.reshape(B, H, g, S // g, g, S // g, g, S // g)
    assert torch.equal(blocks, m.reshape(B, H, g, 1, g, 1, g, 1).expand_as(blocks))  # constant over each patch
    tri = vit.attention_map(xd)
    want = F.interpolate(m.cpu(), size=(S, S, S), mode="trilinear", align_corners=False)
    assert tri.shape == (B, H, S, S, S) and float((tri.cpu() - want).abs().max()) <= 1e-6
    with pytest.raises(ValueError):
        vit.attention_map(xd, upsample="cubic")


@pytest.mark.gpu
@pytest.mark.parametrize("D", [48, 768])
@pytest.mark.parametrize("dtype,bar", [("fp32", 1e-4), ("bf16", 5e-3)])
def test_feature_bank_search_end_to_end(lib, cuda, dtype, bar, D):
    """From raw fp32 features against fp64 cosine.  bf16 bank: two operands each rounded to within 2^-9 relative with
    sum |q_i g_i| <= 1 give 2^-8 ~ 3.9e-3, plus accumulation."""
    from headct_foundation_amd import FeatureBank
    gen = torch.Generator().manual_seed(D)
    G, Q, k = 300, 20, 10
    gf, qf = torch.randn(G, D, generator=gen) * 3.0 + 0.5, torch.randn(Q, D, generator=gen) * 0.2 + 0.5
    S = F.normalize(qf.double(), dim=1) @ F.normalize(gf.double(), dim=1).T
    bank = FeatureBank(gf.to(cuda), labels=torch.arange(G) % 3, dtype=dtype)
    assert len(bank) == G and bank.feats.dtype == DTYPES[dtype]
    scores, idx = bank.search(qf.to(cuda), k)
    assert scores.dtype == torch.float32 and idx.dtype == torch.int32
    RR.check_topk(scores, idx, S, k, bar)
    # leave-one-out search of the bank against itself never returns the query
    Sself = F.normalize(gf.double(), dim=1) @ F.normalize(gf.double(), dim=1).T
    scores, idx = bank.search(None, k, exclude="self")
    assert not bool((idx.cpu() == torch.arange(G).view(-1, 1)).any())
    RR.check_topk(scores, idx, Sself, k, bar, torch.arange(G))
    scores_in, idx_in = bank.search(gf.to(cuda), 1)  # without the exclusion every scan finds itself
    assert torch.equal(idx_in.cpu().view(-1).to(torch.int64), torch.arange(G))


# ---- plumbing run --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_main_retrieval_plumbing_run(lib, cuda, tmp_path):
    """main_retrieval.py as a subprocess: synthetic data, the tiny ViT, a checkpoint saved here."""
    from headct_foundation_amd.dino_model import ViTBackbone
    torch.manual_seed(0)
    vit = ViTBackbone(in_chans=3, img_size=24, patch_size=12, hidden_size=48, mlp_dim=96, num_layers=2, num_heads=3, compute_dtype="fp32")
    torch.save({"state_dict": {"module." + k: v for k, v in vit.state_dict().items()}, "epoch": 3}, tmp_path / "pre.pt")
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("MODEL:\n  NAME: vit\n")
    out = tmp_path / "out"
    opts = ["DATA.SYNTHETIC", "True", "DATA.SYNTHETIC_SAMPLES", "32", "VIT.INPUT_SIZE", "24", "VIT.PATCH_SIZE", "12", "VIT.HIDDEN_SIZE", "48",
            "VIT.MLP_DIM", "96", "VIT.NUM_LAYERS", "2", "VIT.NUM_HEADS", "3", "MAE.COMPUTE_DTYPE", "fp32", "LOG.OUTPUT_DIR", str(tmp_path / "log")]
    cmd = [sys.executable, os.path.join(ROOT, "main_retrieval.py"), "--cfg", str(cfg), "--model_name", "vit", "--model_load_path", str(tmp_path / "pre.pt"),
           "--batch_size", "4", "--topk", "1", "5", "--attention_maps", "1", "--bank_dtype", "fp32", "--pooling", "cls_mean", "--save_dir", str(out),
           "--opts"] + opts
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-4000:]
    gf, qf = np.load(out / "gallery_features.npy"), np.load(out / "query_features.npy")
    gl, ql, nb = np.load(out / "gallery_labels.npy"), np.load(out / "query_labels.npy"), np.load(out / "neighbours.npy")
    gn, qn = json.load(open(out / "gallery_names.json")), json.load(open(out / "query_names.json"))
    assert gf.shape == (32, 96) and qf.shape == (8, 96) and gf.dtype == np.float32  # cls_mean: 2 D
    assert len(gl) == len(gn) == 32 and len(ql) == len(qn) == 8 and nb.shape == (8, 5) and nb.dtype == np.int32
    m = json.load(open(out / "retrieval.json"))
    assert {"P@1", "mAP@1", "P@5", "mAP@5", "kNN_accuracy", "kNN_AUROC"} <= set(m)
    assert "P@5" in log and "MulticlassAUROC" in log
    # the neighbours recomputed from the saved features (fp64 cosine) pass the rank-robust check; scores are not saved, so they are the
    # reference's own at the saved rows
    S = F.normalize(torch.from_numpy(qf).double(), dim=1) @ F.normalize(torch.from_numpy(gf).double(), dim=1).T
    idx = torch.from_numpy(nb)
    RR.check_topk(torch.gather(S, 1, idx.to(torch.int64)), idx, S, 5, 1e-4, order_slack=2e-4)
    want = RR.retrieval_metrics_brute(nb, ql, gl, (1, 5))
    assert all(abs(m[k] - want[k]) < 1e-9 for k in want)
    att = np.load(out / "attention_0.npy")
    assert att.shape == (3, 24, 24, 24) and att.dtype == np.float16 and not os.path.exists(out / "attention_1.npy")
