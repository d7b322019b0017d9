"""Host side of retrieval and attention maps: exported symbols, metrics, k-NN, pooling, the entry point's flags (no GPU)."""
import os
import re
import sys

import numpy as np
import pytest
import torch

from tests import retrieval_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("hct_topk_dot", "hct_topk_dot_workspace", "hct_topk_dot_chunks", "hct_attention_row_probs")


def test_new_symbols_are_exported_declared_and_host_checked(lib):
    import headct_foundation_amd as pkg
    from headct_foundation_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "headct_hip.h")).read()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b" + s + r"\s*\(", hdr) and s in _lib.exported_symbols() and hasattr(lib, s), s
    assert "retrieval.hip" in build.SOURCES
    for s in ("FeatureBank", "extract_features", "knn_predict", "pool_tokens", "retrieval_metrics"):
        assert hasattr(pkg, s), s
    # host arithmetic: chunks = min(ceil(G / 1024), max(1, 2048 / ceil(Q / 64))), workspace = Q * chunks * k keys of 8 bytes
    assert lib.hct_topk_dot_chunks(70, 1000) == 1 and lib.hct_topk_dot_chunks(70, 5000) == 5 and lib.hct_topk_dot_chunks(1, 1) == 1
    assert lib.hct_topk_dot_chunks(4096, 1_000_000) == 32
    assert lib.hct_topk_dot_workspace(70, 5000, 10) == 70 * 5 * 10 * 8
    assert lib.hct_topk_dot_workspace(4096, 1_000_000, 10) < 0.01 * 4096 * 1e6 * 4
    assert lib.hct_topk_dot_workspace(4, 100, 0) == 0 and lib.hct_topk_dot_workspace(4, 100, 65) == 0
    # argument checks come back as HCT_E_BADARG before any launch
    for k in (0, 65):
        assert lib.hct_topk_dot(None, 4, None, 100, 64, _lib.HCT_BF16, None, k, None, None, None, 0, None) == -1
        assert b"hct_topk_dot" in lib.hct_last_error_string()
    assert lib.hct_attention_row_probs(None, 1, 8, 1, 12, _lib.HCT_F32, None, 1, None, None) == -1
    assert b"multiple of 8" in lib.hct_last_error_string()


@pytest.mark.parametrize("with_empty", [False, True])
def test_retrieval_metrics_against_brute_force(with_empty):
    from headct_foundation_amd.retrieval import retrieval_metrics
    rng = np.random.RandomState(5)
    Q, G, K = 37, 200, 10
    gl, ql = rng.randint(0, 4, size=G), rng.randint(0, 4, size=Q)
    idx = np.stack([rng.permutation(G)[:K] for _ in range(Q)])
    if with_empty:
        idx[::3, 6:] = -1
        idx[5] = -1
    ks = (1, 5, 10)
    got = retrieval_metrics(torch.from_numpy(idx).to(torch.int32), torch.from_numpy(ql), torch.from_numpy(gl), ks)
    want = RR.retrieval_metrics_brute(idx, ql, gl, ks)
    assert set(got) == {f"{m}@{k}" for m in ("P", "mAP") for k in ks}
    for key in want:
        assert abs(got[key] - want[key]) < 1e-12, (key, got[key], want[key])


def test_retrieval_metrics_hand_worked_query():
    from headct_foundation_amd.retrieval import retrieval_metrics
    gl = torch.tensor([1, 0, 1, 1, 0, 0])
    idx = torch.tensor([[0, 1, 2, 3, 4]], dtype=torch.int32)  # relevant at ranks 1, 3, 4 of 5
    m = retrieval_metrics(idx, torch.tensor([1]), gl, (5,))
    assert abs(m["P@5"] - 0.6) < 1e-12 and abs(m["mAP@5"] - (1 + 2 / 3 + 3 / 4) / 3) < 1e-12
    m = retrieval_metrics(torch.full((1, 5), -1, dtype=torch.int32), torch.tensor([1]), gl, (1, 5))
    assert m == {"P@1": 0.0, "mAP@1": 0.0, "P@5": 0.0, "mAP@5": 0.0}
    both = retrieval_metrics(torch.cat([idx, torch.full((1, 5), -1, dtype=torch.int32)]), torch.tensor([1, 1]), gl, (5,))
    assert abs(both["P@5"] - 0.3) < 1e-12 and abs(both["mAP@5"] - (1 + 2 / 3 + 3 / 4) / 6) < 1e-12
    with pytest.raises(ValueError):
        retrieval_metrics(idx, torch.tensor([1]), gl, (6,))


def test_knn_predict_against_numpy():
    from headct_foundation_amd.retrieval import knn_predict
    rng = np.random.RandomState(2)
    Q, G, K, C = 11, 50, 7, 3
    gl = rng.randint(0, C, size=G)
    idx = np.stack([rng.permutation(G)[:K] for _ in range(Q)]).astype(np.int32)
    scores = np.sort(rng.uniform(-1, 1, size=(Q, K)).astype(np.float32), axis=1)[:, ::-1].copy()
    idx[3, 4:] = -1
    scores[3, 4:] = -np.inf
    idx[7] = -1
    scores[7] = -np.inf
    for T in (0.07, 1.0):
        got = knn_predict(torch.from_numpy(scores), torch.from_numpy(idx), torch.from_numpy(gl), C, T=T)
        want = RR.knn_ref(scores, idx, gl, C, T)
        assert got.shape == (Q, C) and got.dtype == torch.float32
        assert np.abs(got.numpy() - want).max() < 1e-5
        assert np.abs(got.numpy().sum(axis=1) - 1).max() < 1e-5
    assert np.allclose(got[7].numpy(), 1 / C)


@pytest.mark.parametrize("regs", [0, 2])
def test_pool_tokens_against_numpy(regs):
    from headct_foundation_amd.retrieval import pool_tokens
    t = torch.randn(3, 1 + regs + 8, 12, generator=torch.Generator().manual_seed(1))
    for pooling, width in (("cls", 12), ("mean", 12), ("cls_mean", 24)):
        got = pool_tokens(t, regs, pooling)
        assert got.shape == (3, width)
        assert np.abs(got.numpy() - RR.pool_ref(t.numpy(), regs, pooling)).max() < 1e-6
    # the register tokens do not leak into the mean
    t2 = t.clone()
    t2[:, 1:1 + regs] += 100.0
    assert torch.equal(pool_tokens(t2, regs, "mean"), pool_tokens(t, regs, "mean"))
    with pytest.raises(ValueError):
        pool_tokens(t, regs, "max")


def test_main_retrieval_parses_the_new_flags(tmp_path, monkeypatch):
    import main_retrieval as M
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("MODEL:\n  NAME: vit\n")
    monkeypatch.setattr(sys, "argv", ["main_retrieval.py", "--cfg", str(cfg), "--model_name", "vit", "--model_load_path", "x.pt", "--pooling", "cls_mean",
                                      "--topk", "1", "5", "--bank_dtype", "fp32", "--attention_maps", "2", "--save_dir", str(tmp_path / "out"),
                                      "--gallery_csv_path", "g.csv", "--query_csv_path", "q.csv", "--batch_size", "4"])
    args, config = M.parse_option()
    assert args.topk == [1, 5] and args.bank_dtype == "fp32" and args.attention_maps == 2 and args.save_dir == str(tmp_path / "out")
    assert config.VIT.POOLING == "cls_mean" and config.MODEL.PRETRAINED == "x.pt" and config.DATA.BATCH_SIZE == 4
    assert config.DATA.TRAIN_CSV_PATH == "g.csv" and config.DATA.TEST_CSV_PATH == "q.csv"
    monkeypatch.setattr(sys, "argv", ["main_retrieval.py", "--cfg", str(cfg)])
    args, config = M.parse_option()
    assert args.topk == [1, 5, 10] and args.bank_dtype == "bf16" and args.attention_maps == 0 and config.VIT.POOLING == "cls"


def test_gpu_only_paths_refuse_the_cpu():
    from headct_foundation_amd import FeatureBank, HctError
    from headct_foundation_amd.retrieval import attention_row_probs, topk_dot
    with pytest.raises(HctError):
        FeatureBank(torch.zeros(4, 8))
    with pytest.raises(HctError):
        topk_dot(torch.zeros(2, 8), torch.zeros(4, 8), 1)
    with pytest.raises(HctError):  # an out-of-range row is refused before anything is launched
        attention_row_probs(torch.zeros(1, 4, 3, 1, 8), 1, 4, 1, 8, [0, 4])
