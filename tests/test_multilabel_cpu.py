"""CPU: the host side of multi-label fine-tuning (TRAIN.LABEL_NAMES) -- label reader, sampling and positive weights, the
per-label metrics against scikit-learn, config / CLI / head width, the argument checks of hct_sigmoid_bce that return before any
launch, and the case list of the GPU test against the loop constants of csrc/multilabel.hip."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import multilabel_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RSNA = ["epidural", "intraparenchymal", "intraventricular", "subarachnoid", "subdural", "any"]


# ---- readers and weights ------------------------------------------------------------------------------------------------------------
def _write_csv(path, rows):
    path.write_text("\n".join([",".join(["img_path"] + RSNA)] + [",".join(r) for r in rows]) + "\n")
    return str(path)


def test_read_multilabels(tmp_path):
    from headct_foundation_amd.data import read_multilabels
    rows = [["a.nii", "0", "1", "", "nan", "-1", "1"],
            ["b.nii", "1", "0", "0", "NaN", "1.0", "0"],
            ["a.nii", "1", "1", "0", "0", "0", "-1.0"]]  # a.nii again: the last row wins in label_of
    f = _write_csv(tmp_path / "t.csv", rows)
    paths, labels, label_of = read_multilabels(f, "rsna", ["any", "epidural", "intraventricular", "subarachnoid", "subdural"])
    assert paths == ["a.nii", "b.nii", "a.nii"]
    assert labels.dtype == np.float32 and labels.shape == (3, 5)
    assert labels.tolist() == [[1, 0, -1, -1, -1], [0, 1, 0, -1, 1], [-1, 1, 0, 0, 0]]
    assert set(label_of) == {"a.nii", "b.nii"} and label_of["a.nii"].tolist() == [-1, 1, 0, 0, 0] and label_of["b.nii"].tolist() == [0, 1, 0, -1, 1]
    p_all, l_all, _ = read_multilabels(f, "rsna", ["all"])
    assert l_all.shape == (3, 6) and l_all[1].tolist() == [1, 0, 0, -1, 1, 0]
    bad = _write_csv(tmp_path / "bad.csv", rows + [["c.nii", "0", "0", "2", "0", "0", "0"]])
    with pytest.raises(ValueError) as e:
        read_multilabels(bad, "rsna", ["all"])
    assert "bad.csv" in str(e.value) and "row 3" in str(e.value) and "intraventricular" in str(e.value)
    with pytest.raises(ValueError):
        read_multilabels(f, "rsna", ["ICH"])  # not one of rsna's


def test_all_expands_in_class_mappings_order():
    from headct_foundation_amd.data import CLASS_MAPPINGS, expand_label_names
    assert expand_label_names("rsna", ["all"]) == RSNA == CLASS_MAPPINGS["rsna"]
    assert len(expand_label_names("cq500", ["all"])) == 14 and len(expand_label_names("nyu", ["all"])) == 11
    assert expand_label_names("rsna", ["any", "subdural"]) == ["any", "subdural"]


def test_sample_weights_single_label_is_the_single_label_path():
    from headct_foundation_amd.data import WeightedShardSampler, class_weights, multilabel_sample_weights
    rng = np.random.default_rng(3)
    y = (rng.random(61) < 0.23).astype(np.int64)
    want = class_weights(y, 2).double().numpy()[y]  # what the single-label loader hands its sampler
    got = multilabel_sample_weights(y.reshape(-1, 1).astype(np.float32))
    assert got.shape == (61,) and np.array_equal(got, want)
    assert np.array_equal(got.astype(np.float32), class_weights(y, 2)[torch.from_numpy(y)].numpy())
    for rank, world in ((0, 1), (1, 2)):
        a = list(WeightedShardSampler(got, 40, rank, world, seed=42 + rank))
        b = list(WeightedShardSampler(want, 40, rank, world, seed=42 + rank))
        assert a == b and len(a) == 40


def _table():
    rng = np.random.default_rng(5)
    y = (rng.random((40, 3)) < np.array([0.5, 0.2, 0.8])).astype(np.float32)
    y[rng.random((40, 3)) < 0.25] = -1.0
    y[7] = -1.0  # a row without a valid label
    return y


def test_sample_weights_with_gaps_is_the_double_loop():
    from headct_foundation_amd.data import multilabel_sample_weights
    y = _table()
    got = multilabel_sample_weights(y)
    want = np.zeros(len(y))
    for i in range(len(y)):
        acc, k = 0.0, 0
        for t in range(y.shape[1]):
            if y[i, t] < 0:
                continue
            total = int((y[:, t] >= 0).sum())
            count = int((y[:, t] == y[i, t]).sum())
            acc += float(np.float32(1 / (count / total)))  # each ratio is class_weights' fp32 value
            k += 1
        want[i] = acc / k if k else 0.0
    empty = (y < 0).all(axis=1)
    assert empty[7] and (got[empty] == 0.0).all() and (got[~empty] > 0).all()
    assert np.allclose(got, want, rtol=1e-15, atol=0.0)


def test_pos_weight_is_its_formula():
    from headct_foundation_amd.data import multilabel_pos_weight, multilabel_sample_weights
    y = _table()
    w = multilabel_sample_weights(y)
    got = multilabel_pos_weight(y, w)
    assert got.dtype == torch.float32 and got.shape == (3,)
    for t in range(3):
        neg = sum(w[i] for i in range(len(y)) if y[i, t] == 0)
        pos = sum(w[i] for i in range(len(y)) if y[i, t] == 1)
        assert abs(float(got[t]) - neg / pos) <= 1e-6 * neg / pos
    ones = np.ones(len(y))  # unweighted: the plain count ratio
    plain = multilabel_pos_weight(y, ones)
    assert np.allclose(plain.numpy(), [(y[:, t] == 0).sum() / (y[:, t] == 1).sum() for t in range(3)], rtol=1e-6)


def test_weights_refuse_a_column_without_one_of_the_values():
    from headct_foundation_amd.data import multilabel_pos_weight, multilabel_sample_weights
    y = _table()
    y[y[:, 1] == 1, 1] = -1.0  # label 1 has no positive left
    with pytest.raises(ValueError, match="column 1.*value 1"):
        multilabel_sample_weights(y)
    with pytest.raises(ValueError, match="'b'.*value 1"):
        multilabel_pos_weight(y, np.ones(len(y)), names=["a", "b", "c"])
    z = _table()
    z[z[:, 2] == 0, 2] = 1.0
    with pytest.raises(ValueError, match="column 2.*value 0"):
        multilabel_sample_weights(z)


def test_labelled_volumes_yields_label_rows(tmp_path):
    """LabelledVolumes with rows of labels: fp32 [B, T] targets, and an all-missing row for a scan that failed to load."""
    from headct_foundation_amd.data import LabelledVolumes, VolumeCache

    def loader(path, roi, in_channels, device):
        if path == "broken.nii":
            raise OSError("unreadable")
        return torch.zeros((in_channels,) + tuple(roi), dtype=torch.float16)

    class _Cast:  # the device augmentation has no CPU path: stand in for the cast
        def __call__(self, x):
            return x.float()

    cache = VolumeCache(tmp_path / "cache", [4, 4, 4], 1, loader=loader)
    label_of = {"a.nii": np.array([1, -1, 0], np.float32), "broken.nii": np.array([1, 1, 1], np.float32), "b.nii": np.array([0, 0, 1], np.float32)}
    lv = LabelledVolumes(["a.nii", "broken.nii", "b.nii"], label_of, [0, 1, 2], cache, 3, "cpu", augment=_Cast(), pool=None, num_workers=1)
    (vol, target, names), = list(lv)
    assert target.dtype == torch.float32 and target.tolist() == [[1, -1, 0], [-1, -1, -1], [0, 0, 1]] and names == ["a.nii", "None", "b.nii"]
    single = LabelledVolumes(["a.nii", "b.nii"], {"a.nii": 1, "b.nii": 0}, [0, 1], cache, 2, "cpu", augment=_Cast(), pool=None, num_workers=1)
    (_, t1, _), = list(single)
    assert t1.dtype == torch.int64 and t1.tolist() == [1, 0]


def test_loaders_refuse_few_shots_in_multilabel_mode(tmp_path):
    import config as cfgmod
    from headct_foundation_amd.data import get_fewshots_dataloaders
    f = _write_csv(tmp_path / "t.csv", [["a.nii", "0", "1", "0", "1", "0", "1"], ["b.nii", "1", "0", "1", "0", "1", "0"]])
    c = cfgmod._C.clone()
    c.DATA.TRAIN_CSV_PATH = c.DATA.VAL_CSV_PATH = c.DATA.TEST_CSV_PATH = f
    c.DATA.DATASET, c.DATA.FEW_SHOTS, c.DATA.CACHE_DIR = "rsna", 2, str(tmp_path / "cache")
    c.TRAIN.LABEL_NAMES = ["any", "subdural"]
    c.MODEL.ROI, c.VIT.INPUT_SIZE = [24, 24, 24], 24
    with pytest.raises(ValueError, match="per class of one label"):
        get_fewshots_dataloaders(c, "cpu")


def test_synthetic_multilabelled():
    from headct_foundation_amd.data import SyntheticMultiLabelled
    s = SyntheticMultiLabelled(5, 4, 2, 12, 14, "cpu", seed=1)
    assert len(s) == 5 and len(set(s.boxes)) == 14
    allt = torch.cat([t for _, t, _ in s.batches])
    assert abs(float((allt < 0).float().mean()) - 1 / 7) < 0.02 and bool((allt < 0).any(dim=0).all())
    again = SyntheticMultiLabelled(5, 4, 2, 12, 14, "cpu", seed=1)
    for i, (v, t, names) in enumerate(s.batches):
        assert v.shape == (4, 2, 12, 12, 12) and t.shape == (4, 14) and t.dtype == torch.float32 and len(names) == 4
        truth = ((torch.arange(1, 15).view(1, -1) >> ((torch.arange(4) + i) % 4).view(-1, 1)) & 1).float()
        assert bool(((t == truth) | (t < 0)).all())
        assert bool((truth.sum(0) > 0).all()) and bool((truth.sum(0) < 4).all())  # both values in every batch of 4
        assert torch.equal(v, again.batches[i][0])
        for k, (z, y, x) in enumerate(s.boxes):  # label k brightens its own sub-cube
            m = v[:, :, z:z + 4, y:y + 4, x:x + 4].mean(dim=(1, 2, 3, 4))
            assert bool((m[truth[:, k] == 1] > 0.85).all()) and bool((m[truth[:, k] == 0] < 0.65).all())
    with pytest.raises(ValueError, match="14"):
        SyntheticMultiLabelled(1, 4, 1, 12, 15, "cpu")


# ---- metrics ------------------------------------------------------------------------------------------------------------------------
def test_multilabel_metrics_vs_sklearn():
    from sklearn.metrics import average_precision_score, roc_auc_score
    from headct_foundation_amd.metrics import MultilabelMetrics
    rng = np.random.default_rng(11)
    N, T = 400, 5
    rate = np.array([0.5, 0.3, 0.05, 0.7, 0.4])
    t = (rng.random((N, T)) < rate).astype(np.float32)
    p = np.round(np.clip(0.35 * t + 0.65 * rng.random((N, T)), 0, 1), 1).astype(np.float32)  # one decimal: ties
    t[rng.random((N, T)) < 0.15] = -1.0
    t[t[:, 4] == 1, 4] = 0.0  # label 4: all-negative among its valid entries
    names = ["a", "b", "c", "d", "e"]
    m = MultilabelMetrics(names)
    for lo, hi in ((0, 57), (57, 301), (301, 400)):
        m(torch.from_numpy(p[lo:hi]), torch.from_numpy(t[lo:hi]))
    out = m.compute()
    assert set(out) == {"MultilabelAccuracy", "MultilabelAUROC", "MultilabelAveragePrecision"}
    assert all(v.shape == (T,) and v.dtype == np.float32 for v in out.values())
    assert m.has_both_values().tolist() == [True, True, True, True, False]
    for c in range(4):
        v = t[:, c] >= 0
        assert len(np.unique(p[v, c])) < 12 and 5 < (t[v, c] == 1).sum() < v.sum()
        assert abs(out["MultilabelAUROC"][c] - roc_auc_score(t[v, c], p[v, c])) <= 1e-6
        assert abs(out["MultilabelAveragePrecision"][c] - average_precision_score(t[v, c], p[v, c])) <= 1e-6
        assert abs(out["MultilabelAccuracy"][c] - ((p[v, c] >= 0.5) == (t[v, c] == 1)).sum() / v.sum()) <= 1e-6
    assert out["MultilabelAUROC"][4] == out["MultilabelAveragePrecision"][4] == out["MultilabelAccuracy"][4] == 0.0
    m.reset()
    assert m.compute()["MultilabelAUROC"].tolist() == [0.0] * T
    with pytest.raises(ValueError):
        m(p[:3, :4], t[:3, :4])


# ---- config, CLI, head width ----------------------------------------------------------------------------------------------------------
def _parse(monkeypatch, tmp_path, argv):
    import main_downstream
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("MODEL:\n  NAME: vit\nVIT:\n  INPUT_SIZE: 24\n  PATCH_SIZE: 12\n  HIDDEN_SIZE: 48\n  MLP_DIM: 96\n  NUM_LAYERS: 1\n  NUM_HEADS: 3\n")
    monkeypatch.setattr("sys.argv", ["main_downstream.py", "--cfg", str(cfg)] + argv)
    return main_downstream.parse_option()[1]


def test_label_names_reach_the_config(monkeypatch, tmp_path):
    import config as cfgmod
    assert cfgmod._C.TRAIN.LABEL_NAMES == [] and cfgmod._C.TRAIN.POS_WEIGHT == "none"
    c = _parse(monkeypatch, tmp_path, ["--label_names", "ICH", "IPH", "--pos_weight", "balanced"])
    assert c.TRAIN.LABEL_NAMES == ["ICH", "IPH"] and c.TRAIN.POS_WEIGHT == "balanced"
    c = _parse(monkeypatch, tmp_path, ["--opts", "TRAIN.LABEL_NAMES", "['ICH','IPH']"])
    assert c.TRAIN.LABEL_NAMES == ["ICH", "IPH"] and c.TRAIN.POS_WEIGHT == "none"
    assert _parse(monkeypatch, tmp_path, []).TRAIN.LABEL_NAMES == []


@pytest.mark.parametrize("head", ["linear", "attentive"])
def test_build_model_head_width(monkeypatch, tmp_path, head):
    import main_downstream
    c = _parse(monkeypatch, tmp_path, ["--classifier", head])
    _, cls = main_downstream.build_model(c, "cpu")
    assert cls.linear.weight.shape == (2, 48) and cls.linear.bias.shape == (2,)
    c = _parse(monkeypatch, tmp_path, ["--classifier", head, "--dataset", "cq500", "--label_names", "ICH", "IPH", "MidlineShift"])
    _, cls = main_downstream.build_model(c, "cpu")
    assert cls.linear.weight.shape == (3, 48) and cls.linear.bias.shape == (3,)
    c = _parse(monkeypatch, tmp_path, ["--classifier", head, "--dataset", "cq500", "--label_names", "all"])
    assert main_downstream.build_model(c, "cpu")[1].linear.weight.shape == (14, 48)
    with pytest.raises(ValueError, match="not among"):
        main_downstream.build_model(_parse(monkeypatch, tmp_path, ["--dataset", "rsna", "--label_names", "ICH"]), "cpu")
    free = _parse(monkeypatch, tmp_path, ["--label_names", "a", "b", "c", "d", "--opts", "DATA.SYNTHETIC", "True"])
    assert main_downstream.build_model(free, "cpu")[1].linear.weight.shape == (4, 48)  # synthetic data: the names are free
    with pytest.raises(ValueError, match="NUM_CLASSES must be 2"):
        main_downstream.build_model(_parse(monkeypatch, tmp_path, ["--label_names", "ICH", "--opts", "DATA.NUM_CLASSES", "3"]), "cpu")


def test_engine_reexports_and_cpu_tensors_are_refused():
    import engine_downstream
    from headct_foundation_amd import HctError, bce_with_logits
    assert engine_downstream.bce_with_logits is bce_with_logits and "bce_with_logits" in engine_downstream.__all__
    with pytest.raises(HctError, match="no CPU fallback"):
        bce_with_logits(torch.zeros(2, 3), torch.zeros(2, 3))


# ---- ABI: the paths that return before any launch -------------------------------------------------------------------------------------
def test_sigmoid_bce_argument_checks(lib):
    HCT_E_BADARG, HCT_E_WORKSPACE = -1, -3  # include/headct_hip.h
    fake = 4096  # pointers that are never dereferenced: every call below returns before a launch
    need = lib.hct_sigmoid_bce_workspace_bytes(64, 14)
    call = lambda B, loss, label_loss, dlogits, ws_bytes: lib.hct_sigmoid_bce(fake, fake, None, B, 14, None, loss, label_loss, dlogits, fake, ws_bytes, None)
    for rc, want in ((call(0, fake, None, None, need), HCT_E_BADARG), (call(64, None, None, None, need), HCT_E_BADARG),
                     (call(64, fake, fake, fake, need - 1), HCT_E_WORKSPACE)):
        assert rc == want and rc != 0
        assert b"hct_sigmoid_bce" in lib.hct_last_error_string()
    assert lib.hct_sigmoid_bce(fake, fake, None, 64, 0, None, fake, None, None, fake, need, None) == HCT_E_BADARG
    assert lib.hct_sigmoid_bce(fake, fake, None, 64, 14, None, fake, None, None, None, need, None) == HCT_E_WORKSPACE


# ---- sizes and reference --------------------------------------------------------------------------------------------------------------
def test_workspace_bytes_follow_the_shape(lib):
    for B, T in R.CASES + [R.EXTRA_SHAPE, (4096, 33), (100000, 3), (5, 100000)]:
        assert lib.hct_sigmoid_bce_workspace_bytes(B, T) == R.workspace_bytes(B, T), (B, T)
    assert lib.hct_sigmoid_bce_workspace_bytes(0, 3) == 0 == lib.hct_sigmoid_bce_workspace_bytes(3, 0)


def test_cases_cross_the_loop_limits():
    assert {(B, T) for B in (1, 3, 64, 257, 1025) for T in (1, 6, 14, 33)} <= set(R.CASES) and len(set(R.CASES)) == len(R.CASES)
    sh = {c: R.shape(*c) for c in R.CASES}
    assert all(s["cx"] * s["ry"] == R.THREADS and s["cx"] >= min(T, R.THREADS) for (B, T), s in sh.items())
    # the block's thread grid: one column of threads (T = 1), one row of threads (T >= THREADS), widths that are no power of two
    assert any(s["ry"] == R.THREADS for s in sh.values()) and any(s["ry"] == 1 for s in sh.values())
    assert any(T < s["cx"] for (B, T), s in sh.items()) and any(T == s["cx"] > 1 for (B, T), s in sh.items())
    # columns: a second column block that ends raggedly (also the finalize block's second trip over the columns)
    assert any(s["col_blocks"] > 1 and T % s["cx"] for (B, T), s in sh.items())
    # rows of a thread: none (B < ry), one trip, exactly ROW_TRIPS, a ragged last trip
    assert any(B < s["ry"] for (B, T), s in sh.items())
    assert any(s["row_blocks"] == 1 and B == s["ry"] * R.ROW_TRIPS for (B, T), s in sh.items())
    assert any(s["chunk"] % s["ry"] for s in sh.values())
    # row blocks: one, several, the cap (more wanted than MAX_ROW_BLOCKS), a last block that is short
    rbs = {s["row_blocks"] for s in sh.values()}
    assert 1 in rbs and any(1 < r < R.MAX_ROW_BLOCKS // 2 for r in rbs)
    assert any(-(-B // (s["ry"] * R.ROW_TRIPS)) > R.MAX_ROW_BLOCKS for (B, T), s in sh.items())
    assert any(s["row_blocks"] > 1 and B % s["chunk"] for (B, T), s in sh.items())
    assert all(s["row_blocks"] <= R.MAX_ROW_BLOCKS and (s["row_blocks"] - 1) * s["chunk"] < B <= s["row_blocks"] * s["chunk"] for (B, T), s in sh.items())
    # the gradient pass: a partly filled single block, several blocks, a second grid-stride trip that ends raggedly
    per_trip = R.THREADS * R.GRAD_BLOCKS
    sizes = [B * T for B, T in R.CASES]
    assert any(n < R.THREADS for n in sizes) and any(R.THREADS < n < per_trip and n % R.THREADS for n in sizes)
    assert any(per_trip < n < 2 * per_trip and n % R.THREADS for n in sizes)
    assert R.EXTRA_SHAPE == (64, 14)


def test_inputs_are_what_the_issue_sets():
    for B, T in [(64, 14), (257, 33)]:
        x, y, w = R.inputs(B, T)
        xf, yf = x.flatten(), y.flatten()
        i = torch.arange(B * T)
        assert bool((yf[i % 5 == 2] == -1).all()) and set(yf[i % 5 != 2].tolist()) == {0.0, 1.0}
        assert bool((xf[(i % 13 == 5)] == 0).all())
        assert bool((xf[(i % 11 == 3) & (i % 13 != 5)] == -100).all()) and bool((xf[(i % 7 == 0) & (i % 11 != 3) & (i % 13 != 5)] == 100).all())
        assert x.dtype == y.dtype == w.dtype == torch.float32 and 0.05 <= float(w.min()) and float(w.max()) <= 20.0
        assert R.inputs(B, T)[0] is x  # computed once, shared


def test_reference_is_torch_bce_with_logits():
    """The reference's own pieces: the masked sum over max(n, 1), the per-label means, the closed forms the header states, and
    torch's fp32 evaluation of the same inputs two orders inside the bar."""
    x, y, w = R.inputs(257, 33)
    loss, label_loss, grad, n = R.reference(x, y, w, R.DLOSS)
    valid = y >= 0
    assert n == int(valid.sum()) and n < y.numel()
    xd, yd, wd = x.double(), y.double().clamp(min=0), w.double()
    sp = lambda z: z.clamp(min=0) + torch.log1p(torch.exp(-z.abs()))
    l = ((1 - yd) * xd + (1 + (wd - 1) * yd) * sp(-xd)) * valid
    assert abs(float(l.sum() / n) - float(loss)) <= 1e-12 * float(loss)
    assert torch.allclose(l.sum(0) / valid.sum(0), label_loss, rtol=1e-12, atol=0)
    d = R.DLOSS * ((1 - yd) * torch.sigmoid(xd) - wd * yd * torch.sigmoid(-xd)) * valid / n
    assert float((d - grad).abs().max()) * n / R.DLOSS <= 1e-12 and bool((grad[~valid] == 0).all())
    x32 = x.clone().requires_grad_(True)
    l32 = F.binary_cross_entropy_with_logits(x32, y.clamp(min=0), weight=valid.float(), pos_weight=w, reduction="sum") / n
    l32.backward()
    assert abs(float(l32.detach()) - float(loss)) <= 0.01 * R.FP32_BAR * float(loss)
    assert float(((x32.grad.double() * R.DLOSS - grad).abs() * n / (R.DLOSS * wd.clamp(min=1))).max()) <= 0.1 * R.FP32_BAR
    # nothing valid: the reference's numerator is 0 and max(n, 1) keeps it finite
    l0, ll0, g0, n0 = R.reference(x, -torch.ones_like(y), w)
    assert n0 == 0 and float(l0) == 0.0 and not bool(ll0.any()) and not bool(g0.any())
