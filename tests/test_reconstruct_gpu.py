"""MAE reconstruction on the GPU: the two kernels through the C ABI and `MaskedAutoencoderViT.reconstruct` end to end, against the
float64 restatement of tests/reconstruct_ref.py on top of the CPU oracle.  Bars: the project's fp32 bar 1e-3 relative L2 per tensor (the
arithmetic is fp32 on identical inputs: observed values are near 1e-6 and are printed), counts and masks exact, the bf16 prediction
bar 2e-2 for the bf16 model."""
import csv
import dataclasses
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import mae_oracle as O
from tests import reconstruct_ref as RF
from tests.util import build_hip_model, grads_by_name, rel_err

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP32_BAR = 1e-3
BF16_BAR = 2e-2


# ---- kernels through the C ABI ---------------------------------------------------------------------------------------------------
def _kernel_inputs(S, P, C, x_dtype, pred_dtype, norm_pix, B=3):
    """x, two predictions and two masks (CPU), rounded to the tested storage types.  Patch (0, 0) is all zero (air after the HU
    window: variance 0) and patch (0, 1) has a single non-zero voxel; both are masked.  Patches 6 and 7 of every volume are kept in
    both calls."""
    cfg = RF.geometry(S, P, C, norm_pix)
    L, pd = cfg.num_patches, cfg.patch_dim
    assert L == 8
    g = torch.Generator().manual_seed(S * 100 + P * 10 + C)
    xp = torch.rand(B, L, pd, generator=g)
    xp[0, 0] = 0.0
    xp[0, 1] = 0.0
    xp[0, 1, pd // 3] = 0.625
    x = O.unpatchify(cfg, xp).contiguous().to(x_dtype)
    preds = [torch.randn(B, L, pd, generator=g).to(pred_dtype) for _ in range(2)]
    m1 = torch.tensor([1, 1, 0, 1, 0, 1, 0, 0], dtype=torch.float32).repeat(B, 1)
    m2 = torch.tensor([0, 1, 1, 1, 0, 0, 0, 0], dtype=torch.float32).repeat(B, 1)
    m2[1] = torch.tensor([1, 0, 0, 1, 1, 1, 0, 0], dtype=torch.float32)
    return cfg, x, preds, [m1, m2]


def _run_kernels(cfg, x, preds, masks, has_cls, dev, inplace):
    from headct_foundation_amd.reconstruct import recon_accum, recon_finish
    B, L, pd = preds[0].shape
    xd = x.to(dev)
    # only cnt needs zeroing: the sums start as NaN
    recon_sum = torch.full(x.shape, float("nan"), dtype=torch.float32, device=dev)
    err_sum = torch.full((B, L), float("nan"), dtype=torch.float32, device=dev)
    cnt = torch.zeros(B, L, dtype=torch.int32, device=dev)
    for pred, mask in zip(preds, masks):
        if has_cls:  # the plan's layout [B (L + 1), pd]; the class rows must never be read
            full = torch.full((B, L + 1, pd), float("nan"), dtype=pred.dtype)
            full[:, 1:] = pred
            pred = full.view(B * (L + 1), pd)
        recon_accum(pred.contiguous().to(dev), has_cls, xd, mask.to(dev), cfg.patch_size, cfg.norm_pix_loss, recon_sum, err_sum, cnt)
    recon, err, vol = recon_finish(recon_sum, err_sum, cnt, xd, cfg.patch_size, error_volume=True, inplace=inplace)
    torch.cuda.synchronize()
    return recon.cpu(), err.cpu(), cnt.cpu(), vol.cpu()


@pytest.mark.parametrize("norm_pix", [False, True])
@pytest.mark.parametrize("pred_dtype,has_cls", [(torch.bfloat16, True), (torch.float32, False)])
@pytest.mark.parametrize("S,P,C,x_dtype", [(8, 4, 1, torch.float32), (8, 4, 3, torch.float32), (16, 8, 1, torch.float16), (24, 12, 3, torch.float32)])
def test_kernels_against_reference(lib, cuda, S, P, C, x_dtype, pred_dtype, has_cls, norm_pix):
    """(8, 4, 1): pd = 64, fewer quads than threads; (8, 4, 3): channel interleave; (16, 8, 1): fp16 volume; (24, 12, 3): pd = 5184,
    432 quads = 1.7 passes of the block."""
    cfg, x, preds, masks = _kernel_inputs(S, P, C, x_dtype, pred_dtype, norm_pix)
    st = RF.State(cfg, x.shape[0])
    for pred, mask in zip(preds, masks):
        RF.accumulate(cfg, st, pred, x, mask)
    w_recon, w_err, w_cnt, w_vol = RF.finish(cfg, st, x)
    recon, err, cnt, vol = _run_kernels(cfg, x, preds, masks, has_cls, cuda, inplace=False)
    figures = {"recon": rel_err(recon, w_recon), "err": rel_err(err, w_err), "err_vol": rel_err(vol, w_vol)}
    print(f"recon kernels S={S} P={P} C={C} x={x_dtype} pred={pred_dtype} norm_pix={norm_pix}: {figures}")
    assert recon.dtype == torch.float32 and bool(torch.isfinite(recon).all()) and bool(torch.isfinite(err).all())
    assert torch.equal(cnt.to(torch.int64), w_cnt) and int(cnt.max()) == 2 and int(cnt.min()) == 0
    for key, value in figures.items():
        assert value <= FP32_BAR, (key, value)
    # patches kept in both calls: the scan itself, bit for bit, and no error
    kept = w_cnt == 0
    assert int(kept.sum()) >= 2 * x.shape[0]
    assert torch.equal(O.patchify(cfg, recon)[kept], O.patchify(cfg, x.float())[kept])
    assert bool((err[kept] == 0).all())
    # a second identical sequence (this one finishing in place, over recon_sum) is bit-identical
    again = _run_kernels(cfg, x, preds, masks, has_cls, cuda, inplace=True)
    for a, b in zip((recon, err, cnt, vol), again):
        assert torch.equal(a, b)


def test_kernels_refuse_bad_geometry_by_name(lib, cuda):
    from headct_foundation_amd import HctError
    from headct_foundation_amd.reconstruct import recon_accum, recon_finish
    for S, P, what in ((12, 6, "P % 4"), (10, 4, "S % P")):
        x = torch.zeros(1, 1, S, S, S, device=cuda)
        L = 8
        args = (torch.zeros(L, P ** 3, device=cuda), False, x, torch.ones(1, L, device=cuda), P, False, torch.zeros_like(x),
                torch.zeros(1, L, device=cuda), torch.zeros(1, L, dtype=torch.int32, device=cuda))
        with pytest.raises(HctError, match="hct_mae_recon_accum.*" + what):
            recon_accum(*args)
        with pytest.raises(HctError, match="hct_mae_recon_finish"):
            recon_finish(args[6], args[7], args[8], x, P)
    x = torch.zeros(1, 1, 8, 8, 8, device=cuda)
    with pytest.raises(HctError, match="16-byte aligned"):  # a misaligned prediction is refused, not read
        recon_accum(torch.zeros(8 * 64 + 4, device=cuda)[1:1 + 8 * 64].view(8, 64), False, x, torch.ones(1, 8, device=cuda), 4, False, torch.zeros_like(x),
                    torch.zeros(1, 8, device=cuda), torch.zeros(1, 8, dtype=torch.int32, device=cuda))
    torch.cuda.synchronize()


# ---- end to end ----------------------------------------------------------------------------------------------------------------
def _check_against(rec, ref, cfg, bar, tag):
    B = rec.recon.shape[0]
    assert torch.equal(rec.masks.cpu(), ref["masks"]), tag
    assert torch.equal(rec.count.cpu().to(torch.int64), ref["count"]), tag
    assert rec.recon.dtype == torch.float32 and rec.error.dtype == torch.float32 and rec.count.dtype == torch.int32 and rec.masks.dtype == torch.uint8
    assert tuple(rec.error.shape) == (B, cfg.grid, cfg.grid, cfg.grid) and tuple(rec.recon.shape) == (B, cfg.in_chans) + (cfg.input_size,) * 3
    figures = {"recon": rel_err(rec.recon, ref["recon"]), "error": rel_err(rec.error, ref["error"]), "loss": rel_err(rec.loss, ref["loss"])}
    if rec.error_volume is not None:
        figures["error_volume"] = rel_err(rec.error_volume, ref["error_volume"])
    print(f"reconstruct {tag}: {figures}")
    for key, value in figures.items():
        assert value <= bar, (tag, key, value)


@pytest.mark.parametrize("name,passes", [("micro", 1), ("micro", None), ("micro", 4), ("yaml_cut", None)])
def test_reconstruct_fp32_vs_oracle(lib, cuda, name, passes):
    """`micro`; `yaml_cut`: three channels, patch 12, norm_pix_loss, qkv bias.  Masks are the schedule's, counts exact, recon / error at
    the fp32 bar, and for every pass the masked mean of the kernel's per-patch terms is the forward's own loss (hct_masked_mse)."""
    from headct_foundation_amd.reconstruct import cover_masks, cover_noise, cover_slots, recon_accum
    cfg = O.CONFIGS[name]
    B, L, K, seed = 2, cfg.num_patches, cfg.len_keep, 3
    params = O.make_params(cfg, 1)
    x = O.make_volume(cfg, B, 1).float()
    model = build_hip_model(cfg, params, cuda, "fp32", full_pred=False).eval()
    rec = model.reconstruct(x.to(cuda), passes=passes, seed=seed, error_volume=True)
    ref = RF.reconstruct(cfg, RF.oracle_predictor(params), x, passes=passes, seed=seed)
    n = ref["masks"].shape[0]
    assert n == (RF.cover_passes(L, K) if passes is None else passes) and tuple(rec.loss.shape) == (n,)
    assert torch.equal(rec.masks.cpu(), RF.window_masks(RF.slots(B, L, seed), n, K))
    assert torch.equal(rec.masks.cpu(), cover_masks(cover_slots(B, L, seed), n, K))
    _check_against(rec, ref, cfg, FP32_BAR, f"{name} passes={passes}")
    if passes != 1:
        assert int(rec.count.min()) >= 1
    # per pass: sum over the masked patches of e / (B M) against the forward's loss
    slot = cover_slots(B, L, seed, cuda)
    xd = x.to(cuda)
    for p in range(n):
        with torch.no_grad():
            loss, _, _ = model(xd, noise=cover_noise(slot, p, n, K))
        scratch = torch.empty_like(xd)
        e = torch.empty(B, L, device=cuda)
        cnt = torch.zeros(B, L, dtype=torch.int32, device=cuda)
        mask = model.activation("mask", B)
        recon_accum(model.activation("pred_full", B), True, xd, mask, cfg.patch_size, cfg.norm_pix_loss, scratch, e, cnt)
        masked = mask.view(B, L) != 0
        assert torch.equal(cnt.view(B, L) == 1, masked)
        mean_e = float(e[masked].double().sum() / (B * (L - K)))
        print(f"{name} pass {p}: masked mean of e {mean_e:.9f}, forward loss {float(loss):.9f}, reconstruct loss {float(rec.loss[p]):.9f}")
        assert abs(mean_e - float(loss)) <= 1e-5 * abs(float(loss))
        assert abs(float(rec.loss[p]) - float(loss)) <= 1e-5 * abs(float(loss))


def test_reconstruct_one_pass_with_explicit_noise(lib, cuda):
    cfg = O.CONFIGS["micro"]
    params = O.make_params(cfg, 0)
    x, noise = O.make_volume(cfg, 2, 0).float(), O.make_noise(cfg, 2, 0)
    model = build_hip_model(cfg, params, cuda, "fp32", full_pred=False)
    rec = model.reconstruct(x.to(cuda), passes=1, noise=noise.to(cuda))
    ref = RF.reconstruct(cfg, RF.oracle_predictor(params), x, passes=1, noise=noise)
    _check_against(rec, ref, cfg, FP32_BAR, "micro explicit noise")
    kept = (rec.count.cpu() == 0).view(2, -1)
    assert int(kept.sum()) == 2 * cfg.len_keep
    assert torch.equal(O.patchify(cfg, rec.recon.cpu())[kept], O.patchify(cfg, x)[kept])
    with pytest.raises(ValueError):
        model.reconstruct(x.to(cuda), passes=4, noise=noise.to(cuda))
    loose = dataclasses.replace(cfg, mask_ratio=0.4)  # K = 38, M = 26: covering takes 3 passes
    with pytest.raises(ValueError, match="passes = 2.*cover_passes = 3"):
        build_hip_model(loose, params, cuda, "fp32").reconstruct(x.to(cuda), passes=2)


def test_reconstruct_bf16_vs_emulating_oracle(lib, cuda):
    """`tiny` in bf16 against the oracle with the HIP path's roundings: the project's bf16 prediction bar for recon and error."""
    cfg = O.CONFIGS["tiny"]
    params = O.make_params(cfg, 0)
    x = O.make_volume(cfg, 2, 0).float()
    model = build_hip_model(cfg, params, cuda, "bf16", full_pred=False)
    rec = model.reconstruct(x.to(cuda), seed=1)
    ref = RF.reconstruct(cfg, RF.oracle_predictor(params, emulate_bf16=True), x, seed=1)
    _check_against(rec, ref, cfg, BF16_BAR, "tiny bf16")


@pytest.mark.parametrize("name,dtype", [("micro", "fp32"), ("yaml_cut", "bf16")])
def test_fp16_volume_equals_its_fp32_upcast(lib, cuda, name, dtype):
    cfg = O.CONFIGS[name]
    model = build_hip_model(cfg, O.make_params(cfg, 0), cuda, dtype, full_pred=False)
    x16 = O.make_volume(cfg, 2, 0).to(torch.float16).to(cuda)
    a = model.reconstruct(x16, seed=4, error_volume=True)
    b = model.reconstruct(x16.float(), seed=4, error_volume=True)
    for key in ("recon", "error", "count", "loss", "masks", "error_volume"):
        assert torch.equal(getattr(a, key), getattr(b, key)), key


def test_reconstruct_leaves_the_training_state_alone(lib, cuda):
    """`training`, every `.grad`, the flat buffers: unchanged by the call; the training step that follows gives the loss and the
    gradients of a twin that never called it."""
    cfg = O.CONFIGS["micro"]
    params = O.make_params(cfg, 0)
    x = O.make_volume(cfg, 2, 0).float().to(cuda)
    n0, n1 = O.make_noise(cfg, 2, 0).to(cuda), O.make_noise(cfg, 2, 1).to(cuda)
    out = {}
    for key in ("plain", "with_call"):
        model = build_hip_model(cfg, params, cuda, "fp32", full_pred=False)
        model.train()
        model(x, noise=n0)[0].backward()
        if key == "with_call":
            before = grads_by_name(model)
            flat, flat_grad = model._flat.clone(), model._flat_grad.clone()
            model.reconstruct(x, passes=4)
            assert model.training
            after = grads_by_name(model)
            assert set(before) == set(after) and all(torch.equal(before[k], after[k]) for k in before)
            assert torch.equal(flat, model._flat) and torch.equal(flat_grad, model._flat_grad)
            model.eval()
            model.reconstruct(x, passes=1)
            assert not model.training
            model.train()
        model.zero_grad(set_to_none=True)
        loss = model(x, noise=n1)[0]
        loss.backward()
        torch.cuda.synchronize()
        out[key] = (float(loss.detach()), grads_by_name(model))
    assert out["plain"][0] == out["with_call"][0]
    assert all(torch.equal(out["plain"][1][k], out["with_call"][1][k]) for k in out["plain"][1])


# ---- plumbing run --------------------------------------------------------------------------------------------------------
def test_main_reconstruct_plumbing_run(lib, cuda, tmp_path):
    """main_reconstruct.py as a subprocess: synthetic data, the `micro` geometry, a checkpoint saved here in the reference's layout."""
    from headct_foundation_amd.data import SyntheticVolumes
    from headct_foundation_amd.nifti import read_nifti
    cfg = O.CONFIGS["micro"]
    params = O.make_params(cfg, 2)
    torch.save({"state_dict": {"module." + k: v for k, v in params.items()}, "epoch": 7}, tmp_path / "mae.pt")
    yaml = tmp_path / "cfg.yaml"
    yaml.write_text("MODEL:\n  NAME: mae\n")
    out = tmp_path / "out"
    opts = ["DATA.SYNTHETIC", "True", "DATA.SYNTHETIC_SAMPLES", "4", "MAE.INPUT_SIZE", "32", "MAE.PATCH_SIZE", "8", "MAE.IN_CHANS", "1",
            "MAE.ENCODER_DEPTH", "2", "MAE.ENCODER_EMBED_DIM", "48", "MAE.ENCODER_MLP_DIM", "96", "MAE.ENCODER_NUM_HEADS", "3", "MAE.DECODER_DEPTH", "1",
            "MAE.DECODER_EMBED_DIM", "48", "MAE.DECODER_MLP_DIM", "96", "MAE.DECODER_NUM_HEADS", "3", "MAE.USE_BIAS", "True", "MAE.COMPUTE_DTYPE", "fp32",
            "LOG.OUTPUT_DIR", str(tmp_path / "log")]
    cmd = [sys.executable, os.path.join(ROOT, "main_reconstruct.py"), "--cfg", str(yaml), "--model_name", "mae", "--model_load_path", str(tmp_path / "mae.pt"),
           "--batch_size", "2", "--seed", "11", "--passes", "4", "--nifti", "--max_scans", "2", "--save_dir", str(out), "--opts"] + opts
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-4000:]
    rows = list(csv.reader(open(out / "scores.csv")))
    assert rows[0] == ["name", "score_mean", "score_max"] + [f"loss_pass{p}" for p in range(4)] and len(rows) == 1 + 2
    maps = np.load(out / "error_maps.npy")
    assert maps.shape == (2, 4, 4, 4) and maps.dtype == np.float32
    summary = json.load(open(out / "reconstruct.json"))
    assert summary["passes"] == 4 and summary["cover_passes"] == 2 and summary["mask_ratio"] == 0.75 and summary["n_scans"] == 2
    # the same model on the same volumes and seed, in this process
    model = build_hip_model(cfg, params, cuda, "fp32", full_pred=False).eval()
    data = next(iter(SyntheticVolumes(1, 2, 1, 32, cuda, 11)))
    rec = model.reconstruct(data, passes=4, seed=11, error_volume=True)
    assert abs(summary["mean_loss"] - float(rec.loss.mean())) <= 1e-6 * float(rec.loss.mean())
    assert np.array_equal(maps, rec.error.cpu().numpy())
    for b, row in enumerate(rows[1:]):
        stem = row[0]
        for kind, want in (("input", data[b, 0]), ("recon", rec.recon[b, 0]), ("error", rec.error_volume[b])):
            raw, slope, _, affine = read_nifti(out / f"{stem}_{kind}.nii.gz")
            assert slope is None and np.array_equal(affine, np.eye(4))
            assert raw.dtype == np.float32 and np.array_equal(raw, want.cpu().numpy()), (stem, kind)
        assert abs(float(row[1]) - float(rec.error[b].mean())) <= 1e-6 * float(rec.error[b].mean())
        assert abs(float(row[2]) - float(rec.error[b].max())) <= 1e-6 * float(rec.error[b].max())
