"""Host side of the MAE reconstruction path: the mask schedule, the float64 yardstick's own sanity, the NIfTI writer, the entry point's
flags (no GPU)."""
import logging
import os
import re
import types

import numpy as np
import pytest
import torch

from oracle import mae_oracle as O
from tests import reconstruct_ref as RF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID_L = (8, 27, 64, 125, 216, 512)


def test_new_symbols_are_exported_declared_and_host_checked(lib):
    import headct_foundation_amd as pkg
    from headct_foundation_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "headct_hip.h")).read()
    for s in ("hct_mae_recon_accum", "hct_mae_recon_finish"):
        assert re.search(r"\b" + s + r"\s*\(", hdr) and s in _lib.exported_symbols() and hasattr(lib, s), s
    assert "reconstruct.hip" in build.SOURCES
    for s in ("Reconstruction", "anomaly_score", "cover_passes", "write_nifti"):
        assert hasattr(pkg, s), s
    assert hasattr(pkg.MaskedAutoencoderViT, "reconstruct")
    # geometry violations come back as HCT_E_BADARG, by name, before any launch
    for S, P, C, what in ((8, 3, 4, b"P % 4"), (10, 4, 1, b"S % P"), (8, 4, 1, None)):
        rc = lib.hct_mae_recon_accum(None, _lib.HCT_F32, 0, None, _lib.HCT_F32, None, 1, C, S, P, 0, None, None, None, None)
        assert rc == -1 and b"hct_mae_recon_accum" in lib.hct_last_error_string()
        assert what is None or what in lib.hct_last_error_string()
    assert lib.hct_mae_recon_accum(None, _lib.HCT_F32, 0, None, _lib.HCT_BF16, None, 1, 1, 8, 4, 0, None, None, None, None) == -1
    assert b"fp32 or fp16" in lib.hct_last_error_string()
    assert lib.hct_mae_recon_finish(None, None, None, None, _lib.HCT_F32, 1, 1, 8, 3, None, None, None, None) == -1
    assert b"hct_mae_recon_finish" in lib.hct_last_error_string()


# ---- schedule --------------------------------------------------------------------------------------------------------------------
def _keeps(L):
    return range(L) if L <= 64 else sorted(set(range(0, L, 11)) | {1, L // 4, L // 2, L - 2, L - 1})


@pytest.mark.parametrize("L", GRID_L)
def test_schedule_masks_windows_and_cover_condition(L):
    """Every pass masks exactly M patches; the masks the model's rank order derives from `cover_noise` are the ring windows; the
    windows cover every patch iff n >= cover_passes = ceil(L / M)."""
    from headct_foundation_amd.reconstruct import cover_masks, cover_noise, cover_passes, cover_slots
    B = 2
    for K in _keeps(L):
        M = L - K
        need = cover_passes(L, K)
        assert need == RF.cover_passes(L, K) == -(-L // M)
        cfg = types.SimpleNamespace(len_keep=K)  # all that random_masking_from_noise reads
        slot = cover_slots(B, L, seed=3)
        assert torch.equal(slot, RF.slots(B, L, 3)) and torch.equal(torch.sort(slot, dim=1).values, torch.arange(L).expand(B, L))
        for n in sorted({1, need - 1, need, need + 1, 2 * need + 1} - {0}):
            want = RF.window_masks(slot, n, K) if L <= 64 else None
            got = cover_masks(slot, n, K)
            seen = torch.zeros(B, L, dtype=torch.int64)
            for p in range(n):
                noise = cover_noise(slot, p, n, K)
                assert noise.dtype == torch.float32 and torch.equal(noise, RF.noise_of(slot, p, n, K))
                assert torch.equal(torch.sort(noise, dim=1).values, torch.arange(L, dtype=torch.float32).expand(B, L))  # distinct integers
                mask = O.random_masking_from_noise(cfg, noise)[3]
                assert int(mask.sum()) == B * M
                assert torch.equal(mask.to(torch.uint8), got[p])
                if want is not None:
                    assert torch.equal(got[p], want[p])
                seen += mask.to(torch.int64)
            assert bool((seen > 0).all()) == (n >= need), (L, K, n)


def test_schedule_through_the_oracles_masking():
    """`oracle.random_masking_from_noise` itself on the geometries the end-to-end tests use (L = 64, K = 16)."""
    from headct_foundation_amd.reconstruct import cover_noise, cover_slots
    cfg = O.CONFIGS["micro"]
    L, K = cfg.num_patches, cfg.len_keep
    slot = cover_slots(3, L, seed=0)
    for n in (1, 2, 4):
        want = RF.window_masks(slot, n, K)
        for p in range(n):
            mask = O.random_masking_from_noise(cfg, cover_noise(slot, p, n, K))[3]
            assert torch.equal(mask.to(torch.uint8), want[p])


def test_counts_of_the_worked_examples():
    from headct_foundation_amd.reconstruct import cover_masks, cover_passes, cover_slots
    slot = cover_slots(2, 216, seed=1)
    assert cover_passes(216, 54) == 2
    assert bool((cover_masks(slot, 4, 54).sum(dim=0) == 3).all())
    two = cover_masks(slot, 2, 54).sum(dim=0)
    assert int(two.min()) == 1 and int(two.max()) == 2


def test_refused_passes_raise():
    from headct_foundation_amd.reconstruct import cover_passes, resolve_passes
    assert cover_passes(216, 198) == 12
    assert resolve_passes(216, 198, None) == 12 and resolve_passes(216, 198, 1) == 1 and resolve_passes(216, 198, 12) == 12
    assert resolve_passes(216, 198, 40) == 40
    for bad in (2, 11):
        with pytest.raises(ValueError, match=rf"{bad}.*12"):
            resolve_passes(216, 198, bad)
    with pytest.raises(ValueError):
        resolve_passes(216, 198, 0)
    with pytest.raises(ValueError):  # mask_ratio so small that no patch is masked
        cover_passes(64, 64)
    with pytest.raises(ValueError):
        resolve_passes(64, 64, None)


def test_anomaly_score():
    from headct_foundation_amd.reconstruct import anomaly_score
    err = torch.tensor([[1.0, 5.0, 3.0, 9.0], [2.0, 2.0, 7.0, 4.0], [1.0, 1.0, 1.0, 1.0]]).view(3, 1, 2, 2)
    cnt = torch.tensor([[1, 2, 1, 0], [0, 0, 3, 1], [0, 0, 0, 0]], dtype=torch.int32).view(3, 1, 2, 2)
    assert torch.equal(anomaly_score(err, cnt, "mean"), torch.tensor([3.0, 5.5, 0.0]))
    assert torch.equal(anomaly_score(err, cnt, "max"), torch.tensor([5.0, 7.0, 0.0]))
    with pytest.raises(ValueError):
        anomaly_score(err, cnt, "median")


# ---- the yardstick's own sanity -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["micro", "yaml_cut"])
def test_reference_perfect_predictor_gives_the_scan_back(name):
    """pred := target: recon == x to 1e-6 and the error vanishes (this pins the de-normalisation of norm_pix_loss); with one pass the
    kept patches of recon are the scan bit for bit."""
    cfg = O.CONFIGS[name]
    x = O.make_volume(cfg, 2, 1)
    for passes in (None, 4):
        r = RF.reconstruct(cfg, RF.perfect_predictor, x, passes=passes, seed=2)
        assert float((r["recon"] - x.double()).abs().max()) < 1e-6
        assert float(r["error"].abs().max()) < 1e-12 and int(r["count"].min()) >= 1
    r = RF.reconstruct(cfg, RF.perfect_predictor, x, passes=1, seed=2)
    assert float((r["recon"] - x.double()).abs().max()) < 1e-6
    assert int(r["count"].max()) == 1 and int(r["count"].sum()) == 2 * (cfg.num_patches - cfg.len_keep)


@pytest.mark.parametrize("name", ["micro", "yaml_cut"])
def test_reference_one_pass_keeps_unmasked_patches(name):
    cfg = O.CONFIGS[name]
    params = O.make_params(cfg, 0)
    x = O.make_volume(cfg, 2, 0)
    r = RF.reconstruct(cfg, RF.oracle_predictor(params), x, passes=1, seed=5)
    kept = (r["count"] == 0).view(2, cfg.num_patches)
    assert int(kept.sum()) == 2 * cfg.len_keep
    got, want = O.patchify(cfg, r["recon"]), O.patchify(cfg, x.double())
    assert torch.equal(got[kept], want[kept])           # bit-equal where nothing was predicted
    assert not torch.equal(got[~kept], want[~kept])
    assert bool((r["error"].view(2, -1)[kept] == 0).all()) and bool((r["error"].view(2, -1)[~kept] > 0).all())
    # the masked mean of the per-patch terms is the forward's own loss
    m = r["masks"][0].double()
    assert abs(float((r["patch_err"][0] * m).sum() / m.sum()) - float(r["loss"][0])) < 1e-12
    # error_volume: every voxel of a patch carries the patch's error
    one = RF.geometry(cfg.input_size, cfg.patch_size, 1)
    assert torch.equal(O.patchify(one, r["error_volume"].unsqueeze(1))[:, :, 0], r["error"].view(2, -1))


# ---- NIfTI writer ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ext", [".nii", ".nii.gz"])
@pytest.mark.parametrize("dtype", ["f4", "i2"])
def test_write_nifti_round_trip(tmp_path, ext, dtype):
    from headct_foundation_amd.nifti import read_nifti, write_nifti
    rng = np.random.RandomState(3)
    shape = (5, 7, 11)  # [nk, nj, ni], non-cubic
    a = rng.standard_normal(shape).astype(np.float32) if dtype == "f4" else rng.randint(-2000, 3000, size=shape).astype(np.int16)
    affine = np.array([[0.0, -0.5, 0.0, 12.5], [0.75, 0.0, 0.0, -30.0], [0.0, 0.0, 2.5, 7.25], [0.0, 0.0, 0.0, 1.0]])
    path = tmp_path / ("v" + ext)
    write_nifti(path, a, affine, dtype=dtype)
    raw, slope, inter, aff = read_nifti(path)
    assert raw.dtype == a.dtype and raw.shape == shape and raw.tobytes() == a.tobytes()
    assert slope is None and inter is None  # scl_slope 0: the stored values are the values
    assert np.array_equal(aff, affine)
    write_nifti(path, a, dtype=dtype)
    assert np.array_equal(read_nifti(path)[3], np.eye(4))
    with pytest.raises(ValueError):
        write_nifti(path, a[0], dtype=dtype)
    with pytest.raises(ValueError):
        write_nifti(path, a, dtype="f8")
    if dtype == "i2":
        with pytest.raises(ValueError):
            write_nifti(path, a.astype(np.float32) + 0.5, dtype="i2")


# ---- entry point -----------------------------------------------------------------------------------------------------------------
def test_main_reconstruct_parses_its_flags_and_needs_a_gpu(tmp_path, monkeypatch):
    import main_reconstruct as M
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("MODEL:\n  NAME: mae\n")
    args, config = M.parse_option(["--cfg", str(cfg), "--model_name", "mae", "--model_load_path", "m.pt", "--save_dir", str(tmp_path / "out"),
                                   "--passes", "4", "--max_scans", "2", "--label_name", "ICH", "--nifti", "--test_csv_path", "t.csv",
                                   "--batch_size", "3", "--opts", "MAE.MASK_RATIO", "0.5"])
    assert args.passes == 4 and args.max_scans == 2 and args.nifti and args.save_dir == str(tmp_path / "out") and args.label_name == "ICH"
    assert config.MODEL.PRETRAINED == "m.pt" and config.DATA.TEST_CSV_PATH == "t.csv" and config.DATA.BATCH_SIZE == 3
    assert config.TRAIN.LABEL_NAME == "ICH" and config.MAE.MASK_RATIO == 0.5 and config.MODEL.NAME == "mae"
    args, config = M.parse_option(["--cfg", str(cfg)])
    assert args.passes is None and args.max_scans == 0 and not args.nifti and not args.label_name
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SystemExit, match="needs an MI355X"):
        M.main(config, args, logging.getLogger("test_reconstruct"))


def test_reconstruct_refuses_the_cpu():
    from headct_foundation_amd import HctError
    from headct_foundation_amd.reconstruct import recon_accum, recon_finish, reconstruct
    z = torch.zeros(1, 1, 8, 8, 8)
    with pytest.raises(HctError):
        recon_accum(torch.zeros(8, 64), False, z, torch.zeros(1, 8), 4, False, z.clone(), torch.zeros(1, 8), torch.zeros(1, 8, dtype=torch.int32))
    with pytest.raises(HctError):
        recon_finish(z.clone(), torch.zeros(1, 8), torch.zeros(1, 8, dtype=torch.int32), z, 4)

    class _M:
        num_patches, len_keep = 8, 2
    with pytest.raises(HctError):
        reconstruct(_M(), z)
