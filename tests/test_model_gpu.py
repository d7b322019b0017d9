"""Whole-model parity on the GPU: HIP path (through the C ABI driver) vs. the CPU oracle and the golden
fixtures generated from the reference.  Tolerances: fp32 mode 1e-3 relative (north_star) -- in practice
~1e-5; bf16 mode (bf16 storage + MFMA, fp32 accumulate) is checked at the looser tolerance written per test."""
import numpy as np
import pytest
import torch

from oracle import mae_oracle as O
from tests.util import build_hip_model, grads_by_name, load_golden, rel_err, sample_of

pytestmark = pytest.mark.gpu

CASES = [("micro", 2, 0), ("yaml_cut", 2, 1), ("tiny", 2, 0), ("vitb_cut", 2, 0)]


def _run_hip(cfg, params, x, noise, device, dtype):
    model = build_hip_model(cfg, params, device, dtype)
    model.train()
    loss, a, b = model(x.to(device), noise=noise.to(device))
    assert a is None and b is None
    loss.backward()
    torch.cuda.synchronize()
    return model, float(loss.detach())


@pytest.mark.parametrize("name,batch,seed", CASES)
def test_fp32_forward_backward_vs_oracle(lib, cuda, name, batch, seed):
    cfg = O.CONFIGS[name]
    params = O.make_params(cfg, seed)
    x, noise = O.make_volume(cfg, batch, seed), O.make_noise(cfg, batch, seed)
    o_loss, o_pred, o_mask, o_grads, o_inter = O.forward_backward(cfg, params, x, noise, want_inter=True)
    model, loss = _run_hip(cfg, params, x, noise, cuda, "fp32")
    tol = 1e-3  # north_star: 1e-3 relative fp32
    assert abs(loss - float(o_loss)) / abs(float(o_loss)) < tol
    assert torch.equal(model.last_mask(batch).cpu(), o_mask)
    assert torch.equal(model.activation("ids_restore", batch).cpu().long(), o_inter["ids_restore"])
    assert rel_err(model.last_pred(batch), o_pred) < tol
    assert rel_err(model.activation("latent", batch).float().view_as(o_inter["latent"]), o_inter["latent"]) < tol
    for key in ("enc_in", "dec_in"):
        assert rel_err(model.activation(key, batch).view_as(o_inter[key]), o_inter[key]) < tol, key
    for i in range(cfg.encoder_depth):
        assert rel_err(model.activation(f"enc{i}.out", batch).view_as(o_inter[f"enc{i}.out"]), o_inter[f"enc{i}.out"]) < tol
    for i in range(cfg.decoder_depth):
        assert rel_err(model.activation(f"dec{i}.out", batch).view_as(o_inter[f"dec{i}.out"]), o_inter[f"dec{i}.out"]) < tol
    grads = grads_by_name(model)
    assert set(grads) == set(o_grads)
    worst = max((rel_err(grads[k], o_grads[k]), k) for k in grads if not k.endswith("qkv.bias"))
    assert worst[0] < tol, worst
    for k in grads:
        if k.endswith("qkv.bias"):  # K-third has a mathematically zero gradient: compare absolutely
            assert (grads[k] - o_grads[k]).abs().max() < 1e-6 + 1e-3 * o_grads[k].abs().max(), k
    # reconstructed voxels
    vol = model.unpatchify(model.last_pred(batch).contiguous(), x.to(cuda))
    assert rel_err(vol, O.unpatchify(cfg, o_pred)) < tol


@pytest.mark.parametrize("name,batch,seed", CASES)
def test_fp32_vs_golden_reference_outputs(lib, cuda, name, batch, seed):
    """Against the committed outputs of the REFERENCE itself (tests/golden/make_golden.py)."""
    fx = load_golden(f"{name}_b{batch}_s{seed}")
    cfg = O.CONFIGS[name]
    params = O.make_params(cfg, seed)
    x, noise = O.make_volume(cfg, batch, seed), O.make_noise(cfg, batch, seed)
    model, loss = _run_hip(cfg, params, x, noise, cuda, "fp32")
    assert abs(loss - fx["loss"]) / abs(fx["loss"]) < 1e-3
    got, want, l2, l2w = sample_of(model.last_pred(batch), fx["pred"])
    assert abs(l2 - l2w) / l2w < 1e-3 and torch.allclose(got, want, rtol=1e-3, atol=1e-4 * float(want.abs().max()))
    grads = grads_by_name(model)
    for k, entry in fx["grads"].items():
        got, want, l2, l2w = sample_of(grads[k], entry)
        if k.endswith("qkv.bias"):
            assert (got - want).abs().max() < 1e-6 + 1e-3 * float(want.abs().max()), k
        else:
            assert abs(l2 - l2w) <= 1e-3 * l2w + 1e-9, k
            assert torch.allclose(got, want, rtol=2e-3, atol=2e-4 * float(want.abs().max()) + 1e-10), k


@pytest.mark.parametrize("name,batch,seed", CASES)
def test_bf16_forward_backward_vs_oracle(lib, cuda, name, batch, seed):
    """bf16 storage + MFMA (fp32 accumulate, fp32 residual stream / statistics / loss).
    Tolerances (documented): loss 5e-3 relative, pred 2e-2, gradients 6e-2 relative L2 per tensor."""
    cfg = O.CONFIGS[name]
    params = O.make_params(cfg, seed)
    x, noise = O.make_volume(cfg, batch, seed), O.make_noise(cfg, batch, seed)
    o_loss, o_pred, o_mask, o_grads, _ = O.forward_backward(cfg, params, x, noise)
    model, loss = _run_hip(cfg, params, x, noise, cuda, "bf16")
    assert abs(loss - float(o_loss)) / abs(float(o_loss)) < 5e-3
    assert torch.equal(model.last_mask(batch).cpu(), o_mask)
    assert rel_err(model.last_pred(batch), o_pred) < 2e-2
    grads = grads_by_name(model)
    assert set(grads) == set(o_grads)
    bad = [(rel_err(grads[k], o_grads[k]), k) for k in grads if not k.endswith("qkv.bias")]
    assert max(bad)[0] < 6e-2, sorted(bad)[-5:]
    for k in grads:
        if k.endswith("qkv.bias"):  # K-third has a mathematically zero gradient: compare absolutely, as the fp32 test does
            assert (grads[k] - o_grads[k]).abs().max() < 1e-6 + 6e-2 * o_grads[k].abs().max(), k


@pytest.mark.parametrize("name,batch,seed", CASES)
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_compact_decoder_tail_vs_full_and_oracle(lib, cuda, name, batch, seed, dtype):
    """The module's default training forward runs the decoder's tail (last block's proj / MLP, decoder_norm, decoder_pred, loss) on
    the masked patches' rows only -- the loss takes no other row, mae.py:298-299.  Loss and EVERY gradient must be those of the
    full computation (same kernels on a row subset: 1e-5 fp32; bf16 differs by summation order of the column sums only), and
    the masked rows of pred / of the last block's output must match the oracle's."""
    cfg = O.CONFIGS[name]
    params = O.make_params(cfg, seed)
    x, noise = O.make_volume(cfg, batch, seed), O.make_noise(cfg, batch, seed)
    full = build_hip_model(cfg, params, cuda, dtype, full_pred=True)
    tail = build_hip_model(cfg, params, cuda, dtype, full_pred=False)
    out = {}
    for key, m in (("full", full), ("tail", tail)):
        m.train()
        loss, _, _ = m(x.to(cuda), noise=noise.to(cuda))
        loss.backward()
        torch.cuda.synchronize()
        out[key] = (float(loss), grads_by_name(m))
    tol = 1e-5 if dtype == "fp32" else 2e-3
    assert abs(out["tail"][0] - out["full"][0]) <= tol * abs(out["full"][0])
    assert set(out["tail"][1]) == set(out["full"][1])
    for k, g in out["full"][1].items():
        if k.endswith("qkv.bias"):
            assert (out["tail"][1][k] - g).abs().max() <= 1e-6 + tol * g.abs().max(), k
        else:
            assert rel_err(out["tail"][1][k], g) < tol, k
    with pytest.raises(Exception):
        tail.last_pred(batch)  # no prediction exists for the kept patches
    # masked rows: identical row sets, and the values of the full run / the oracle
    rows_t, pred_t = tail.last_pred_masked(batch)
    rows_f, pred_f = full.last_pred_masked(batch)
    order_t, order_f = torch.argsort(rows_t), torch.argsort(rows_f)
    assert torch.equal(rows_t[order_t], rows_f[order_f])
    assert rel_err(pred_t[order_t], pred_f[order_f]) < (1e-5 if dtype == "fp32" else 1e-2)
    if dtype == "fp32":
        o_loss, o_pred, o_mask, o_grads, o_inter = O.forward_backward(cfg, params, x, noise, want_inter=True)
        L = tail.num_patches
        b, t = rows_t.cpu() // (L + 1), rows_t.cpu() % (L + 1)
        assert bool((t >= 1).all()) and bool((o_mask[b, t - 1] == 1).all()) and rows_t.numel() == int(o_mask.sum())
        assert rel_err(pred_t.cpu(), o_pred[b, t - 1]) < 1e-3
        last = o_inter[f"dec{cfg.decoder_depth - 1}.out"]
        got = tail.activation(f"dec{cfg.decoder_depth - 1}.out", batch)[:rows_t.numel()].cpu()
        assert rel_err(got, last.reshape(-1, last.shape[-1])[rows_t.cpu()]) < 1e-3
        assert abs(out["tail"][0] - float(o_loss)) / abs(float(o_loss)) < 1e-3
        worst = max((rel_err(out["tail"][1][k], o_grads[k]), k) for k in o_grads if not k.endswith("qkv.bias"))
        assert worst[0] < 1e-3, worst


@pytest.mark.parametrize("name,batch,seed", [("micro2", 2, 0), ("tiny", 3, 1), ("yaml_cut2", 2, 1)])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_first_decoder_block_on_cat_rows_vs_every_row(lib, cuda, name, batch, seed, dtype):
    """The masked tokens enter the decoder as mask_token + pos[l] in every volume (mae.py:259-265): the first decoder block's
    LayerNorm1 / qkv run on the kept + class rows and ONE table row per patch position, forward and backward (weight gradient, input
    gradient, LayerNorm backward, mask_token / decoder_cls_token gradients from the pieces).  Loss and every gradient must be those of
    the run that pushes every row through (`dec0_table = False`): 1e-5 fp32; bf16 rounds the per-position sums once more (3e-3)."""
    import dataclasses
    # (micro / yaml_cut with a second decoder block: qkv bias and norm_pix_loss on the path; the path needs two decoder blocks)
    cfg = dataclasses.replace(O.CONFIGS[name[:-1]], decoder_depth=2) if name.endswith("2") else O.CONFIGS[name]
    assert cfg.decoder_depth >= 2
    params = O.make_params(cfg, seed)
    x, noise = O.make_volume(cfg, batch, seed), O.make_noise(cfg, batch, seed)
    out = {}
    for key in ("rows", "cat"):
        m = build_hip_model(cfg, params, cuda, dtype, full_pred=False)
        m.dec0_table = key == "cat"
        m.train()
        loss, _, _ = m(x.to(cuda), noise=noise.to(cuda))
        loss.backward()
        torch.cuda.synchronize()
        out[key] = (float(loss), grads_by_name(m))
    tol = 1e-5 if dtype == "fp32" else 3e-3
    assert abs(out["cat"][0] - out["rows"][0]) <= tol * abs(out["rows"][0])
    assert set(out["cat"][1]) == set(out["rows"][1])
    for k, g in out["rows"][1].items():
        if k.endswith("qkv.bias"):
            assert (out["cat"][1][k] - g).abs().max() <= 1e-6 + tol * g.abs().max(), k
        else:
            assert rel_err(out["cat"][1][k], g) < tol, (k, rel_err(out["cat"][1][k], g))
    if dtype == "fp32":
        o_loss, _, _, o_grads, _ = O.forward_backward(cfg, params, x, noise)
        assert abs(out["cat"][0] - float(o_loss)) / abs(float(o_loss)) < 1e-3
        for k in ("mask_token", "decoder_cls_token", "decoder_blocks.0.attn.qkv.weight", "decoder_blocks.0.att_norm.weight", "decoder_embed.weight"):
            assert rel_err(out["cat"][1][k], o_grads[k]) < 1e-3, k


FROZEN_MAE = ("decoder_blocks.0.attn.qkv.weight",                                       # first decoder block: cat rows
              "decoder_blocks.1.mlp.linear2.weight",                                    # every row
              "decoder_blocks.2.mlp.linear1.weight", "decoder_blocks.2.attn.proj.weight",  # compact tail
              "decoder_pred.weight", "decoder_embed.weight", "patch_embedding.patch_embeddings.weight",
              "patch_embedding.patch_embeddings.bias", "cls_token", "mask_token")


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_frozen_mae_parameters_are_skipped(lib, cuda, dtype):
    """A frozen parameter of an MAE model has no gradient, whichever row form its block runs in: `.grad` None and a zero slice of the
    flat gradient (so norms over the flat buffer are norms of the trainable gradients), while loss and every trainable gradient are
    those of the all-trainable step.  fp32: bit for bit (no product's arithmetic depends on another's being skipped).  bf16: the grouped
    weight-gradient launch's job table changes when jobs leave it, so two forms of the same step are compared, at the tolerance
    test_compact_decoder_tail_vs_full_and_oracle compares two forms with (2e-3)."""
    import dataclasses
    cfg = dataclasses.replace(O.CONFIGS["micro"], decoder_depth=3)
    batch = 2
    params = O.make_params(cfg, 0)
    x, noise = O.make_volume(cfg, batch, 0), O.make_noise(cfg, batch, 0)
    out = {}
    for key in ("all", "frozen"):
        m = build_hip_model(cfg, params, cuda, dtype, full_pred=False)
        m.dec0_table = True
        named = dict(m.named_parameters())
        if key == "frozen":
            for n in FROZEN_MAE:
                named[n].requires_grad_(False)
        m.train()
        loss, _, _ = m(x.to(cuda), noise=noise.to(cuda))
        loss.backward()
        torch.cuda.synchronize()
        out[key] = (float(loss), grads_by_name(m))
        if key == "frozen":
            for n in FROZEN_MAE:
                assert named[n].grad is None, n
                assert not bool(m._grad_view(n).any()), (n, float(m._grad_view(n).abs().max()))
    assert set(out["frozen"][1]) == set(out["all"][1]) - set(FROZEN_MAE)
    if dtype == "fp32":
        assert out["frozen"][0] == out["all"][0]
        for k, g in out["frozen"][1].items():
            assert torch.equal(g, out["all"][1][k]), k
        return
    tol = 2e-3
    assert abs(out["frozen"][0] - out["all"][0]) <= tol * abs(out["all"][0])
    for k, g in out["frozen"][1].items():
        want = out["all"][1][k]
        if k.endswith("qkv.bias"):
            assert (g - want).abs().max() <= 1e-6 + tol * want.abs().max(), k
        else:
            assert rel_err(g, want) < tol, (k, rel_err(g, want))


def test_train_curve_fp32_vs_golden(lib, cuda):
    """N-step loss curve, LR values and parameters after training vs the reference's own train_one_epoch."""
    from headct_foundation_amd.optim import HipAdamW, clip_gradients
    from headct_foundation_amd.lr_sched import get_cosine_schedule_with_warmup
    for name, batch, seed in (("micro", 2, 0), ("tiny", 2, 0)):
        fx = load_golden(f"{name}_b{batch}_s{seed}")
        hp = fx["train"]["hp"]
        cfg = O.CONFIGS[name]
        model = build_hip_model(cfg, O.make_params(cfg, seed), cuda, "fp32")
        opt = HipAdamW(model, lr=hp["base_lr"], weight_decay=hp["weight_decay"], betas=(hp["beta1"], hp["beta2"]))
        sched = get_cosine_schedule_with_warmup(opt, hp["warmup"], hp["total"], lr_end=hp["min_lr"])
        losses, lrs = [], []
        for i in range(fx["train"]["steps"]):
            opt.zero_grad()
            x = O.make_volume(cfg, batch, seed + 10 + i).to(cuda)
            noise = O.make_noise(cfg, batch, seed + 10 + i).to(cuda)
            loss, _, _ = model(x, noise=noise)
            loss.backward()
            clip_gradients(model, hp["grad_clip"])
            lrs.append(opt.param_groups[0]["lr"])
            opt.step()
            sched.step()
            losses.append(float(loss))
        assert np.allclose(lrs, fx["train"]["lrs"], rtol=1e-9)
        assert np.allclose(losses, fx["train"]["logged_losses"], atol=2e-4), (losses, fx["train"]["logged_losses"])
        named = dict(model.named_parameters())
        for k, entry in fx["train"]["params_after"].items():
            got, want, l2, l2w = sample_of(named[k], entry)
            atol = 4 * hp["base_lr"] if k.endswith("qkv.bias") else 1e-5
            assert torch.allclose(got, want, rtol=1e-4, atol=atol), k


@pytest.mark.parametrize("dtype,tol", [("fp32", 1e-3), ("bf16", 2e-2)])
def test_vit_feature_extraction_vs_oracle_and_reference_fixture(lib, cuda, dtype, tol):
    """HIP ViT (forward only, register tokens, final LN eps 1e-6) vs the oracle and the reference-generated fixture."""
    import json, os
    from headct_foundation_amd import ViT
    fx = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "vit_features.json")))
    ctor = dict(fx["ctor"])
    params = O.make_vit_params({k: v["shape"] for k, v in fx["state_dict"].items()})
    x = torch.from_numpy(O.hash_uniform(2 * 32 ** 3, 7).reshape(2, 1, 32, 32, 32).astype(np.float32)) * 0.5 + 0.5
    model = ViT(**ctor, compute_dtype=dtype)
    assert list(model.state_dict().keys()) == list(fx["state_dict"].keys())  # names and registration order of vit.py:100-130
    model.load_state_dict(params, strict=True)
    model = model.to(cuda)
    out, hidden = model(x.to(cuda))
    o_out, o_hidden = O.vit_forward(params, x, 16, 3, 2)
    assert rel_err(out, o_out) < tol
    for a, b in zip(hidden, o_hidden):
        assert rel_err(a, b) < tol
    if dtype == "fp32":
        for t, entry in [(out, fx["out"])] + list(zip(hidden, fx["hidden"])):
            got, want, l2, l2w = sample_of(t, entry)
            assert torch.allclose(got, want, rtol=1e-3, atol=1e-4)
    # a volume of another size (48^3 on a 32^3 model): position table resized on the device for the call
    r = fx["resized_48"]
    x48 = torch.from_numpy(O.hash_uniform(2 * 48 ** 3, r["x_seed"]).reshape(2, 1, 48, 48, 48).astype(np.float32)) * 0.5 + 0.5
    out, hidden = model(x48.to(cuda))
    o_out, o_hidden = O.vit_forward(params, x48, 16, 3, 2)
    assert out.shape == (2, 30, 192) and rel_err(out, o_out) < tol
    for a, b in zip(hidden, o_hidden):
        assert rel_err(a, b) < tol
    if dtype == "fp32":
        for t, entry in [(out, r["out"])] + list(zip(hidden, r["hidden"])):
            got, want, l2, l2w = sample_of(t, entry)
            assert torch.allclose(got, want, rtol=1e-3, atol=1e-4)
    with pytest.raises(Exception, match="multiple of 16"):
        model(torch.zeros(1, 1, 40, 40, 40, device=cuda))


@pytest.mark.parametrize("name", ["linear", "attention_q1", "attention_q3", "vit_tanh", "vit_linear"])
def test_classifier_heads_vs_oracle_and_reference_fixture(lib, cuda, name):
    """HIP LinearClassifier / AttentionClassifier (eval arithmetic) and ViT(classification=True) vs the oracle and the
    outputs of the reference's own modules (tests/golden/classifier_heads.json).  fp32 path: rel 1e-3 (observed ~1e-6)."""
    import json, os
    from headct_foundation_amd import AttentionClassifier, LinearClassifier, ViT
    from tests.test_oracle_golden import _head_inputs, _head_oracle
    e = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "classifier_heads.json")))[name]
    params, x = _head_inputs(name, e)
    want = _head_oracle(name, e, params, x)
    if name == "linear":
        model = LinearClassifier(**e["ctor"])
    elif name.startswith("attention"):
        model = AttentionClassifier(**e["ctor"])
    else:
        model = ViT(**e["ctor"], compute_dtype="fp32")
    model.load_state_dict(params, strict=True)
    model = model.to(cuda).eval()
    out = model(x.to(cuda))
    out = out[0] if isinstance(out, tuple) else out
    assert out.shape == want.shape and rel_err(out, want) < 1e-3
    assert torch.allclose(out.cpu(), torch.tensor(e["out"]).reshape(want.shape), rtol=1e-3, atol=1e-5)


def test_attention_classifier_bf16_full_width(lib, cuda):
    """AttentionClassifier at ViT-B width on 217 tokens, bf16 key/value projection (MFMA GEMM) vs the oracle: 2e-2."""
    from headct_foundation_amd import AttentionClassifier
    torch.manual_seed(5)
    m = AttentionClassifier(768, 5, num_heads=12, qkv_bias=True, num_queries=4, compute_dtype="bf16")
    with torch.no_grad():
        m.cls_token.mul_(40.0)
        m.bn1.running_mean.normal_(0, 0.2)
        m.bn1.running_var.uniform_(0.5, 1.5)
        m.bn2.running_mean.normal_(0, 0.05)
        m.bn2.running_var.uniform_(0.05, 0.2)
    params = {k: v.detach().clone() for k, v in m.state_dict().items()}
    x = torch.randn(6, 217, 768)
    want = O.attention_classifier_forward(params, x, 12, 4)
    out = m.to(cuda).eval()(x.to(cuda))
    assert rel_err(out, want) < 2e-2


def test_linear_probe_step_vs_oracle_and_reference_fixture(lib, cuda):
    """Linear probing on the HIP kernels (training-mode LinearClassifier, cross_entropy, backward, running statistics) vs the
    oracle and the reference-generated fixture: fp32, rel 1e-3 (observed ~1e-6); then a few AdamW steps must lower the loss."""
    import json, os
    from headct_foundation_amd import LinearClassifier, cross_entropy
    from tests.test_oracle_golden import _head_inputs
    e = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "classifier_heads.json")))["linear_probe_step"]
    params, x = _head_inputs("linear_probe_step", e)
    target = torch.tensor(e["target"])
    o_logits, o_loss, o_grads, o_stats = O.linear_probe_step(params, x, target)
    model = LinearClassifier(**e["ctor"])
    model.load_state_dict(params, strict=True)
    model = model.to(cuda).train()
    xg, tg = x.to(cuda), target.to(cuda)
    logits = model(xg)
    loss = cross_entropy(logits, tg)
    loss.backward()
    assert rel_err(logits.detach(), o_logits) < 1e-3 and abs(float(loss.detach()) - float(o_loss)) < 1e-5
    assert abs(float(loss.detach()) - e["loss"]) < 1e-5
    assert rel_err(model.linear.weight.grad, o_grads["linear.weight"]) < 1e-3
    assert rel_err(model.linear.bias.grad, o_grads["linear.bias"]) < 1e-3
    assert torch.allclose(model.linear.weight.grad.cpu().flatten(), torch.tensor(e["grad_weight"]), rtol=1e-3, atol=1e-6)
    assert rel_err(model.bn.running_mean, o_stats["bn.running_mean"]) < 1e-5 and rel_err(model.bn.running_var, o_stats["bn.running_var"]) < 1e-5
    assert int(model.bn.num_batches_tracked) == 1
    # torch's own loss on the HIP logits gives the same parameter gradients through the HIP backward
    model.zero_grad()
    torch.nn.functional.cross_entropy(model(xg), tg).backward()
    assert rel_err(model.linear.weight.grad, o_grads["linear.weight"]) < 1e-3
    # upstream scale (loss / accumulation steps) reaches the gradients
    model.zero_grad()
    (cross_entropy(model(xg), tg) / 4).backward()
    assert rel_err(model.linear.weight.grad * 4, o_grads["linear.weight"]) < 1e-3
    opt = torch.optim.AdamW(model.parameters(), lr=1e-2)
    first = None
    for _ in range(20):
        opt.zero_grad()
        l = cross_entropy(model(xg), tg)
        l.backward()
        opt.step()
        first = float(l.detach()) if first is None else first
    assert float(l.detach()) < 0.5 * first
    with pytest.raises(Exception, match="detached"):
        model(xg.clone().requires_grad_(True))
    bad = cross_entropy(model(xg), torch.tensor([0, 7, 1, 1, 0], device=cuda))
    assert not torch.isfinite(bad.detach())


@pytest.mark.parametrize("name,dtype,tol_loss,tol_grad", [("micro", "fp32", 1e-3, 1e-3), ("tiny", "bf16", 5e-3, 6e-2)])
def test_odd_and_changing_batch_sizes_vs_oracle(lib, cuda, name, dtype, tol_loss, tol_grad):
    """Ragged row counts (batch 3, 1, 5 -> token rows that are no multiple of any tile) on ONE model instance, as the
    short last batch of an epoch produces them: each batch size gets its own plan; loss and gradients vs the oracle."""
    cfg = O.CONFIGS[name]
    params = O.make_params(cfg, 0)
    model = build_hip_model(cfg, params, cuda, dtype, full_pred=False)  # the module default (compact decoder tail)
    model.train()
    # bf16 also at batch 41: past the 8-, 16- and 32-volume trips of the batch reductions (fp32: test_batch_reductions_past_their_loop_limits_vs_oracle)
    for batch in (3, 1, 5, 3) + ((41,) if dtype == "bf16" else ()):
        x, noise = O.make_volume(cfg, batch, 20 + batch), O.make_noise(cfg, batch, 20 + batch)
        o_loss, o_pred, o_mask, o_grads, _ = O.forward_backward(cfg, params, x, noise)
        model.zero_grad()
        loss, _, _ = model(x.to(cuda), noise=noise.to(cuda))
        loss.backward()
        torch.cuda.synchronize()
        assert abs(float(loss.detach()) - float(o_loss)) / abs(float(o_loss)) < tol_loss, batch
        assert torch.equal(model.last_mask(batch).cpu(), o_mask)
        grads = grads_by_name(model)
        worst = max((rel_err(grads[k], o_grads[k]), k) for k in grads if not k.endswith("qkv.bias"))
        assert worst[0] < tol_grad, (batch, worst)
        for k in grads:
            if k.endswith("qkv.bias"):  # K-third has a mathematically zero gradient: compare absolutely
                assert (grads[k] - o_grads[k]).abs().max() < 1e-6 + tol_grad * o_grads[k].abs().max(), (batch, k)


@pytest.mark.parametrize("batch", [41,    # dec0_table_sum_kernel's 32-volume trip (4 groups x 8) taken twice; 8- and 16-volume trips of dpos / dcls
                                   261])  # kAsmBlocks = 256 reduce blocks take a second volume; fold_partials / dec0_token_grads fold nblk = 256 > 128 partials
def test_batch_reductions_past_their_loop_limits_vs_oracle(lib, cuda, batch):
    """The plan-only kernels (dec0_index, dec0_table, dec0_table_sum, dec0_token_grads, the compact form of the masked MSE) and the
    assembly backwards at batch sizes whose reductions take their loops more than once: `micro` with two decoder blocks, fp32, in
    the four settings {full_pred} x {dec0_table}.  Loss and every gradient against the oracle at 1e-3, the four settings against each
    other at 1e-5.  Batch 261 also folds 261 x 48 = 12528 compact loss rows (loss_fold_kernel: 2048 per trip) and, with full_pred,
    261 x 64 rows."""
    import dataclasses
    cfg = dataclasses.replace(O.CONFIGS["micro"], decoder_depth=2)
    params = O.make_params(cfg, 0)
    x, noise = O.make_volume(cfg, batch, 20 + batch), O.make_noise(cfg, batch, 20 + batch)
    o_loss, _, o_mask, o_grads, _ = O.forward_backward(cfg, params, x, noise)
    assert batch * (cfg.num_patches - cfg.len_keep) > (2048 if batch > 256 else 0)
    xd, nd = x.to(cuda), noise.to(cuda)
    out = {}
    for full_pred in (True, False):
        for table in (True, False):
            m = build_hip_model(cfg, params, cuda, "fp32", full_pred=full_pred)
            m.dec0_table = table
            m.train()
            loss, _, _ = m(xd, noise=nd)
            loss.backward()
            torch.cuda.synchronize()
            key = (full_pred, table)
            out[key] = (float(loss.detach()), grads_by_name(m))
            assert torch.equal(m.last_mask(batch).cpu(), o_mask), key
            assert abs(out[key][0] - float(o_loss)) / abs(float(o_loss)) < 1e-3, key
            assert set(out[key][1]) == set(o_grads)
            worst = max((rel_err(out[key][1][k], o_grads[k]), k) for k in o_grads if not k.endswith("qkv.bias"))
            print(f"batch {batch} full_pred={full_pred} dec0_table={table}: loss {out[key][0]:.7f} (oracle {float(o_loss):.7f}), worst gradient {worst}")
            assert worst[0] < 1e-3, (key, worst)
            for k in o_grads:
                if k.endswith("qkv.bias"):  # K-third has a mathematically zero gradient: compare absolutely
                    assert (out[key][1][k] - o_grads[k]).abs().max() < 1e-6 + 1e-3 * o_grads[k].abs().max(), (key, k)
    base = out[(True, False)]  # every row through every block
    for key, (loss, grads) in out.items():
        assert abs(loss - base[0]) <= 1e-5 * abs(base[0]), key
        for k, g in base[1].items():
            if k.endswith("qkv.bias"):
                assert (grads[k] - g).abs().max() <= 1e-6 + 1e-5 * g.abs().max(), (key, k)
            else:
                assert rel_err(grads[k], g) < 1e-5, (key, k, rel_err(grads[k], g))


@pytest.mark.parametrize("mask_ratio", [0.5, 0.9])
def test_other_mask_ratios_vs_oracle(lib, cuda, mask_ratio):
    """The number of kept tokens follows int(L * (1 - mask_ratio)) (mae.py:204): other ratios than the fixtures' against the
    oracle, fp32, rel 1e-3."""
    import dataclasses
    cfg = dataclasses.replace(O.CONFIGS["micro"], mask_ratio=mask_ratio)
    params = O.make_params(cfg, 3)
    x, noise = O.make_volume(cfg, 2, 3), O.make_noise(cfg, 2, 3)
    o_loss, o_pred, o_mask, o_grads, _ = O.forward_backward(cfg, params, x, noise)
    model, loss = _run_hip(cfg, params, x, noise, cuda, "fp32")
    assert int(o_mask.sum()) == 2 * (cfg.num_patches - int(cfg.num_patches * (1 - mask_ratio)))
    assert abs(loss - float(o_loss)) / abs(float(o_loss)) < 1e-3
    assert torch.equal(model.last_mask(2).cpu(), o_mask)
    assert rel_err(model.last_pred(2), o_pred) < 1e-3
    grads = grads_by_name(model)
    worst = max((rel_err(grads[k], o_grads[k]), k) for k in grads if not k.endswith("qkv.bias"))
    assert worst[0] < 1e-3, worst


@pytest.mark.parametrize("mask_ratio,kept", [(0.6, 400), (0.9, 99)])
def test_thousand_patch_grid_keeps_the_reference_count(lib, cuda, mask_ratio, kept):
    """L = 1000 (80^3 volume, 8^3 patches): int(1000 * (1 - 0.9)) = 99 and int(1000 * (1 - 0.6)) = 400 in Python doubles; a
    float32 ratio across the C ABI gave 100 / 399.  Loss, mask and gradients against the oracle, fp32, rel 1e-3."""
    import dataclasses
    cfg = dataclasses.replace(O.CONFIGS["micro"], input_size=80, patch_size=8, mask_ratio=mask_ratio, encoder_depth=1)
    assert int(cfg.num_patches * (1 - mask_ratio)) == kept
    params = O.make_params(cfg, 5)
    x, noise = O.make_volume(cfg, 1, 5), O.make_noise(cfg, 1, 5)
    o_loss, o_pred, o_mask, o_grads, _ = O.forward_backward(cfg, params, x, noise)
    model, loss = _run_hip(cfg, params, x, noise, cuda, "fp32")
    assert model.len_keep == kept and int(o_mask.sum()) == cfg.num_patches - kept
    assert torch.equal(model.last_mask(1).cpu(), o_mask)
    assert abs(loss - float(o_loss)) / abs(float(o_loss)) < 1e-3
    grads = grads_by_name(model)
    worst = max((rel_err(grads[k], o_grads[k]), k) for k in grads if not k.endswith("qkv.bias"))
    assert worst[0] < 1e-3, worst


@pytest.mark.parametrize("name,batch,seed", CASES)
def test_bf16_gradients_vs_bf16_storage_oracle(lib, cuda, name, batch, seed):
    """The benchmark dtype held tighter than the 6e-2 of the fp32-oracle comparison above: the oracle is run with bfloat16
    rounding at the points where the HIP bf16 path stores bfloat16 (oracle/mae_oracle.py `emulate_bf16`), so rounding is common
    to both sides and what remains is accumulation order plus the rounding of backward intermediates.
    Tolerances: loss 1e-3 relative, pred 5e-3, per-tensor gradient L2 2e-2 (3x tighter than against the fp32 oracle; a wrong
    low-order term in one epilogue mode -- a missing bias, a dropped scale, gelu' of the wrong argument -- is 1e-1 and more)."""
    cfg = O.CONFIGS[name]
    params = O.make_params(cfg, seed)
    x, noise = O.make_volume(cfg, batch, seed), O.make_noise(cfg, batch, seed)
    o_loss, o_pred, o_mask, o_grads, _ = O.forward_backward(cfg, params, x, noise, emulate_bf16=True)
    model, loss = _run_hip(cfg, params, x, noise, cuda, "bf16")
    assert abs(loss - float(o_loss)) / abs(float(o_loss)) < 1e-3
    assert rel_err(model.last_pred(batch), o_pred) < 5e-3
    grads = grads_by_name(model)
    bad = [(rel_err(grads[k], o_grads[k]), k) for k in grads if not k.endswith("qkv.bias")]
    assert max(bad)[0] < 2e-2, sorted(bad)[-5:]
    for k in grads:
        if k.endswith("qkv.bias"):  # K-third has a mathematically zero gradient: compare absolutely
            assert (grads[k] - o_grads[k]).abs().max() < 1e-6 + 2e-2 * o_grads[k].abs().max(), k


@pytest.mark.parametrize("name,steps", [("tiny", 24), ("vitb_cut", 20)])
def test_bf16_loss_curve_vs_oracle(lib, cuda, name, steps):
    """`north_star`: "loss curve matching reference within tolerance", on the dtype the benchmark runs (bf16 storage + MFMA).
    BASELINE config #1 (ViT-Tiny, 64^3, B=2) and the ViT-B tile shapes (`vitb_cut`: D=768, 96^3, N=55/217, dh=64/48), >= 20
    optimizer steps of train_one_epoch's iteration (zero_grad, forward, backward, clip 3.0, AdamW, cosine-warmup LR) against the
    fp32 oracle on the same volumes and masks.  Tolerance: every step's loss within 5e-3 relative of the fp32 curve, the last
    five within 3e-3 on average, and within 3e-3 of the bf16-storage oracle's curve (printed beside it).
    The learning rate is raised so that the loss actually moves (>= 10 % over the run): a flat curve would prove nothing."""
    from headct_foundation_amd.lr_sched import get_cosine_schedule_with_warmup
    from headct_foundation_amd.optim import HipAdamW, clip_gradients
    cfg = O.CONFIGS[name]
    B = 2
    hp = dict(base_lr=2e-3, min_lr=2e-6, warmup=4, total=60, weight_decay=5e-3, grad_clip=3.0)
    params = O.make_params(cfg, 7)
    st32 = O.TrainState({k: v.clone() for k, v in params.items()})
    st16 = O.TrainState({k: v.clone() for k, v in params.items()})
    model = build_hip_model(cfg, params, cuda, "bf16", full_pred=False).train()  # the module default, as bench.py / the engine run it
    opt = HipAdamW(model, lr=hp["base_lr"], weight_decay=hp["weight_decay"], betas=(0.9, 0.95))
    sched = get_cosine_schedule_with_warmup(opt, hp["warmup"], hp["total"], lr_end=hp["min_lr"])
    hip, ref32, ref16 = [], [], []
    for i in range(steps):
        x, noise = O.make_volume(cfg, B, 100 + i % 4), O.make_noise(cfg, B, 200 + i)
        ref32.append(O.train_step(cfg, st32, x, noise, **hp)[0])
        ref16.append(O.train_step(cfg, st16, x, noise, emulate_bf16=True, **hp)[0])
        opt.zero_grad()
        loss, _, _ = model(x.to(cuda), noise=noise.to(cuda))
        loss.backward()
        clip_gradients(model, hp["grad_clip"])
        opt.step(); sched.step()
        hip.append(float(loss.detach()))
    rel = [abs(a - b) / abs(b) for a, b in zip(hip, ref32)]
    print(f"\\n{name}: step  hip-bf16   oracle-fp32  oracle-bf16-storage")
    for i in range(steps):
        print(f"   {i:3d}  {hip[i]:.5f}   {ref32[i]:.5f}      {ref16[i]:.5f}")
    assert ref32[0] - min(ref32) > 0.1 * ref32[0], "the reference curve is flat: raise the learning rate"
    assert max(rel) < 5e-3, (max(rel), rel.index(max(rel)))          # observed <= 2e-3
    assert sum(rel[-5:]) / 5 < 3e-3
    rel16 = [abs(a - b) / abs(b) for a, b in zip(hip, ref16)]
    assert max(rel16) < 3e-3, (max(rel16), rel16.index(max(rel16)))   # observed <= 1e-3: rounding is common to both sides


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_fp16_cached_volumes_are_read_directly(lib, cuda, dtype):
    """The persistent cache stores fp16 volumes (transforms.py:171-178).  The patch gather and the masked-MSE pass read them as
    they are (half the input bytes of a step): loss and every gradient are bit-identical to feeding the same values as fp32,
    and within the oracle's tolerance of the oracle run on those values."""
    cfg = O.CONFIGS["micro"]
    params = O.make_params(cfg, 4)
    x16 = O.make_volume(cfg, 2, 4).half()
    noise = O.make_noise(cfg, 2, 4)
    o_loss, _, _, o_grads, _ = O.forward_backward(cfg, params, x16.float(), noise)
    m_h, loss_h = _run_hip(cfg, params, x16, noise, cuda, dtype)
    g_h = grads_by_name(m_h)
    m_f, loss_f = _run_hip(cfg, params, x16.float(), noise, cuda, dtype)
    g_f = grads_by_name(m_f)
    assert loss_h == loss_f and all(torch.equal(g_h[k], g_f[k]) for k in g_f)
    assert abs(loss_h - float(o_loss)) / abs(float(o_loss)) < (1e-3 if dtype == "fp32" else 5e-3)
