"""MAE reconstruction and error maps: `MaskedAutoencoderViT.reconstruct` (hct_mae_recon_accum after every forward, hct_mae_recon_finish
at the end) against the same work written as a torch composition (last_pred -> float -> where(mask) -> unpatchify -> subtract ->
square -> mean), on ViT-B/16^3 at 96^3, mask ratio 0.75, bf16, B = 64, for 2 and 4 passes.  Both run in one process in alternating
blocks of timed calls, each block between two device synchronisations; the no-grad forwards are the same on both sides.  The two
kernels and the torch glue are also timed on their own, on the activations one forward left behind.  Prints one JSON line: ms per
batch for each path, the share of the fused path spent in the two kernels, and their bytes over time against the HBM floor.  The
bytes are counted from shapes: per pass B M pd (sizeof(pred) + sizeof(x) + 8) (prediction and target read, the fp32 sum read and
written), the finish B C S^3 8 (sum read, reconstruction written).

  python scripts/bench_reconstruct.py [--batch 64] [--passes 2 4] [--blocks 3] [--iters 2] [--x_dtype fp16|fp32] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from headct_foundation_amd import MaskedAutoencoderViT  # noqa: E402
from headct_foundation_amd.reconstruct import cover_noise, cover_slots, recon_accum, recon_finish  # noqa: E402

HBM_BYTES_PER_S = 8.0e12
VITB = dict(input_size=96, patch_size=16, mask_ratio=0.75, in_chans=1, encoder_depth=12, encoder_embed_dim=768, encoder_mlp_dim=3072,
            encoder_num_heads=12, decoder_depth=8, decoder_embed_dim=768, decoder_mlp_dim=3072, decoder_num_heads=16)


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def torch_glue(model, x, target, rs, es, cnt):
    """One pass of the composition on the activations of the last forward."""
    B, L = cnt.shape
    pred = model.last_pred(B)
    mask = model.last_mask(B).view(B, L)
    if model.norm_pix_loss:
        t, mu, sd = target
        v, tgt = pred * sd + mu, (t - mu) / sd
    else:
        v, tgt = pred, target[0]
    rs += model.unpatchify(torch.where(mask.unsqueeze(-1) != 0, v, torch.zeros_like(v)), x)
    es += ((pred - tgt) ** 2).mean(dim=-1) * mask
    cnt += mask


def torch_finish(model, x, rs, es, cnt):
    B, L = cnt.shape
    c = cnt.clamp(min=1)
    seen = model.unpatchify(cnt.unsqueeze(-1).expand(B, L, model.out_chans).contiguous(), x) > 0
    per_voxel = model.unpatchify(c.unsqueeze(-1).expand(B, L, model.out_chans).contiguous(), x)
    return torch.where(seen, rs / per_voxel, x.float()), torch.where(cnt > 0, es / c, torch.zeros_like(es))


def torch_reconstruct(model, x, noises):
    B, L = x.shape[0], model.num_patches
    t = model.patchify(x.float())
    target = (t,)
    if model.norm_pix_loss:
        target = (t, t.mean(dim=-1, keepdim=True), (t.var(dim=-1, keepdim=True) + 1.0e-6) ** 0.5)
    rs = torch.zeros(x.shape, dtype=torch.float32, device=x.device)
    es, cnt = torch.zeros(B, L, device=x.device), torch.zeros(B, L, device=x.device)
    with torch.no_grad():
        for nz in noises:
            model(x, noise=nz)
            torch_glue(model, x, target, rs, es, cnt)
        return torch_finish(model, x, rs, es, cnt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--passes", type=int, nargs="+", default=[2, 4])
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--x_dtype", choices=["fp16", "fp32"], default="fp16", help="fp16: the persistent cache's format")
    ap.add_argument("--out", type=str, default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_reconstruct.py needs an MI355X: the path has no CPU fallback")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = MaskedAutoencoderViT(**VITB, compute_dtype="bf16").to(dev).eval()
    B, L, K, S, P, C = a.batch, model.num_patches, model.len_keep, 96, 16, 1
    M, pd = L - K, model.out_chans
    x = torch.rand(B, C, S, S, S, device=dev, generator=torch.Generator(device=dev).manual_seed(0)).to(torch.float16 if a.x_dtype == "fp16" else torch.float32)
    med = lambda v: sorted(v)[len(v) // 2]
    result = {"metric": "MAE reconstruction + error map, ViT-B/16^3 at 96^3, mask 0.75, bf16", "batch": B, "x_dtype": a.x_dtype, "blocks": a.blocks,
              "iters": a.iters, "runs": []}
    for n in a.passes:
        slot = cover_slots(B, L, 0, dev)
        noises = [cover_noise(slot, p, n, K) for p in range(n)]
        fused = lambda: model.reconstruct(x, passes=n, seed=0)
        eager = lambda: torch_reconstruct(model, x, noises)
        rec, (recon_t, err_t) = fused(), eager()
        agree = {"recon": float((rec.recon - recon_t).norm() / recon_t.norm()), "error": float((rec.error.view(B, L) - err_t).norm() / err_t.norm())}
        for _ in range(a.warmup):
            fused(), eager()
        ms_f, ms_e = [], []
        for _ in range(a.blocks):
            ms_f.append(timed(fused, a.iters))
            ms_e.append(timed(eager, a.iters))
        # the glue alone, on the activations of one forward: n accumulate launches + one finish, against n torch passes + the torch finish
        with torch.no_grad():
            model(x, noise=noises[0])
        plan = model._plan_for(B)
        pred, mask = plan.activation("pred_full"), plan.activation("mask")
        rs, es, cnt = torch.empty(x.shape, dtype=torch.float32, device=dev), torch.empty(B, L, device=dev), torch.zeros(B, L, dtype=torch.int32, device=dev)

        def kernels():
            cnt.zero_()
            for _ in range(n):
                recon_accum(pred, True, x, mask, P, model.norm_pix_loss, rs, es, cnt)
            recon_finish(rs, es, cnt, x, P, inplace=True)

        t = model.patchify(x.float())
        rs_t, es_t, cnt_t = torch.zeros(x.shape, dtype=torch.float32, device=dev), torch.zeros(B, L, device=dev), torch.zeros(B, L, device=dev)

        def glue():
            with torch.no_grad():
                for _ in range(n):
                    torch_glue(model, x, (t,), rs_t, es_t, cnt_t)
                torch_finish(model, x, rs_t, es_t, cnt_t)

        kernels(), glue()
        ms_k = med([timed(kernels, 10) for _ in range(a.blocks)])
        ms_g = med([timed(glue, 10) for _ in range(a.blocks)])
        nbytes = n * B * M * pd * (2 + x.element_size() + 8) + B * C * S ** 3 * 8
        f, e = med(ms_f), med(ms_e)
        result["runs"].append({
            "passes": n, "fused_ms_per_batch": round(f, 3), "fused_ms_min_max": [round(min(ms_f), 3), round(max(ms_f), 3)],
            "torch_composition_ms_per_batch": round(e, 3), "torch_ms_min_max": [round(min(ms_e), 3), round(max(ms_e), 3)],
            "kernels_ms": round(ms_k, 4), "kernels_share_of_fused": round(ms_k / f, 5), "torch_glue_ms": round(ms_g, 4),
            "kernel_bytes_mb": round(nbytes / 2 ** 20, 1), "kernels_gb_per_s": round(nbytes / (ms_k * 1e-3) / 1e9, 1),
            "hbm_floor_ms": round(nbytes / HBM_BYTES_PER_S * 1e3, 4), "kernels_share_of_hbm_floor": round(nbytes / HBM_BYTES_PER_S * 1e3 / ms_k, 4),
            "relative_l2_fused_vs_torch": {k: float(f"{v:.3e}") for k, v in agree.items()},
        })
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
