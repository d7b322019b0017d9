"""Bit-level digest of the native plan (csrc/mae_plan.hip): one training forward + backward per case with fixed seeds; per case the
fp32 bit pattern of the loss and the sha256 of the flat gradient and of every named activation.  Two builds that launch the same
kernels in the same order on the same operands print the same digest; a moved launch or weight-gradient queue entry changes it.

    python scripts/plan_digest.py > digest.json      # every case, one JSON object {case: digest}
    python scripts/plan_digest.py CASE               # one case (cases that set an environment switch run as such a child)
"""
import dataclasses
import hashlib
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import mae_oracle as O  # noqa: E402

ACTS = (["ids_restore", "ids_shuffle", "mask", "patches", "tok", "enc_in", "latent", "dec_in", "tail_rows", "pred_full", "dpred_full",
         "enc0.qkv", "enc0.attn_o", "enc0.lora_t"] + [f"{s}{i}.out" for s in ("enc", "dec") for i in range(12)])


def sha(t):
    return hashlib.sha256(t.detach().contiguous().view(-1).view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def digest(model, batch, loss):
    torch.cuda.synchronize()
    out = {"loss": None if loss is None else "%08x" % (loss.detach().float().cpu().view(torch.int32).item() & 0xFFFFFFFF),
           "grad": sha(model._flat_grad), "acts": {}}
    plan = model._plan_for(batch)
    for name in ACTS:
        try:
            out["acts"][name] = sha(plan.activation(name))
        except KeyError:
            pass
    return out


def mae(name, dtype, full_pred=True, dec0=True, rms=False, bias=None, drop=0.0, group_blocks=None):
    from headct_foundation_amd import MaskedAutoencoderViT, RMSNorm
    cfg = dataclasses.replace(O.CONFIGS[name], decoder_depth=3)  # block 0: cat rows, block 1: every row, block 2: compact tail
    if bias is not None:
        cfg = dataclasses.replace(cfg, use_bias=bias)
    kw = dict(cfg.ctor_kwargs(), dropout_rate=drop, compute_dtype=dtype)
    m = MaskedAutoencoderViT(**kw, norm_layer=RMSNorm) if rms else MaskedAutoencoderViT(**kw)
    m.load_state_dict({k: v for k, v in O.make_params(cfg, 0).items() if k in m.state_dict()}, strict=True)
    m.full_pred, m.dec0_table = full_pred, dec0
    m = m.to("cuda").train()
    if group_blocks is not None:  # the flush policy of the data-parallel wrapper, without a process group
        m._bucket_hook, m.wgrad_group_blocks = (lambda stage, begin, end: None), group_blocks
    if drop:
        m.set_dropout_seed(1234)
    loss, _, _ = m(O.make_volume(cfg, 3, 0).to("cuda"), noise=O.make_noise(cfg, 3, 0).to("cuda"))
    loss.backward()
    return digest(m, 3, loss)


def vit(hidden, heads, dtype, regs=0, lora=False, drop=0.0):
    from headct_foundation_amd.dino_model import ViTBackbone
    from headct_foundation_amd.misc import set_requires_grad_false
    torch.manual_seed(hidden + regs)
    m = ViTBackbone(in_chans=3, img_size=24, patch_size=12, hidden_size=hidden, mlp_dim=2 * hidden, num_layers=2, num_heads=heads,
                    num_register_tokens=regs, lora=lora, dropout_rate=drop, compute_dtype=dtype)
    sd = m.state_dict()
    m.load_state_dict({k: torch.randn(v.shape) * (0.005 if k.endswith("lora_matrix_B") else 0.5 if "token" in k else 0.05) for k, v in sd.items()})
    m = m.to("cuda").train()
    if lora:
        set_requires_grad_false(m, lora=True)  # the backbone's matrices and tokens frozen, adapters / biases / norms train
    if drop:
        m.set_dropout_seed(4321)
    out = m(torch.rand(2, 3, 24, 24, 24).to("cuda"))[0]
    out.backward(torch.randn(out.shape).to(out))
    return digest(m, 2, None)


CASES, ENV = {}, {}
for _n in ("micro", "tiny"):
    for _d in ("fp32", "bf16"):
        for _f in (True, False):
            for _t in (True, False):
                for _r in (False, True):
                    CASES[f"mae.{_n}.{_d}.full{int(_f)}.dec0{int(_t)}.{'rms' if _r else 'ln'}"] = \
                        (lambda n=_n, d=_d, f=_f, t=_t, r=_r: mae(n, d, f, t, r))
for _d in ("fp32", "bf16"):
    CASES[f"mae.micro.{_d}.nobias"] = lambda d=_d: mae("micro", d, False, bias=False)
    CASES[f"mae.micro.{_d}.drop"] = lambda d=_d: mae("micro", d, False, drop=0.1)
    CASES[f"mae.micro.{_d}.folds0"] = lambda d=_d: mae("micro", d, False)
    ENV[f"mae.micro.{_d}.folds0"] = {"HCT_DEFER_FOLDS": "0"}
    for _h, _k in ((48, 3), (128, 2)):
        CASES[f"vit.{_h}.{_d}.plain"] = lambda d=_d, h=_h, k=_k: vit(h, k, d)
        CASES[f"vit.{_h}.{_d}.regs2"] = lambda d=_d, h=_h, k=_k: vit(h, k, d, regs=2)
        CASES[f"vit.{_h}.{_d}.lora"] = lambda d=_d, h=_h, k=_k: vit(h, k, d, lora=True)
        CASES[f"vit.{_h}.{_d}.drop"] = lambda d=_d, h=_h, k=_k: vit(h, k, d, drop=0.1)
CASES["mae.micro.bf16.group1"] = lambda: mae("micro", "bf16", False, group_blocks=1)

if __name__ == "__main__":
    if len(sys.argv) > 1:
        print(json.dumps(CASES[sys.argv[1]](), sort_keys=True))
        sys.exit(0)
    result = {}
    for case, run in CASES.items():
        if case in ENV:  # the switch is read by the library: a fresh process per environment
            r = subprocess.run([sys.executable, os.path.abspath(__file__), case], env=dict(os.environ, **ENV[case]), capture_output=True, text=True, check=True)
            result[case] = json.loads(r.stdout.strip().splitlines()[-1])
        else:
            result[case] = run()
    print(json.dumps(result, sort_keys=True, indent=1))
