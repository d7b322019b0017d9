"""The step-level check: gradients (and activations) of a whole training step held per row and per column to the oracle run in
float64, with bounds that come from the reference side alone.

One relative L2 per tensor (tests/util.py::rel_err) cannot see a fault confined to a few rows or columns -- a tile tail, one
volume's contribution missing from a batch reduction, a bias column sum folded from the wrong partial, a row map off by one.  This
file defines the measure that can, the yardsticks it is held to, and the faults that tests/test_step_ref_cpu.py plants to prove it.

Views.  A tensor is viewed 2-D as (shape[0], -1) after its leading singletons are dropped: the (1, L, D) tables are L x D, the
(1, 1, D) tokens are vectors.  A vector is D slices of one element; a matrix has two families of slices, rows and columns.

Slice error.  err(s) = ||G_s - O_s|| / (||O_s|| + R), R = the RMS of ||O_s|| over the slices of that family.  The `+ R` puts a
slice whose true gradient is zero (the K third of qkv.bias, the position row of a patch no sample kept) on the tensor's own scale;
it belongs to the definition and is no tolerance.  E(G, O) = the maximum of err over both families.

Yardsticks, per case and per tensor, from the reference side only:
    fp32 mode   Y32 = E(oracle in fp32, oracle in fp64)
    bf16 mode   Ybf = E(bf16-storage oracle in fp64, plain oracle in fp64); the device is compared with the bf16-storage oracle
                in fp64.  Ybf is what the forward's bf16 stores cost the tensor; the device also rounds its backward intermediates,
                which the emulation does not -- about as many rounding sites again, hence a distance of the same order.
Bound: E(device, reference) <= M * Y.  M32 / MBF below are the margins in force, M32_CAP / MBF_CAP the conditions they may never
exceed (tests/test_step_ref_cpu.py proves that every required planted fault still fails at the caps).
"""
import dataclasses

import numpy as np
import torch
import torch.nn.functional as F

from oracle import mae_oracle as O
from tests import lora_ref
from tests import rmsnorm_ref as R

# Margins (E <= M * Y).  Start values: 4 (the optimizer tests' precedent) and 2.  The rule for raising one: the next power of two
# at or above twice the worst ratio measured on the device, never above the cap.  Measured ratios (worst fp32 17.4, worst bf16
# 1.75): the docstring of tests/test_step_rows_gpu.py and DESIGN.md section 3.
M32, MBF = 64.0, 2.0
M32_CAP, MBF_CAP = 256.0, 4.0

CASES = [("micro", 2, 0), ("yaml_cut", 2, 1), ("tiny", 2, 0), ("vitb_cut", 2, 0)]
FAULTS = ("row_lacks_sample", "element_lacks_sample", "column_halved", "tail_rows_scaled", "rows_swapped")


# ---- the measure ---------------------------------------------------------------------------------------------------------------
def view2d(t: torch.Tensor) -> torch.Tensor:
    """float64 CPU copy of `t`, leading singletons dropped, then (shape[0], -1); vectors and scalars come back 1-D."""
    t = t.detach().double().cpu()
    while t.dim() > 1 and t.shape[0] == 1:
        t = t[0]
    return t.reshape(-1) if t.dim() <= 1 else t.reshape(t.shape[0], -1)


def _family(diff_norm: torch.Tensor, ref_norm: torch.Tensor) -> torch.Tensor:
    rms = ref_norm.pow(2).mean().sqrt()
    if float(rms) == 0.0:  # an all-zero reference: any difference at all is infinitely far on the tensor's own scale
        return torch.where(diff_norm > 0, torch.full_like(diff_norm, float("inf")), torch.zeros_like(diff_norm))
    return diff_norm / (ref_norm + rms)


def slice_errors(g: torch.Tensor, o: torch.Tensor):
    """{family: err per slice} of `g` against the reference `o` ("rows" and "cols" for a matrix, "elems" for a vector)."""
    g, o = view2d(g), view2d(o)
    assert g.shape == o.shape, (tuple(g.shape), tuple(o.shape))
    if o.dim() == 1:
        return {"elems": _family((g - o).abs(), o.abs())}
    d = g - o
    return {"rows": _family(d.norm(dim=1), o.norm(dim=1)), "cols": _family(d.norm(dim=0), o.norm(dim=0))}


def E(g: torch.Tensor, o: torch.Tensor) -> float:
    return max(float(e.max()) for e in slice_errors(g, o).values())


def E_where(g: torch.Tensor, o: torch.Tensor):
    """(E, family, index of the worst slice): for messages."""
    return max((float(e.max()), fam, int(e.argmax())) for fam, e in slice_errors(g, o).items())


def E_rows(g: torch.Tensor, o: torch.Tensor) -> float:
    """The same statistic on an activation: [..., D] viewed as tokens x D, rows (= tokens) only."""
    o = o.detach().double().cpu()
    o = o.reshape(-1, o.shape[-1])
    g = g.detach().double().cpu().reshape(o.shape)
    return float(_family((g - o).norm(dim=1), o.norm(dim=1)).max())


# ---- the references, run once per case ------------------------------------------------------------------------------------------
_REF = {}


def mae_cfg(name: str, decoder_depth=None):
    cfg = O.CONFIGS[name]
    return cfg if decoder_depth is None else dataclasses.replace(cfg, decoder_depth=decoder_depth)


def act_keys(cfg):
    return (["enc_in", "latent", "dec_in", "pred"] + [f"enc{i}.out" for i in range(cfg.encoder_depth)]
            + [f"dec{i}.out" for i in range(cfg.decoder_depth)])


class MaeRef:
    """One MAE case (config, batch, seed, norm): inputs, the oracle's runs by (precision, emulate_bf16) and the yardsticks."""

    def __init__(self, name, batch, seed, norm="layernorm", decoder_depth=None):
        self.cfg, self.batch, self.norm = mae_cfg(name, decoder_depth), batch, norm
        self.params = (R.make_params if norm == "rmsnorm" else O.make_params)(self.cfg, seed)
        self.x, self.noise = O.make_volume(self.cfg, batch, seed), O.make_noise(self.cfg, batch, seed)
        self._runs, self._y, self._per_sample = {}, {}, None

    def _fb(self, params, x, noise, emulate):
        fb = R.forward_backward if self.norm == "rmsnorm" else O.forward_backward
        return fb(self.cfg, params, x, noise, want_inter=True, emulate_bf16=emulate)

    def run(self, precision: str, emulate: bool = False):
        """dict(loss, mask, grads, acts) of the oracle in "f64" / "f32", with or without the bf16-storage emulation."""
        key = (precision, emulate)
        if key not in self._runs:
            dt = torch.float64 if precision == "f64" else torch.float32
            loss, pred, mask, grads, inter = self._fb({k: v.to(dt) for k, v in self.params.items()}, self.x.to(dt), self.noise, emulate)
            assert loss.dtype == dt and pred.dtype == dt and all(g.dtype == dt for g in grads.values()), "the oracle left its precision"
            self._runs[key] = dict(loss=loss, mask=mask, grads=grads, acts={k: inter[k] for k in act_keys(self.cfg)})
        return self._runs[key]

    def reference(self, mode: str):
        """What the device is compared with: fp32 mode -> the oracle in fp64; bf16 mode -> the bf16-storage oracle in fp64."""
        return self.run("f64", mode == "bf16")

    def yardstick(self, mode: str):
        """{tensor name | "loss" | "act:<key>": Y} -- Y32 (fp32 mode) or Ybf (bf16 mode)."""
        if mode not in self._y:
            if mode == "fp32":
                a, b = self.run("f32"), self.run("f64")
            else:
                a, b = self.run("f64", True), self.run("f64")
            y = {k: E(a["grads"][k], b["grads"][k]) for k in b["grads"]}
            y["loss"] = E(a["loss"], b["loss"])
            y.update({"act:" + k: E_rows(a["acts"][k], b["acts"][k]) for k in b["acts"]})
            self._y[mode] = y
        return self._y[mode]

    def per_sample(self):
        """[{name: contribution of sample b to the batch gradient}] in fp64: the gradient of (loss_b * mask_b).sum() / mask.sum().
        The samples do not interact, so it is the one-sample step's gradient scaled by mask_b.sum() / mask.sum()."""
        if self._per_sample is None:
            p64 = {k: v.double() for k, v in self.params.items()}
            total = float(self.run("f64")["mask"].sum())
            out = []
            for b in range(self.batch):
                _, _, mask, grads, _ = self._fb(p64, self.x[b:b + 1].double(), self.noise[b:b + 1], False)
                out.append({k: g * (float(mask.sum()) / total) for k, g in grads.items()})
            self._per_sample = out
        return self._per_sample


def mae_ref(name, batch, seed, norm="layernorm", decoder_depth=None) -> MaeRef:
    key = ("mae", name, batch, seed, norm, decoder_depth)
    if key not in _REF:
        _REF[key] = MaeRef(name, batch, seed, norm, decoder_depth)
    return _REF[key]


# ---- encoder-only --------------------------------------------------------------------------------------------------------------
# the case at real tile shapes: hidden 768, 12 heads, MLP 3072, one layer, 48^3 volume, patch 16 (L = 27), 2 registers, batch 3
VIT_TILE_CASE = dict(in_chans=1, img_size=48, patch_size=16, hidden_size=768, mlp_dim=3072, num_layers=1, num_heads=12,
                     num_register_tokens=2, qkv_bias=True, batch=3, seed=700, x_seed=55)


def vit_case(which: str, norm: str):
    """"tile": the case above; "small": the fixtures' case (rmsnorm_ref.VIT_CASE under RMSNorm, lora_ref.CASE under LayerNorm)."""
    if which == "tile":
        return VIT_TILE_CASE
    return R.VIT_CASE if norm == "rmsnorm" else lora_ref.CASE


def vit_case_params(case, shapes):
    """Values by seed from O.make_vit_params, the adapters scaled as lora_ref.case_params scales them."""
    p = O.make_vit_params(shapes, case["seed"])
    for k in p:
        if k.endswith("lora_matrix_A"):
            p[k] = p[k] * 50.0
        if k.endswith("lora_matrix_B"):
            p[k] = p[k] * 0.25
    return p


def vit_case_input(case):
    n = case["batch"] * case["in_chans"] * case["img_size"] ** 3
    return torch.from_numpy(O.hash_uniform(n, case["x_seed"]).astype(np.float32)).view(case["batch"], case["in_chans"], *[case["img_size"]] * 3)


def vit_tokens(p, x, case, norm: str, emulate_bf16: bool = False):
    """ViT.forward (vit.py:144-173) in the dtype of its arguments, LayerNorm or RMSNorm, the adapters when the state dict holds them,
    and the bf16 path's rounding points under `emulate_bf16`: the patch embedding's operands and output, the blocks' (O._block /
    lora_ref.block) and the final normalisation's output, which the plan stores in the compute dtype."""
    rms = norm == "rmsnorm"
    p = R.NoNormBias(p) if rms else p
    old_emu, old_block, old_ln = O._EMU[0], O._block, O._layer_norm
    O._EMU[0], O._block = bool(emulate_bf16), lora_ref.block
    if rms:
        O._layer_norm = R.rms_norm
    try:
        B = x.shape[0]
        pe = "patch_embedding.patch_embeddings"
        tok = F.conv3d(O._r(x), O._r(p[pe + ".weight"]), p[pe + ".bias"], stride=case["patch_size"])
        tok = O._r(tok.flatten(2).transpose(-1, -2)) + p["patch_embedding.position_embeddings"]
        h = torch.cat((p["cls_token"].expand(B, -1, -1), p["register_tokens"].expand(B, -1, -1), tok), dim=1)
        for i in range(case["num_layers"]):
            h = O._block(p, f"blocks.{i}", h, case["num_heads"], None, "")
        if rms:
            return O._r(R.rms_norm(h, p["norm.weight"]))
        return O._r(F.layer_norm(h, (h.shape[-1],), p["norm.weight"], p["norm.bias"], 1e-6))
    finally:
        O._EMU[0], O._block, O._layer_norm = old_emu, old_block, old_ln


class VitRef:
    """One encoder-only case: loss = lora_ref.case_loss on the tokens; gradients of the trainable tensors only."""

    def __init__(self, which, norm, lora, shapes):
        self.case, self.norm, self.lora = vit_case(which, norm), norm, lora
        self.params = vit_case_params(self.case, shapes)
        self.x = vit_case_input(self.case)
        self.trainable = [k for k in self.params if (lora_ref.trainable(k) if lora else True)]
        self._runs, self._y = {}, {}

    def run(self, precision: str, emulate: bool = False):
        key = (precision, emulate)
        if key not in self._runs:
            dt = torch.float64 if precision == "f64" else torch.float32
            p = {k: v.to(dt).clone().requires_grad_(k in self.trainable) for k, v in self.params.items()}
            tok = vit_tokens(p, self.x.to(dt), self.case, self.norm, emulate)
            loss = lora_ref.case_loss(tok)
            loss.backward()
            assert tok.dtype == dt and all(p[k].grad.dtype == dt for k in self.trainable), "the restatement left its precision"
            self._runs[key] = dict(loss=loss.detach(), tokens=tok.detach(), grads={k: p[k].grad for k in self.trainable})
        return self._runs[key]

    def reference(self, mode: str):
        return self.run("f64", mode == "bf16")

    def yardstick(self, mode: str):
        if mode not in self._y:
            a, b = (self.run("f32"), self.run("f64")) if mode == "fp32" else (self.run("f64", True), self.run("f64"))
            y = {k: E(a["grads"][k], b["grads"][k]) for k in b["grads"]}
            y["loss"] = E(a["loss"], b["loss"])
            y["act:tokens"] = E_rows(a["tokens"], b["tokens"])
            self._y[mode] = y
        return self._y[mode]


def vit_ref(which, norm, lora, shapes) -> VitRef:
    key = ("vit", which, norm, lora)
    if key not in _REF:
        _REF[key] = VitRef(which, norm, lora, shapes)
    return _REF[key]


# ---- the check -------------------------------------------------------------------------------------------------------------------
def ratios(got: dict, want: dict, yard: dict):
    """{name: (E / Y, E, Y, family, slice)} for every tensor of `want`; a name of `yard` that starts with "act:" is measured on rows."""
    out = {}
    for k, o in want.items():
        if k.startswith("act:"):
            e, fam, idx = E_rows(got[k], o), "rows", -1
        else:
            e, fam, idx = E_where(got[k], o)
        y = yard[k]
        out[k] = (e / y if y > 0 else (0.0 if e == 0 else float("inf")), e, y, fam, idx)
    return out


def worst(rs: dict):
    k = max(rs, key=lambda n: rs[n][0])
    return (k,) + rs[k]


# ---- planted faults ----------------------------------------------------------------------------------------------------------------
def _typical(size: torch.Tensor) -> int:
    """Index of the median of the non-zero entries of `size`: a typical slice, neither the easiest nor the hardest to see."""
    nz = (size > 0).nonzero().flatten()
    assert nz.numel() > 0, "nothing to plant a fault in"
    order = size[nz].argsort()
    return int(nz[order[(nz.numel() - 1) // 2]])


def fault_row(per_sample_last: torch.Tensor) -> int:
    """The row the row faults act on, chosen from the reference alone: among the rows that the LAST sample contributes to (for the
    position table: the patches that sample kept) the one whose contribution has the median norm, so that `row_lacks_sample` is a
    non-zero fault wherever the sample reaches the tensor."""
    c = view2d(per_sample_last)
    return _typical(c.abs() if c.dim() == 1 else c.norm(dim=1))


def weakest_row(per_sample_last: torch.Tensor) -> int:
    """Among the rows the last sample contributes to, the one it contributes least to: the hardest `row_lacks_sample` to see."""
    c = view2d(per_sample_last)
    n = c.abs() if c.dim() == 1 else c.norm(dim=1)
    return int(torch.where(n > 0, n, torch.full_like(n, float("inf"))).argmin())


def plant(kind: str, grad: torch.Tensor, per_sample, row=None):
    """A faulted float64 copy of `grad` (its shape kept).  `per_sample`: the samples' contributions to `grad` (they sum to it).  A
    vector is treated as D rows of one element, so its one column is the vector itself.  Every index is chosen from the reference
    (`per_sample`, whose sum is the reference gradient), never from `grad`.
        row_lacks_sample      one row misses the last sample's contribution (one volume left out of a batch reduction)
        element_lacks_sample  one element of that row (the one with the median contribution) misses it
        column_halved         the column of median norm x 0.5 (a column sum folded from half of its partials)
        tail_rows_scaled      the last 16 rows x 0.98 (a tile tail)
        rows_swapped          two neighbouring rows swapped, the pair whose difference is the median one (a row map off by one)
    `row` overrides the row of the first two kinds and the first row of the swapped pair."""
    g2 = view2d(grad).clone()
    vec = g2.dim() == 1
    g = g2.reshape(-1, 1) if vec else g2
    last = view2d(per_sample[-1]).reshape(g.shape)
    ref = sum(view2d(p) for p in per_sample).reshape(g.shape)
    r = fault_row(per_sample[-1]) if row is None else int(row)
    if kind == "row_lacks_sample":
        g[r] -= last[r]
    elif kind == "element_lacks_sample":
        c = _typical(last[r].abs())
        g[r, c] -= last[r, c]
    elif kind == "column_halved":
        g[:, _typical(ref.norm(dim=0))] *= 0.5
    elif kind == "tail_rows_scaled":
        g[-16:] *= 0.98
    elif kind == "rows_swapped":
        if row is None:
            r = _typical((ref[1:] - ref[:-1]).norm(dim=1))
        g[[r, r + 1]] = g[[r + 1, r]]
    else:
        raise ValueError(kind)
    return g.reshape(grad.shape)
