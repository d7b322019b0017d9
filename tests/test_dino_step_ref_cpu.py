"""The check checks (no GPU): tests/dino_step_ref.py's restatement of the DINO step, its inputs, yardsticks and margins.

The fp32 CPU run of the restatement stands in for the device, as in tests/test_step_ref_cpu.py.  What is shown:
  * the restatement agrees with what is already pinned: dino_oracle.dino_step at 1e-12 in float64 and tests/golden/dino.json["step"] at
    the bars of test_dino_step_vs_reference_fixture, and each helper restated in the caller's dtype agrees with its float64 original;
  * the inputs meet the conditions a comparison needs (every yardstick > 0, every row and column of every gradient non-zero except the
    slices that are mathematically zero, live GELUs, KoLeo neighbours that the bf16 stores do not overturn);
  * per-sample contributions sum to the batch gradient in the plain setting;
  * the stand-in passes at the start margins (the bf16-storage run in fp32 against itself in fp64 at 2 x Ybf, the zero tensors within
    their absolute bounds);
  * in fp32 mode every step_ref.FAULTS kind fails the bound on each of TENSORS at the margin in force and at the cap; in bf16 mode
    `column_halved` and `rows_swapped` do;
  * faults of these kinds pass the bars the DINO step was held to until now (one relative L2 per tensor, 1e-3 in fp32 and 5e-2 in bf16);
  * two faults of this step's own: the KoLeo gradient missing, the iBOT rows one row off.
What bf16 mode does NOT promise (E / Ybf over the seven tensors, `tile16` | `tile15` | `small`): `row_lacks_sample` 1.6 to 13.9 | 1.6 to
11.4 | 1.5 to 40, `element_lacks_sample` 0.26 to 6.7 | 0.45 to 6.0 | 0.94 to 39, `tail_rows_scaled` 0.46 to 0.89 | 0.56 to 0.96 | 0.72 to
1.2 -- one sample of four or five in one row, one element of a 768-wide slice or 2 % of 16 rows can be less than what the forward's bf16
stores cost that slice.  fp32 mode is where those are caught (>= 370 x Y32).  Promised and asserted: `column_halved` 7.0 to 35 and
`rows_swapped` 4.3 to 85.
"""
import json
import os

import numpy as np
import pytest
import torch

from oracle import dino_oracle as D
from oracle import mae_oracle as O
from tests import dino_step_ref as R
from tests import dino_v2_ref as V
from tests import ibot_ref as IR
from tests import step_ref as S
from tests.dropout_ref import Ones
from tests.util import GOLDEN, rel_err, sample_of

CASES = list(R.CASES)
TENSORS = ("head.mlp.0.weight", "head.mlp.4.weight", "head.last_layer.weight_v", "backbone.blocks.0.mlp.linear1.weight",
           "backbone.patch_embedding.position_embeddings", "backbone.blocks.0.attn.proj.bias", "backbone.cls_token")
ALL = [(c, s) for c in CASES for s in R.SETTINGS]


def _ids(cs):
    return f"{cs[0]}-{cs[1]}"


def test_margins_are_within_their_caps():
    assert R.START_M32 == 4.0 <= R.M32_DINO <= R.M32_DINO_CAP == 256.0 and R.START_MBF == 2.0 <= R.MBF_DINO <= R.MBF_DINO_CAP == 4.0


def test_the_measure_is_step_refs():
    assert R.E is S.E and R.E_rows is S.E_rows and R.ratios is S.ratios and R.worst is S.worst and R.plant is S.plant


# ---- agreement with what is already pinned ---------------------------------------------------------------------------------------------------
def test_helpers_agree_with_their_float64_originals():
    g = torch.Generator().manual_seed(5)
    t = torch.randn(6, 1028, generator=g, dtype=torch.float64)
    lc, lr, log_n = R.sk_logs(t, 0.04, 3, n_total=11)
    wc, wr, wn = IR.sk_logs(t, 0.04, 3, n_total=11)
    assert rel_err(lc, wc) < 1e-12 and rel_err(lr, wr) < 1e-12 and log_n == wn
    q, _, _ = V.sk_log(t, 0.04, 3)
    assert rel_err(R.teacher_q(t, 0.04, sk_iters=3), q) < 1e-12
    s = torch.randn(12, 1028, generator=g, dtype=torch.float64).requires_grad_(True)
    loss = R.dino_from_q(s, q, 4, 0.1)
    loss.backward()
    want, dwant = V.dino_loss_from_q(s.detach(), q, 4, 0.1)
    assert abs(float(loss) - float(want)) < 1e-12 * abs(float(want)) and rel_err(s.grad, dwant) < 1e-12
    x = V.koleo_inputs(7, 64, 3).double().requires_grad_(True)
    loss, idx, margin, _ = R.koleo(x)
    loss.backward()
    want, dx, widx, _, wmargin = V.koleo(x.detach())
    assert abs(float(loss) - float(want)) < 1e-12 and torch.equal(idx, widx) and margin == pytest.approx(wmargin, rel=1e-9) and rel_err(x.grad, dx) < 1e-12


def test_backbone_and_head_agree_with_the_existing_restatements():
    """`tokens` is step_ref.vit_tokens bit for bit without masks (plain and emulating) and ibot_ref.vit_forward_masked with them (plain;
    under the emulation that one rounds the dropout path's two extra stores); `head_forward` without the emulation is
    dino_oracle.dino_head_forward, with and without BatchNorm."""
    ref = R.dino_ref("small", "ibot-ragged")
    vit = ref.vit
    p = {k: v.double() for k, v in ref.sb.items()}
    x = torch.cat(ref.crops[:2]).double()
    plain = {k: v for k, v in p.items() if k != "mask_token"}
    for emulate in (False, True):
        assert torch.equal(R.tokens(plain, x, vit, None, emulate), S.vit_tokens(plain, x, vit, "layernorm", emulate))
    mask = torch.from_numpy(ref.masks).bool()
    want = IR.vit_forward_masked(p, x, mask, vit["patch_size"], vit["num_heads"], vit["num_layers"], Ones())
    got = R.tokens(p, x, vit, mask, False)
    assert rel_err(got, want) < 1e-12 and rel_err(got, R.tokens(p, x, vit, None, False)) > 1e-2
    rows = torch.randn(10, vit["hidden_size"], dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    for use_bn in (False, True):
        hp = {k: (v.double() if v.is_floating_point() else v) for k, v in R.make_head_params_scaled(vit["hidden_size"], ref.head, 7, use_bn).items()}
        a, b = {k: v.clone() for k, v in hp.items()}, {k: v.clone() for k, v in hp.items()}
        assert rel_err(R.head_forward(a, rows), D.dino_head_forward(b, rows)) < 1e-12
        assert all(torch.equal(a[k], b[k]) for k in a)  # (the running statistics moved alike)


def _fixture_ref():
    fx = json.load(open(os.path.join(GOLDEN, "dino.json")))["step"]
    assert {k: fx["vit"][k] for k in R._SMALL_VIT} == R._SMALL_VIT and fx["crops"] == 4 and fx["batch"] == 2
    hk = fx["head"]
    assert (hk["hidden_dim"], hk["bottleneck_dim"], hk["out_dim"]) == (64, 32, 128)
    shapes = R.backbone_shapes(R._SMALL_VIT)
    assert sorted(shapes) == sorted(fx["backbone_keys"])
    S_ = fx["vit"]["img_size"]
    params = dict(student_backbone=O.make_vit_params(shapes, seed0=fx["backbone_seed"][0]), teacher_backbone=O.make_vit_params(shapes, seed0=fx["backbone_seed"][1]),
                  student_head=D.make_head_params(hk["in_dim"], hk["out_dim"], hk["hidden_dim"], hk["bottleneck_dim"], fx["head_seed"][0]),
                  teacher_head=D.make_head_params(hk["in_dim"], hk["out_dim"], hk["hidden_dim"], hk["bottleneck_dim"], fx["head_seed"][1]),
                  crops=[R.hu((2, 3, S_, S_, S_), fx["crop_seed0"] + i, 0.0, 1.0) for i in range(4)], center=R.hu((1, hk["out_dim"]), fx["center_seed"], -0.2, 0.2))
    return fx, params, R.DinoRef("small", params=params, freeze_last_layer=False)


def test_plain_setting_agrees_with_dino_oracle_and_the_fixture():
    fx, p, ref = _fixture_ref()
    assert fx["teacher_temp"] == R.TEACHER_TEMP
    run = ref.run("f64")
    d = lambda t: {k: v.double() for k, v in t.items()}
    loss, gb, gh, center = D.dino_step(d(p["student_backbone"]), d(p["student_head"]), d(p["teacher_backbone"]), d(p["teacher_head"]),
                                       [c.double() for c in p["crops"]], p["center"].double(), patch=ref.vit["patch_size"], heads=ref.vit["num_heads"],
                                       layers=ref.vit["num_layers"], student_temp=R.STUDENT_TEMP, teacher_temp=R.TEACHER_TEMP, freeze_last_layer=False)
    assert abs(float(run["losses"]["loss"]) - float(loss)) < 1e-12 * abs(float(loss))
    want = {"backbone." + k: v for k, v in gb.items()}
    want.update({"head." + k: v for k, v in gh.items()})
    assert set(want) == set(run["grads"])
    for k, o in want.items():
        if k.endswith("qkv.bias"):  # (the K third is round-off in both)
            assert float((run["grads"][k] - o).abs().max()) < 1e-12 * float(o.abs().max()), k
        else:
            assert rel_err(run["grads"][k], o) < 1e-12, (k, rel_err(run["grads"][k], o))
    assert rel_err(run["centers"]["center"], center) < 1e-12
    # the fixture (the reference project's own modules), at the fp32 bars of test_dino_step_vs_reference_fixture
    assert abs(float(run["losses"]["loss"]) - fx["loss"]) < 2e-5 * abs(fx["loss"])
    _, _, l2, l2w = sample_of(run["acts"]["logits"], fx["logits"])
    assert abs(l2 - l2w) < 1e-4 * l2w
    frozen = R.DinoRef("small", params=p, freeze_last_layer=True, runs=ref._runs)
    assert set(frozen.grad_names()) == set(fx["grads"])
    for k, entry in fx["grads"].items():
        got, want_s, l2, l2w = sample_of(run["grads"][k], entry)
        assert abs(l2 - l2w) <= 1e-3 * l2w + 1e-12, k
        assert torch.allclose(got, want_s, rtol=0.0, atol=1e-6 + 2e-3 * float(want_s.abs().max())), k
    got, want_s, _, _ = sample_of(run["centers"]["center"], fx["center_after"])
    assert torch.allclose(got, want_s, rtol=1e-3, atol=1e-5)


def test_the_fixtures_head_initialiser_is_dead_at_the_yaml_width():
    """Why this file has an initialiser of its own: with dino_oracle.make_head_params (matrices in [-0.6, 0.2), mean -0.2) at hidden 2048
    every input of the head's second GELU lies below -6, the loss does not depend on the matrices, and the float64 gradient is exactly
    zero from mlp.4.weight back through the whole backbone: a step test on those parameters would compare zeros with zeros."""
    ref = R.dino_ref("tile16", "plain", freeze_last_layer=False)
    h = ref.head
    heads = [D.make_head_params(768, h["out_dim"], h["hidden_dim"], h["bottleneck_dim"], seed) for seed in (5, 9)]
    assert -0.21 < float(heads[0]["mlp.2.weight"].mean()) < -0.19
    dead = R.DinoRef("tile16", params=dict(student_backbone=ref.sb, teacher_backbone=ref.tb, crops=ref.crops, center=ref.center0, student_head=heads[0],
                                           teacher_head=heads[1]), freeze_last_layer=False).run("f64")
    assert float((dead["gelu_in"][1] < -6.0).double().mean()) == 1.0
    alive = {k for k, g in dead["grads"].items() if float(g.abs().max()) > 0}
    assert alive == {"head.mlp.4.bias", "head.last_layer.weight_v"}, alive


# ---- conditions on the inputs ----------------------------------------------------------------------------------------------------------------
def _exempt(ref, name, n):
    """Slices that are zero in exact arithmetic, by name: bool [n] (True = exempt)."""
    out = torch.zeros(n, dtype=torch.bool)
    if name in ref.zero_names():
        out[:] = True
    if name.endswith("attn.qkv.bias"):  # the K third: the softmax does not see a bias of the keys
        out[n // 3:2 * n // 3] = True
    return out


@pytest.mark.parametrize("cs", ALL, ids=_ids)
def test_input_conditions(cs):
    ref = R.dino_ref(*cs, freeze_last_layer=False)
    run, emu = ref.run("f64"), ref.run("f64", True)
    for mode in ("fp32", "bf16"):
        y = ref.yardstick(mode)
        assert all(0 < v < float("inf") for v in y.values()), (mode, {k: v for k, v in y.items() if not 0 < v < float("inf")})
        assert set(y) == set(ref.flat(ref.reference(mode), "fp32"))
        # a yardstick of order 1 says that the format alone changes the tensor completely: twice that would hold nothing
        assert all(v < 0.5 for k, v in y.items()), (mode, {k: v for k, v in y.items() if not v < 0.5})
    for name, g in run["grads"].items():
        g2 = S.view2d(g)
        if g2.dim() == 1:
            ex, norms = _exempt(ref, name, g2.numel()), {"elems": g2.abs()}
        else:
            assert name not in ref.zero_names()
            ex, norms = None, {"rows": g2.norm(dim=1), "cols": g2.norm(dim=0)}
        scale = float(max(S.view2d(v).abs().max() for v in run["grads"].values()))
        for fam, n in norms.items():
            live = n if ex is None else n[~ex]
            assert live.numel() == 0 or float(live.min()) > 1e-10 * float(n.max()) > 0, (name, fam, "a zero slice", int(n.argmin()))
            if ex is not None:
                assert bool((n[ex] < 1e-12 * scale).all()), (name, fam, "a slice listed as mathematically zero is not")
    for u in run["gelu_in"] + emu["gelu_in"]:
        assert float((u < -6.0).double().mean()) < 0.01, "a dead GELU layer"
    if ref.koleo_weight > 0:
        assert len(run["nn_idx"]) == 2 and all(torch.equal(a, b) for a, b in zip(run["nn_idx"], emu["nn_idx"])), "the bf16 stores changed a nearest neighbour"
        shift = max(float((a - b).abs().max()) for a, b in zip(run["nn_dots"], emu["nn_dots"]))
        print(_ids(cs), "KoLeo: smallest best-minus-second cosine", run["nn_margin"], emu["nn_margin"], "largest move of a cosine under the bf16 stores", shift)
        assert min(run["nn_margin"], emu["nn_margin"]) > 4.0 * shift
    if ref.ibot_weight > 0:
        counts = ref.masks.sum(axis=1)
        total = ref.V * ref.B + int(counts.sum())
        assert counts[0] == 0 and counts[1] == 1 and (total % 16 == 0) == (cs[1].endswith("exact")), (counts, total)
        assert all(ref.masks.shape[1] / 4.0 <= c <= ref.masks.shape[1] / 2.0 for c in counts[2:]), "about a third"


def test_cases_take_both_dgrad_routes_and_cross_the_loss_chunks():
    for name, rows16 in (("tile16", True), ("tile15", False)):
        c = R.CASES[name]
        assert ((c["crops"] * c["batch"]) % 16 == 0) == rows16 and c["head"]["bottleneck_dim"] % 16 == 0
        assert c["head"]["out_dim"] > 4 * IR.LOSS_CHUNK and c["head"]["out_dim"] % IR.LOSS_CHUNK == 4
    assert R.CASES["small"]["crops"] * R.CASES["small"]["batch"] == 8


@pytest.mark.parametrize("case", CASES)
def test_per_sample_contributions_sum_to_the_batch_gradient(case):
    ref = R.dino_ref(case, "plain", freeze_last_layer=False)
    grads, per = ref.run("f64")["grads"], ref.per_sample()
    assert len(per) == ref.B
    for k, g in grads.items():
        if k.endswith("qkv.bias"):
            assert float((sum(p[k] for p in per) - g).abs().max()) < 1e-12 * float(g.abs().max()), k
        else:
            assert rel_err(sum(p[k] for p in per), g) < 1e-12, k


# ---- the stand-in ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cs", ALL, ids=_ids)
def test_stand_in_passes_at_the_start_margins(cs):
    ref = R.dino_ref(*cs, freeze_last_layer=False)
    rs = R.ratios(ref.flat(ref.run("f32"), "fp32"), ref.flat(ref.run("f64"), "fp32"), ref.yardstick("fp32"))
    assert R.worst(rs)[1] <= R.START_M32, R.worst(rs)
    e32, e64 = ref.run("f32", True), ref.run("f64", True)
    # (gradients only, as in test_step_ref_cpu: under the emulation fp32 noise flips single bf16 roundings, and a scalar's yardstick is one draw)
    names = [k for k in ref.grad_names() if k not in ref.zero_names()]
    rs = R.ratios({k: e32["grads"][k] for k in names}, {k: e64["grads"][k] for k in names}, ref.yardstick("bf16"))
    print(_ids(cs), "bf16-storage run, fp32 against fp64: worst E / Ybf", R.worst(rs)[:2])
    assert R.worst(rs)[1] <= R.START_MBF, R.worst(rs)
    for mode, run in (("fp32", ref.run("f32")), ("bf16", e32)):
        for k, bound in ref.zero_bias_bounds(mode).items():
            g = run["grads"][k].double().abs()
            assert bool((g <= bound).all()), (mode, k, float(g.max()))
            assert float(torch.as_tensor(bound).min()) > 0


# ---- planted faults --------------------------------------------------------------------------------------------------------------------------
def _planted(ref, mode, name, kind, row=None):
    """(faulted stand-in, stand-in, reference, yardstick) of one tensor."""
    stand_in = ref.run("f32", mode == "bf16")["grads"][name]
    per = [p[name] for p in ref.per_sample()]
    return R.plant(kind, stand_in, per, row=row), stand_in, ref.reference(mode)["grads"][name], ref.yardstick(mode)[name]


@pytest.mark.parametrize("case", CASES)
def test_fp32_mode_catches_every_planted_fault(case):
    ref = R.dino_ref(case, "plain", freeze_last_layer=False)
    for name in TENSORS:
        for kind in S.FAULTS:
            planted, stand_in, want, y = _planted(ref, "fp32", name, kind)
            assert bool((planted != stand_in.double()).any()), (name, kind, "nothing planted")
            e = R.E(planted, want)
            assert e > R.M32_DINO * y and e > R.M32_DINO_CAP * y, (name, kind, e / y)


@pytest.mark.parametrize("case", CASES)
def test_bf16_mode_catches_halved_columns_and_swapped_rows(case):
    ref = R.dino_ref(case, "plain", freeze_last_layer=False)
    seen = {}
    for name in TENSORS:
        for kind in S.FAULTS:
            planted, stand_in, want, y = _planted(ref, "bf16", name, kind)
            e = R.E(planted, want)
            seen[(name, kind)] = e / y
            if kind in ("column_halved", "rows_swapped"):
                assert bool((planted != stand_in.double()).any()), (name, kind, "nothing planted")
                assert e > R.MBF_DINO * y and e > R.MBF_DINO_CAP * y, (name, kind, e / y)
    for kind in S.FAULTS:
        vals = [v for (n, k), v in seen.items() if k == kind]
        print(f"{case} bf16 mode {kind}: E / Ybf {min(vals):.3g} to {max(vals):.3g}")


def _row_under_bar(ref, name, bar):
    """The row whose loss of the last sample is the LARGEST single-row fault that one relative L2 per tensor at `bar` lets through."""
    last = S.view2d(ref.per_sample()[-1][name])
    share = last.norm(dim=1) / S.view2d(ref.run("f64")["grads"][name]).norm()
    return int(torch.where(share < 0.75 * bar, share, torch.zeros_like(share)).argmax())


@pytest.mark.parametrize("case", ["tile16", "tile15"])
def test_faults_that_one_l2_per_tensor_accepts(case):
    """The gap being closed.  fp32: on head.mlp.0.weight (2048 x 768), head.last_layer.weight_v (4100 x 256) and the backbone's
    linear1.weight (3072 x 768), a row that lacks one sample and an element that lacks one pass rel_err < 1e-3 against the fp32 run --
    the bar of test_dino_step_vs_reference_fixture -- and fail the new bound at its cap.  bf16: two swapped rows and a halved column of
    the same tensors pass that test's 5e-2 and fail at the cap."""
    ref = R.dino_ref(case, "plain", freeze_last_layer=False)
    for name in ("head.mlp.0.weight", "head.last_layer.weight_v", "backbone.blocks.0.mlp.linear1.weight"):
        o32 = ref.run("f32")["grads"][name]
        for kind, row in (("row_lacks_sample", _row_under_bar(ref, name, 1e-3)), ("element_lacks_sample", None)):
            planted, _, want, y = _planted(ref, "fp32", name, kind, row=row)
            old, new = rel_err(planted, o32), R.E(planted, want) / y
            print(f"{case} {name} fp32 {kind}: per-tensor L2 {old:.2e} (bar 1e-3), E / Y32 {new:.0f}")
            assert 0 < old < 1e-3 and new > R.M32_DINO_CAP >= R.M32_DINO
        for kind in ("rows_swapped", "column_halved"):
            planted, _, want, y = _planted(ref, "bf16", name, kind)
            old, new = rel_err(planted, o32), R.E(planted, want) / y
            print(f"{case} {name} bf16 {kind}: per-tensor L2 {old:.2e} (bar 5e-2), E / Ybf {new:.1f}")
            assert 0 < old < 5e-2 and new > R.MBF_DINO_CAP >= R.MBF_DINO


# ---- two faults of this step's own ---------------------------------------------------------------------------------------------------------------
def _worst_over_grads(ref, mode, got):
    names = [k for k in ref.grad_names() if k not in ref.zero_names()]
    want = ref.reference(mode)["grads"]
    return R.worst(R.ratios({k: got[k] for k in names}, {k: want[k] for k in names}, ref.yardstick(mode)))


@pytest.mark.parametrize("case", CASES)
def test_a_missing_koleo_gradient_fails(case):
    """The stand-in's gradients are those of the koleo_weight = 0 run (autograd's add at the class-token rows left out): every backbone
    tensor moves, the head's do not."""
    ref, plain = R.dino_ref(case, "koleo", freeze_last_layer=False), R.dino_ref(case, "plain", freeze_last_layer=False)
    for mode, cap in (("fp32", R.M32_DINO_CAP), ("bf16", R.MBF_DINO_CAP)):
        got = ref._step(torch.float32, mode == "bf16", koleo_weight=0.0)["grads"]
        same = plain.run("f32", mode == "bf16")["grads"]
        assert all(torch.equal(got[k], same[k]) for k in got), "the fault is the plain run's gradients"
        w = _worst_over_grads(ref, mode, got)
        print(f"{case} {mode} KoLeo gradient missing: worst E / Y {w[1]:.3g} ({w[0]})")
        assert w[0].startswith("backbone.") and w[1] > cap
        rs = R.ratios({k: got[k] for k in got if k.startswith("backbone.") and k not in ref.zero_names()},
                      {k: v for k, v in ref.reference(mode)["grads"].items() if k.startswith("backbone.")}, ref.yardstick(mode))
        if mode == "fp32":
            assert all(r[0] > cap for r in rs.values()), {k: r[0] for k, r in rs.items() if not r[0] > cap}


@pytest.mark.parametrize("setting", ["ibot-ragged", "ibot-sk-exact"])
@pytest.mark.parametrize("case", CASES)
def test_ibot_rows_one_row_off_fail(case, setting):
    """The student gathers, and scatters its gradient back to, row r + 1 for every masked row r whose successor is still a patch row of
    the same sample."""
    ref = R.dino_ref(case, setting, freeze_last_layer=False)
    T1 = 1 + ref.vit["num_register_tokens"] + R.num_patches(ref.vit)
    rows, _ = IR.rows_and_weights(ref.masks, ref.vit["num_register_tokens"])
    off = np.where((rows + 1) % T1 != 0, rows + 1, rows)
    assert (off != rows).sum() >= len(rows) - 2 * ref.B and bool(((off % T1) > ref.vit["num_register_tokens"]).all())
    for mode, cap in (("fp32", R.M32_DINO_CAP), ("bf16", R.MBF_DINO_CAP)):
        got = ref._step(torch.float32, mode == "bf16", student_rows=off)["grads"]
        w = _worst_over_grads(ref, mode, got)
        m = R.ratios({"backbone.mask_token": got["backbone.mask_token"]}, {"backbone.mask_token": ref.reference(mode)["grads"]["backbone.mask_token"]},
                     ref.yardstick(mode))["backbone.mask_token"][0]
        print(f"{case} {setting} {mode} iBOT rows one off: worst E / Y {w[1]:.3g} ({w[0]}), mask_token {m:.3g}")
        assert w[1] > cap and m > cap
