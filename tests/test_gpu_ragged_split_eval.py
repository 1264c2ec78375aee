"""The fp32-level fused eval plan on ragged maps, Settings(fused_eval="fp16x2+ragged") (onet_amd/inference.py).

The helpers, recipes and bounds of tests/test_gpu_fused_eval.py, used as they stand: every output within TOL = 2e-4 of its tensor's
largest magnitude against the fp64 oracle, labels equal where the fp64 margin exceeds MARGIN = 1e-3 (those pixels more than 0.9 of
all), every traced slot tensor under the bound it was scaled by, and the trace and the launch records following the plan dictionary.
The oracle of each recipe runs once per session.  Both inputs meet the margin share with the oracle alone (run on the host before the
seeds were fixed: 0.9943 at 2 x 1 x 48 x 80, seed 201; 0.9944 at 1 x 3 x 224 x 224, seed 202).

Labels-only calls: scores / segment(head="fused") / validate against the forward of the same model.  The fp16 HEAD instance runs
the 16x16x32 main loop, the forward's plain launch the 32x32x16 one, so the bound is the one tests/test_gpu_fused_head.py derives for
that instance (K2), per pixel: the 64-term dot-product bound of both forms, 2.1 x 66 u |V| (L, h >= 0), plus the accumulation-order
term sum_c |L_c| |sc_c| 2 (27 Cin) u (|x| * |w|)_c."""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import onet_oracle as orc
import test_gpu_fused_eval as fe
import test_gpu_fused_head as fh
from test_gpu_fused_eval import dev  # noqa: F401  (the module-scoped fixture)

pytestmark = pytest.mark.gpu

VALUE = "fp16x2+ragged"
UNAMES = ("up4", "up3", "up2", "up1")
_RUNS = {}


def _traced_run(m, Xg):
    """one forward with inference.TRACE on -> (outputs, {kind: launches}, [traced names], fe._traced's rows, {name: [(slots, guard
    exponent, copies of the scale and amax magnitude slots) per pass]}) -- copies: the slots live in an arena the next forward reuses"""
    from onet_amd import inference, ops
    inference.TRACE = []
    ops.profile_start(everything=False)
    try:
        with torch.no_grad():
            out = m(Xg)
        torch.cuda.synchronize()
        names, rows, tensors = [], [], {}
        for name, t in inference.TRACE:
            bound = fe._slot_max(t.scale)
            k = 13 - math.floor(math.log2(bound)) if bound >= 2.0 ** 15 else 0        # the guard exponent the slots select
            names.append(name)
            rows.append((name, bound, float(t.P.float().sum(3).abs().max()) * 2.0 ** -k))
            tensors.setdefault(name, []).append((t.P, k, t.scale.clone(), t.amax.clone()))
    finally:
        kinds = {k: len(v) for k, v in ops.profile_stop()[0].items()}
        inference.TRACE = None
    return out, kinds, names, rows, tensors


def _run(dev, B, C, H, W, share, bias, seed):
    """model, oracle, plan and one traced forward of a recipe under conv = "split" and the new value -- built once"""
    import onet_amd
    from onet_amd import ops
    key = (B, C, H, W, share, bias, seed)
    if key not in _RUNS:
        X = orc.det_input(B, C, H, W, seed=seed)
        top = fe._calibrated(orc.det_state_dict(C, 1981), X, bias)
        dwn = None if share else fe._calibrated(orc.det_state_dict(C, 1982), X, bias)
        ref = fe._oracle(X, top, dwn, bias)
        m = fe._onet(fe._prefixed(top, dwn), C, share, dev)
        m.bias = bias
        m.settings = ops.Settings(conv="split", fused_eval=VALUE)
        Xg = X.to(dev)
        plan = onet_amd.fused_eval_plan(m, Xg.shape)
        out, kinds, names, rows, tensors = _traced_run(m, Xg)
        _RUNS[key] = dict(X=X, Xg=Xg, ref=ref, m=m, plan=plan, out=out, kinds=kinds, names=names, rows=rows, tensors=tensors,
                          passes=1 if share else 2)
    return _RUNS[key]


def _check_run(r, d, convt, what):
    """the plan dictionary, then the executor against it (trace order, launch records), the outputs against the oracle and every
    traced tensor against its bound"""
    plan, kinds, passes = r["plan"], r["kinds"], r["passes"]
    assert plan["fused"] and plan["depth"] == d and plan["operands"] == "fp16x2" and plan["twin"] == (passes == 1), plan
    assert plan["convt"] == dict(zip(UNAMES, convt)), plan
    for n, v in plan["layers"].items():
        blk = n.split(".")[0]
        level = fe_level(blk)
        want = "fallback" if level >= d else "stem" if n == "inc.c1" else "plain+head" if n == "up4.c2" else \
            "fused+pool" if (n.endswith(".c2") and blk in ("inc", "down1", "down2", "down3")) else "fused"
        assert v == want, (n, v, want)
    n_of = {k: sum(1 for v in plan["layers"].values() if v == k) for k in ("fused", "fused+pool", "plain+head")}
    assert r["names"] == fe._slot_writers(plan) * passes, (what, r["names"], fe._slot_writers(plan))
    assert kinds.get("conv3x3_split_pre_act_kernel", 0) == passes * n_of["fused"] > 0, (what, kinds, plan)
    assert kinds.get("conv3x3_split_pre_act_pool_kernel", 0) == passes * n_of["fused+pool"] > 0, (what, kinds, plan)
    assert kinds.get("conv3x3_split_pre_kernel", 0) == passes * n_of["plain+head"], (what, kinds, plan)
    assert kinds.get("convt_slot_fwd_kernel", 0) == passes * sum(1 for v in plan["convt"].values() if v == "slots"), (what, kinds, plan)
    assert "conv3x3_split_kernel" not in kinds, (what, kinds)          # no fused level falls back to the in-staging kernel
    print(f"{what} worst error {fe._compare(r['m'], r['out'], r['ref'], fe.TOL, what):.2e}")
    fe._check_bounds(r["rows"], what)


def fe_level(blk):
    names = ("inc", "down1", "down2", "down3", "down4")
    return names.index(blk) if blk in names else UNAMES.index(blk)


def test_m1_ragged_levels_against_the_oracle(dev):
    """M1: Onet(1, shared) at 2 x 1 x 48 x 80 (twin batch of 4) under conv = "split": levels 48 x 80, 24 x 40 and 12 x 20 -- none made
    of full tiles -- are fused, the 6 x 10 level is the fall-back; the ConvTranspose2d of levels 0 and 1 run the two-part ragged
    slot-operand entry (960 and 240 pixels), level 2's the general kernel and one conversion pass ("fp32->slots").
    Measured on an MI355X: Lt 8.1e-7, Vt 3.5e-6, Ld 8.4e-7, Vd 3.6e-6, S 2.9e-5 (bound 2e-4); worst bound / exact maximum 5857x
    (up2.c1: two chained bounds, as on full tiles)."""
    from onet_amd import inference, ops
    r = _run(dev, 2, 1, 48, 80, True, 0.0, 201)
    _check_run(r, 3, ("slots", "slots", "fp32->slots", "fallback"), "M1 fp16 ragged")
    assert r["plan"]["batch"] == 4 and r["plan"]["fallback_reason"].startswith("level 3: down3.c1"), r["plan"]
    with ops.using(r["m"].settings):
        routes = [lv.route for lv in inference._query(r["m"].topu, (4, 1, 48, 80)).levels[:4]]
    assert routes == ["slots_ragged", "slots_ragged", "pack", None], routes


def test_m1_labels_only_calls(dev):
    """scores, segment(head="fused") and validate on the 48 x 80 input: one head-epilogue launch per pass and no plain launch; V within
    the fp16 HEAD instance's dot-product bound of the forward's V (module docstring); labels equal to predict_label(S), and to the
    oracle's labels on its margin pixels; validate's counts == the counts of segment's labels.
    Measured on an MI355X: worst |V_scores - V_out| / bound Vt 1.0e-4, Vd 1.2e-4 (the accumulation-order term is a worst case over
    27 Cin terms and dominates the bound, as in tests/test_gpu_fused_head.py K2)."""
    import onet_amd
    r = _run(dev, 2, 1, 48, 80, True, 0.0, 201)
    m, Xg, out = r["m"], r["Xg"], r["out"]
    (Vt, Vd, S), k_sc, _ = fh._mfma_kinds(lambda: onet_amd.scores(m, Xg))
    lab, k_lab, _ = fh._mfma_kinds(lambda: onet_amd.segment(m, Xg, head="fused"))
    for kk in (k_sc, k_lab):
        assert kk.get("conv3x3_split_pre_head_kernel", 0) == 1 and "conv3x3_split_pre_kernel" not in kk, kk
    p1 = onet_amd.fused_eval_plan(m, Xg.shape, head="fused")
    assert p1["layers"]["up4.c2"] == "fused+head" and p1["depth"] == 3, p1
    # the last unit's operand of the traced forward (twin batch: X, then its complement) and its coefficients, for the order term
    (P, k, _, _), = r["tensors"]["up4.c1"]
    x = fh.unsplit(P) * 2.0 ** -k
    u2 = m.topu.up4.conv.double_conv
    conv, bn = u2[3], u2[4]
    aw = F.conv2d(x.abs(), conv.weight.detach().cpu().double().abs() * (1 + 2.0 ** -21), None, 1, 1)
    sc = (bn.weight.detach().cpu().double() / torch.sqrt(bn.running_var.detach().cpu().double() + bn.eps)).abs().view(1, -1, 1, 1)
    order = sc * (2 * 27 * conv.in_channels * fh.U) * aw
    worst = {}
    for got, ref, L, half, n in ((Vt, out[1], out[0], slice(0, 2), "Vt"), (Vd, out[3], out[2], slice(2, 4), "Vd")):
        assert tuple(got.shape) == tuple(ref.shape) and torch.isfinite(got).all() and bool((ref >= 0).all()) and bool((L >= 0).all()), n
        bound = 2.1 * fh.DOT * ref.cpu().double().abs() + (L.cpu().double().abs() * order[half]).sum(1, keepdim=True) + 1e-30
        worst[n] = (got.cpu().double() - ref.cpu().double()).abs() / bound
        print(f"M1 fp16 ragged {n}: worst |V_scores - V_out| / bound = {float(worst[n].max()):.3e}")
        assert float(worst[n].max()) <= 1.0, f"{n}: {float(worst[n].max()):.3f} x the bound"
    assert lab.dtype == torch.int64 and tuple(lab.shape) == (2, 48, 80) and torch.equal(lab, m.predict_label(S))
    # labels against the oracle's on its margin pixels (fe._compare's rule)
    sure = fe._margin(r["ref"], max(fe.MARGIN, 2 * fe.TOL))
    assert float(sure.double().mean()) > 0.9
    assert torch.equal(lab.cpu()[sure], orc.predict_label(r["ref"][4]).long()[sure])
    # validate: the same scores and labels, and the counts of those labels
    gt = (orc.det_input(2, 1, 48, 80, seed=77)[:, 0] > 0.5).to(torch.uint8)
    v = onet_amd.validate(m, Xg, gt.to(Xg.device), want_labels=True)
    torch.cuda.synchronize()
    assert torch.equal(v.labels, lab) and torch.equal(v.Vt, Vt) and torch.equal(v.Vd, Vd)
    p, g = lab.cpu() != 0, gt != 0
    want = torch.stack([(p & g).sum((1, 2)), (p & ~g).sum((1, 2)), (~p & g).sum((1, 2)), (~p & ~g).sum((1, 2))], dim=1)
    assert torch.equal(v.counts.cpu(), want.to(torch.int64)), (v.counts.cpu(), want)
    assert 0 < int(want[:, 0].sum()) and 0 < int(want[:, 3].sum())


def test_m2_unshared_rgb_224_against_the_oracle(dev):
    """M2: Onet(3, unshared), bias 0.1, at 1 x 3 x 224 x 224 -- the ZY-3 thumbnails' shape -- under conv = "split": level 0 is made of
    full tiles, 112 / 56 / 28 are ragged, the 14-pixel level is the fall-back, whose output enters the 28-pixel concat buffer as
    "fp32->slots" (196 pixels: the general kernel and one conversion pass).
    Measured on an MI355X: Lt 7.3e-7, Vt 5.5e-6, Ld 7.7e-7, Vd 5.0e-6, S 4.5e-5 (bound 2e-4); worst bound / exact maximum 12988x
    (up1.c1).  (The fp64 oracle of two U-Nets at 224 x 224 on the host is most of this test's 6 s.)"""
    r = _run(dev, 1, 3, 224, 224, False, 0.1, 202)
    _check_run(r, 4, ("slots", "slots", "slots", "fp32->slots"), "M2 fp16 ragged 224")
    assert r["plan"]["batch"] == 1, r["plan"]


def test_m3_full_tiles_are_the_pooled_plan_bit_for_bit(dev):
    """M3: 4 x 1 x 256^2 -- every level the plan takes is made of full tiles (the 16-pixel level stays below the predicate's floor) --
    under the new value: the plan dictionary, the launch records, the five outputs and every traced tensor (slots and both sets of
    magnitude slots) bit-identical to "fp16x2+pool"."""
    import onet_amd
    from onet_amd import ops
    m = fe._onet(fe._prefixed(orc.det_state_dict(1, 1981)), 1, True, dev)
    Xg = orc.det_input(4, 1, 256, 256, seed=141).to(dev)
    got = {}
    for value in ("fp16x2+pool", VALUE):
        m.settings = ops.Settings(fused_eval=value)
        plan = onet_amd.fused_eval_plan(m, Xg.shape)
        out, kinds, names, _, tensors = _traced_run(m, Xg)
        got[value] = (plan, kinds, names, out, tensors)
    a, b = got["fp16x2+pool"], got[VALUE]
    assert a[0] == b[0] and b[0]["fused"] and b[0]["depth"] >= 2, (a[0], b[0])
    assert a[1] == b[1] and a[2] == b[2] and b[2], (a[1], b[1], a[2], b[2])
    assert all(torch.equal(x, y) for x, y in zip(a[3], b[3]))
    for name in a[4]:
        for (Pa, ka, sa, ma), (Pb, kb, sb, mb) in zip(a[4][name], b[4][name]):
            assert ka == kb and torch.equal(Pa.contiguous().view(torch.int16), Pb.contiguous().view(torch.int16)), name
            assert torch.equal(sa, sb) and torch.equal(ma, mb), name


def test_m4_depth_at_200(dev):
    """M4: 1 x 1 x 200 x 200 under conv = "split": levels 200 and 100 are fused, the 50-pixel level is W % 4 -- depth 2, the reason
    names W = 50 -- and the forward runs the announced launches: finite and repeatable"""
    import onet_amd
    from onet_amd import ops
    m = fe._onet(fe._prefixed(orc.det_state_dict(1, 1981)), 1, True, dev)
    st = ops.Settings(conv="split", fused_eval=VALUE)
    X = orc.det_input(1, 1, 200, 200, seed=113).to(dev)
    out, kinds = fe._eval(m, X, st)
    plan = onet_amd.fused_eval_plan(m, X.shape)
    assert plan["fused"] and plan["depth"] == 2 and "W = 50" in plan["fallback_reason"], plan
    assert "eval_layer_ok_ragged_fp16" in plan["fallback_reason"], plan
    assert plan["convt"] == dict(zip(UNAMES, ("slots", "fp32->slots", "fallback", "fallback"))), plan
    assert kinds.get("conv3x3_split_pre_act_kernel", 0) == 4 and kinds.get("conv3x3_split_pre_act_pool_kernel", 0) == 2, kinds
    assert kinds.get("conv3x3_split_pre_kernel", 0) == 1 and kinds.get("convt_slot_fwd_kernel", 0) == 1, kinds
    assert all(torch.isfinite(t).all() for t in out) and tuple(out[4].shape) == (1, 2, 200, 200)
    out2, _ = fe._eval(m, X)
    assert all(torch.equal(x, y) for x, y in zip(out, out2))
