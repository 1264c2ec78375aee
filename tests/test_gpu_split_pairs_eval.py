"""The fp32-level fused eval plan at full depth, Settings(fused_eval="fp16x2+ragged+pairs") (onet_amd/inference.py): level 4 -- down4.c1,
down4.c2 and the ConvTranspose2d of up1 -- on image-pair tiles (ops.conv3x3_split_pre_act_pairs).

The helpers and bounds of tests/test_gpu_ragged_split_eval.py (and through it tests/test_gpu_fused_eval.py) under conv = "split", used as
they stand: every output within TOL = 2e-4 of its tensor's largest magnitude against the fp64 oracle, labels equal where the fp64 margin
exceeds MARGIN = 1e-3 of max |V| (those pixels more than 0.9 of all), every traced slot tensor under the bound it was scaled by, the
trace and the launch records following the plan dictionary.  What is this file's own is the launch record of a depth-5 plan (_check_run:
two launches of the pair kind per pass, no fp32 convolution beyond the stem's) and the magnitude records of level 4: the traced bound of
down4.c1 and down4.c2 is no smaller than the exact maximum the pair launch recorded, and no looser than the full-tile plan's chained
bounds get (1.4e4 x: tests/test_gpu_ragged_split_eval.py M2 measures 12988 x) -- a test of its own per recipe
(126 x - 225 x measured; it is what made down3.c2 record its exact maximum: see its docstring).

Levels 0 - 3 need H >= 8 and W >= 20 (ops.RAGGED_MIN_W), so the recipes are the smallest shapes with a level 4 of 9 .. 16 columns.  The
margin-pixel condition of the three recipes' seeds was checked on the fp64 oracle alone before any GPU run (Q1 0.9947, Q2 0.9952,
Q3 0.9938 of the pixels).

Labels-only calls (scores / segment(head="fused") / validate) against the forward of the same model: the per-pixel bound of
tests/test_gpu_ragged_split_eval.py (the fp16 HEAD instance runs the 16x16x32 main loop, the forward's plain launch the 32x32x16 one):
2.1 x 66 u |V| plus the accumulation-order term sum_c |L_c| |sc_c| 2 (27 Cin) u (|x| * |w|)_c.

Q4: on an input whose bottom level is narrower than the floor the new value launches what "fp16x2+ragged" launches, the same bits."""
import pytest
import torch
import torch.nn.functional as F

from oracle import onet_oracle as orc
import test_gpu_fused_eval as fe
import test_gpu_fused_head as fh
import test_gpu_ragged_split_eval as rse
from test_gpu_fused_eval import dev  # noqa: F401  (the module-scoped fixture)

pytestmark = pytest.mark.gpu

VALUE = "fp16x2+ragged+pairs"
RAGGED = "fp16x2+ragged"
UNAMES = rse.UNAMES
PAIRS_KIND = "conv3x3_split_pre_act_pairs_kernel"
FP32_CONV_KINDS = ("conv_fwd_kernel", "conv_wino4_kernel", "conv3x3_split_kernel")
LOOSE = 1.4e4
_RUNS = {}


def _run(dev, B, C, H, W, share, bias, seed):
    """tests/test_gpu_ragged_split_eval.py's _run under the new value: model, oracle, plan and one traced forward of a recipe under
    conv = "split" -- built once"""
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
        out, kinds, names, rows, tensors = rse._traced_run(m, Xg)
        _RUNS[key] = dict(B=B, X=X, Xg=Xg, ref=ref, m=m, plan=plan, out=out, kinds=kinds, names=names, rows=rows, tensors=tensors,
                          passes=1 if share else 2)
    return _RUNS[key]


def _check_run(r, route_up1, what):
    """the plan dictionary at depth 5, the executor against it (trace order, launch records), the outputs against the oracle, every traced
    tensor against its bound, and level 4's bounds against the exact maxima its pair launches recorded"""
    from onet_amd import inference, ops
    plan, kinds, passes, B = r["plan"], r["kinds"], r["passes"], r["B"]
    assert plan["fused"] and plan["depth"] == 5 and plan["fallback_reason"] is None and plan["operands"] == "fp16x2", plan
    assert plan["twin"] == (passes == 1) and plan["batch"] == (2 * B if plan["twin"] else B), plan
    assert plan["convt"] == dict(zip(UNAMES, ("slots",) * 4)), plan
    for n, v in plan["layers"].items():
        blk = n.split(".")[0]
        want = "stem" if n == "inc.c1" else "plain+head" if n == "up4.c2" else \
            "fused+pool" if (n.endswith(".c2") and blk in ("inc", "down1", "down2", "down3")) else "fused"
        assert v == want, (n, v, want)
    n_of = {k: sum(1 for v in plan["layers"].values() if v == k) for k in ("fused", "fused+pool", "plain+head")}
    assert n_of == {"fused": 12, "fused+pool": 4, "plain+head": 1}, n_of
    with ops.using(r["m"].settings):
        levels = inference._query(r["m"].topu, (plan["batch"],) + tuple(r["Xg"].shape[1:])).levels
    assert levels[4].mode == "pairs" and levels[3].route == route_up1 and levels[3].pooled_slots, [(lv.mode, lv.route) for lv in levels]
    assert not any(u.keep_fp32 for lv in levels for u in lv.enc + lv.dec)
    assert r["names"] == fe._slot_writers(plan) * passes, (what, r["names"], fe._slot_writers(plan))
    assert {"down4.c1", "down4.c2", "up1.up", "up1.c1"} <= set(r["names"])
    assert kinds.get(PAIRS_KIND, 0) == passes * 2, (what, kinds, plan)
    assert kinds.get("conv3x3_split_pre_act_kernel", 0) == passes * (n_of["fused"] - 2), (what, kinds, plan)
    assert kinds.get("conv3x3_split_pre_act_pool_kernel", 0) == passes * n_of["fused+pool"], (what, kinds, plan)
    assert kinds.get("conv3x3_split_pre_kernel", 0) == passes * n_of["plain+head"], (what, kinds, plan)
    assert kinds.get("convt_slot_fwd_kernel", 0) == passes * 4, (what, kinds, plan)
    # no fp32 convolution but the stem's one launch per pass: those of the fall-back level are gone with it
    assert sum(kinds.get(k, 0) for k in FP32_CONV_KINDS) == passes, (what, kinds)
    print(f"{what} worst error {fe._compare(r['m'], r['out'], r['ref'], fe.TOL, what):.2e}")
    fe._check_bounds(r["rows"], what)


def _level4_records(r, what):
    """-> [(name, bound, exact maximum the pair launch recorded)] of down4.c1 and down4.c2, one per pass"""
    out = []
    for name in ("down4.c1", "down4.c2"):
        assert len(r["tensors"][name]) == r["passes"]
        for P, k, scale, amax in r["tensors"][name]:
            bound, exact = fe._slot_max(scale), fe._slot_max(amax)
            in_slots = float(P.float().sum(3).abs().max()) * 2.0 ** -k
            print(f"{what} {name}: bound {bound:.4g}, recorded exact maximum {exact:.4g} ({bound / exact:.0f}x), largest slot value {in_slots:.4g}")
            out.append((name, bound, exact))
    return out


def _check_labels_only(r, what):
    """scores, segment(head="fused") and validate against the forward: tests/test_gpu_ragged_split_eval.py's test_m1_labels_only_calls
    for a recipe of one or two passes"""
    import onet_amd
    m, Xg, out, passes, B = r["m"], r["Xg"], r["out"], r["passes"], r["B"]
    H, W = Xg.shape[2:]
    (Vt, Vd, S), k_sc, _ = fh._mfma_kinds(lambda: onet_amd.scores(m, Xg))
    lab, k_lab, _ = fh._mfma_kinds(lambda: onet_amd.segment(m, Xg, head="fused"))
    for kk in (k_sc, k_lab):
        assert kk.get("conv3x3_split_pre_head_kernel", 0) == passes and "conv3x3_split_pre_kernel" not in kk, kk
        assert kk.get(PAIRS_KIND, 0) == 2 * passes and sum(kk.get(k, 0) for k in FP32_CONV_KINDS) == passes, kk
    p1 = onet_amd.fused_eval_plan(m, Xg.shape, head="fused")
    assert p1["layers"]["up4.c2"] == "fused+head" and p1["depth"] == 5, p1
    # the last unit's operand of the traced forward and its coefficients, for the order term: a twin pass holds X, then its complement;
    # an unshared model runs topu over X, then dwnu over the complement
    ops_in = r["tensors"]["up4.c1"]
    assert len(ops_in) == passes
    halves = [(ops_in[0], slice(0, B), m.topu), (ops_in[0], slice(B, 2 * B), m.topu)] if passes == 1 else \
        [(ops_in[0], slice(0, B), m.topu), (ops_in[1], slice(0, B), m.dwnu)]
    for ((P, k, _, _), half, unet), got, ref, L, n in zip(halves, (Vt, Vd), (out[1], out[3]), (out[0], out[2]), ("Vt", "Vd")):
        x = (fh.unsplit(P) * 2.0 ** -k)[half]
        u2 = unet.up4.conv.double_conv
        conv, bn = u2[3], u2[4]
        aw = F.conv2d(x.abs(), conv.weight.detach().cpu().double().abs() * (1 + 2.0 ** -21), None, 1, 1)
        sc = (bn.weight.detach().cpu().double() / torch.sqrt(bn.running_var.detach().cpu().double() + bn.eps)).abs().view(1, -1, 1, 1)
        order = sc * (2 * 27 * conv.in_channels * fh.U) * aw
        assert tuple(got.shape) == tuple(ref.shape) and torch.isfinite(got).all() and bool((ref >= 0).all()) and bool((L >= 0).all()), n
        bound = 2.1 * fh.DOT * ref.cpu().double().abs() + (L.cpu().double().abs() * order).sum(1, keepdim=True) + 1e-30
        worst = float(((got.cpu().double() - ref.cpu().double()).abs() / bound).max())
        print(f"{what} {n}: worst |V_scores - V_out| / bound = {worst:.3e}")
        assert worst <= 1.0, f"{n}: {worst:.3f} x the bound"
    assert lab.dtype == torch.int64 and tuple(lab.shape) == (B, H, W) and torch.equal(lab, m.predict_label(S))
    sure = fe._margin(r["ref"], max(fe.MARGIN, 2 * fe.TOL))
    assert float(sure.double().mean()) > 0.9
    assert torch.equal(lab.cpu()[sure], orc.predict_label(r["ref"][4]).long()[sure])
    gt = (orc.det_input(B, 1, H, W, seed=77)[:, 0] > 0.5).to(torch.uint8)
    v = onet_amd.validate(m, Xg, gt.to(Xg.device), want_labels=True)
    torch.cuda.synchronize()
    assert torch.equal(v.labels, lab) and torch.equal(v.Vt, Vt) and torch.equal(v.Vd, Vd)
    p, g = lab.cpu() != 0, gt != 0
    want = torch.stack([(p & g).sum((1, 2)), (p & ~g).sum((1, 2)), (~p & g).sum((1, 2)), (~p & ~g).sum((1, 2))], dim=1)
    assert torch.equal(v.counts.cpu(), want.to(torch.int64)), (v.counts.cpu(), want)
    assert 0 < int(want[:, 0].sum()) and 0 < int(want[:, 3].sum())


def test_q1_odd_height_narrow_pairs_and_the_ragged_slot_convt(dev):
    """Q1: Onet(1, shared) at 3 x 1 x 80 x 224 (twin batch of 6: three pairs): levels 80 x 224 (full tiles), 40 x 112, 20 x 56, 10 x 28
    (ragged) and 5 x 14 -- pair tiles of odd H and W < 16, whose 70 pixels per image go up on the two-part ragged slot GEMM
    ("slots_ragged").
    Measured on an MI355X: Lt 9.5e-7, Vt 5.1e-6, Ld 8.0e-7, Vd 4.2e-6, S 4.5e-5 (bound 2e-4); worst |V_scores - V_out| / bound
    Vt 1.3e-4, Vd 1.1e-4; worst bound / exact maximum of a traced tensor 13370x (up1.c1: two chained bounds)."""
    r = _run(dev, 3, 1, 80, 224, True, 0.0, 401)
    assert r["plan"]["twin"] and r["plan"]["batch"] == 6, r["plan"]
    _check_run(r, "slots_ragged", "Q1 split pairs 80x224")
    _check_labels_only(r, "Q1 split pairs 80x224")


def test_q2_unshared_rgb_one_image_per_pair_tile(dev):
    """Q2: Onet(3, unshared), bias 0.1, at 1 x 3 x 64 x 256: two passes of ONE image each -- every pair tile of level 4 (4 x 16) holds
    one image, its second half staged out of range and kept out of the record -- levels 64 x 256, 32 x 128, 16 x 64 (full tiles),
    8 x 32 (ragged) and 4 x 16, whose 64 pixels per image go up on the ragged slot GEMM.
    Measured on an MI355X: Lt 7.6e-7, Vt 4.0e-6, Ld 7.3e-7, Vd 5.1e-6, S 6.6e-5 (bound 2e-4); worst |V_scores - V_out| / bound
    Vt 1.2e-4, Vd 1.2e-4; worst bound / exact maximum of a traced tensor 12672x (up1.c1)."""
    r = _run(dev, 1, 3, 64, 256, False, 0.1, 402)
    assert not r["plan"]["twin"] and r["plan"]["batch"] == 1, r["plan"]
    _check_run(r, "slots_ragged", "Q2 split pairs 64x256")
    _check_labels_only(r, "Q2 split pairs 64x256")


def test_q3_four_full_tile_levels_and_the_slot_convt(dev):
    """Q3: Onet(1, shared) at 1 x 1 x 128 x 256 (twin batch of 2): levels 128 x 256, 64 x 128, 32 x 64 and 16 x 32 are made of full
    tiles, level 4 is 8 x 16 -- a full pair of half-height -- and its h w = 128 pixels per image go up on the slot GEMM itself.
    Measured on an MI355X: Lt 9.7e-7, Vt 4.0e-6, Ld 8.2e-7, Vd 5.1e-6, S 4.8e-5 (bound 2e-4); worst |V_scores - V_out| / bound
    Vt 1.3e-4, Vd 1.1e-4; worst bound / exact maximum of a traced tensor 12911x (up1.c1)."""
    r = _run(dev, 1, 1, 128, 256, True, 0.0, 303)
    assert r["plan"]["twin"] and r["plan"]["batch"] == 2, r["plan"]
    _check_run(r, "slots", "Q3 split pairs 128x256")
    _check_labels_only(r, "Q3 split pairs 128x256")


RECIPES = {"q1": (3, 1, 80, 224, True, 0.0, 401), "q2": (1, 3, 64, 256, False, 0.1, 402), "q3": (1, 1, 128, 256, True, 0.0, 303)}


@pytest.mark.parametrize("recipe", sorted(RECIPES))
def test_level4_bounds_hold_the_recorded_maxima_with_the_full_tile_plans_looseness(dev, recipe):
    """The traced bound of down4.c1 and down4.c2 is no smaller than the exact maximum the pair launch recorded, and no looser than
    1.4e4 x -- the figure of the full-tile plan's chained bounds (13808 x at 512 x 512, 12988 x at 224 x 224, both on up1.c1).
    Measured on an MI355X (bound / recorded maximum): q1 down4.c1 126 x, down4.c2 193 x; q2 (two passes) 137 x / 154 x, 215 x / 225 x;
    q3 127 x, 169 x -- one bound each: down4.c1 starts from the exact record of down3.c2 (inference._pooled_unit(record=True)).
    With down3.c2 handing on its BOUND, as every other pooled unit does, down4.c1 chained two bounds over its 4608-term sums and
    measured 16005 x (q1), 17042 x / 16020 x (q2) and 14503 x (q3): this assertion failed, which is why that unit records."""
    r = _run(dev, *RECIPES[recipe])
    recs = _level4_records(r, recipe.upper() + " split pairs")
    for name, bound, exact in recs:
        assert exact > 0 and bound >= exact, (recipe, name, bound, exact)
    for name, bound, exact in recs:
        assert bound / exact <= LOOSE, (recipe, name, bound, exact, bound / exact)


def test_q4_below_the_floor_is_the_ragged_plan_bit_for_bit(dev):
    """Q4: 2 x 1 x 64 x 64 -- level 2 is 16 x 16, a level k < 4 the new value does not add, and level 4 (4 x 4) lies below its floor --
    under the new value: the five outputs, scores and segment(head="fused") bit-identical to "fp16x2+ragged", the same plan and the
    same launch records (MFMA kinds and every other entry point)"""
    import onet_amd
    from onet_amd import ops
    m = fe._onet(fe._prefixed(orc.det_state_dict(1, 1981)), 1, True, dev)
    Xg = orc.det_input(2, 1, 64, 64, seed=304).to(dev)
    got = {}
    m.settings = ops.Settings(conv="split", fused_eval=RAGGED)
    with torch.no_grad():
        m(Xg)                   # (the weight packs are made on first use: not part of either record)
    for value in (RAGGED, VALUE):
        m.settings = ops.Settings(conv="split", fused_eval=value)
        got[value] = (fh._mfma_kinds(lambda: m(Xg)), fh._mfma_kinds(lambda: onet_amd.scores(m, Xg)),
                      fh._mfma_kinds(lambda: onet_amd.segment(m, Xg, head="fused")), onet_amd.fused_eval_plan(m, Xg.shape))
    a, b = got[RAGGED], got[VALUE]
    assert a[3] == b[3] and b[3]["fused"] and b[3]["depth"] == 2, (a[3], b[3])
    for (oa, ka, ra), (ob, kb, rb), what in zip(a[:3], b[:3], ("forward", "scores", "segment")):
        oa, ob = (oa, ob) if isinstance(oa, tuple) else ((oa,), (ob,))
        assert len(oa) == len(ob) and all(torch.equal(x, y) for x, y in zip(oa, ob)), what
        assert ka == kb and ra == rb and ka and PAIRS_KIND not in kb, (what, ka, kb, ra, rb)
