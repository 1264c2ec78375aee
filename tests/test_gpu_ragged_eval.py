"""The one-part fused eval plan on ragged maps, Settings(fused_eval="bf16+pool+ragged") (onet_amd/inference.py).

M1 / M3 hold the plan on levels that are not made of full 16 x 32 tiles to the fp64 oracle with the run's own roundings replayed --
the method, the helpers and the bounds of tests/test_gpu_fused_eval_bf16.py (TOL = 2e-4 of each output's largest magnitude, labels
equal on the margin pixels, those more than 0.9 of all), nothing new -- and scores / segment(head="fused") / validate to the forward
with the bounds of tests/test_gpu_fused_head.py (2.1 x 66 u |V|).  M2: on maps made of full tiles the new value launches what
"bf16+pool" launches and gives the same bits.  M4: the depth at 200 x 200 and the fall-back at W % 4 != 0."""
import pytest
import torch

from oracle import onet_oracle as orc
import test_gpu_fused_eval_bf16 as e16
import test_gpu_fused_head as fh
from test_gpu_fused_eval_bf16 import dev  # noqa: F401  (the module-scoped fixture)

pytestmark = pytest.mark.gpu

VALUE = "bf16+pool+ragged"
UNAMES = e16.UNAMES


def _traced_run(m, Xg):
    """e16._traced_run -- one forward with inference.TRACE on and the ConvTranspose2d wrappers watched -> (outputs, {kind: launches},
    {name: [slot tensor per pass]}, [per ConvTranspose2d call, in order: its bf16-rounded input as fp64 on the host, or None where the
    layer ran at fp32 level]) -- with the ragged slot-operand entry watched beside the three that function knows.  The general kernel
    on a map with h w % 128 != 0 (the plan's "fp32->slots" hand-off below a ragged level) is the direct fp32 kernel: unrounded."""
    from onet_amd import inference, ops
    convt = []
    names = ("convT2x2_fwd", "convT2x2_fwd_p", "convT2x2_fwd_slots", "convT2x2_fwd_slots_ragged")
    real = {n: getattr(ops, n) for n in names}

    def fp32_input(x, Ct):
        B, _, h, w = x.shape
        return x.detach().to(torch.bfloat16).cpu().double() if ops.convt_operand_bf16(B, h, w, Ct) == 1 else None

    def fwd(x, wq, bias, out, Ct, pt, pl):
        B, Cin, h, w = x.shape
        gemm = (pt, pl) == (0, 0) and tuple(out.shape[2:]) == (2 * h, 2 * w) and Cin % 16 == 0 and Ct % 32 == 0 and (h * w) % 128 == 0 and w % 2 == 0
        convt.append(fp32_input(x, Ct) if gemm else None)
        return real["convT2x2_fwd"](x, wq, bias, out, Ct, pt, pl)

    def fwd_p(x, wq, bias, outP, Ct, pt, pl, slots=None):
        done = real["convT2x2_fwd_p"](x, wq, bias, outP, Ct, pt, pl, slots=slots)
        if done:
            convt.append(fp32_input(x, Ct))
        return done

    def on_slots(name):
        def call(xP, wP, bias, outP, Ct, **kw):
            done = real[name](xP, wP, bias, outP, Ct, **kw)
            if done:
                convt.append(e16.unslot(xP))
            return done
        return call

    inference.TRACE = []
    for n, f in zip(names, (fwd, fwd_p, on_slots(names[2]), on_slots(names[3]))):
        setattr(ops, n, f)
    ops.profile_start(everything=False)
    try:
        with torch.no_grad():
            out = m(Xg)
        torch.cuda.synchronize()
        trace = {}
        for name, t in inference.TRACE:
            assert t.P is not None and t.P.shape[3] == 1 and t.scale is None and t.amax is None, name
            trace.setdefault(name, []).append(e16.unslot(t.P))
    finally:
        kinds = {k: len(v) for k, v in ops.profile_stop()[0].items()}
        inference.TRACE = None
        for n, f in real.items():
            setattr(ops, n, f)
    return out, kinds, trace, convt


def _run(dev, B, C, H, W, share, bias, seed):
    """model, plan, traced run and replay lists of one recipe under conv = "bf16" and the new value"""
    import onet_amd
    from onet_amd import ops
    X = orc.det_input(B, C, H, W, seed=seed)
    top = e16._calibrated(orc.det_state_dict(C, 1981), X, bias)
    dwn = None if share else e16._calibrated(orc.det_state_dict(C, 1982), X, bias)
    m = e16._onet(e16._prefixed(top, dwn), C, share, dev)
    m.bias = bias
    m.settings = ops.Settings(conv="bf16", fused_eval=VALUE)
    Xg = X.to(dev)
    plan = onet_amd.fused_eval_plan(m, Xg.shape)
    out, kinds, trace, convt = _traced_run(m, Xg)
    replay, on_slots = e16._replay_lists(trace, convt, B, plan.get("twin", False))
    return dict(B=B, X=X, Xg=Xg, top=top, dwn=dwn, bias=bias, m=m, plan=plan, out=out, kinds=kinds, replay=replay, on_slots=on_slots)


def _assert_plan(plan, d, kinds, passes):
    """depth d of a 5-level U-Net under the new value: the kinds announced and the launch records"""
    fused_levels = e16.NAMES[:d]
    for n, v in plan["layers"].items():
        blk = n.split(".")[0]
        level = e16.NAMES.index(blk) if blk in e16.NAMES else UNAMES.index(blk)
        want = "fallback" if level >= d else "stem" if n == "inc.c1" else "plain+head" if n == "up4.c2" else \
            "fused+pool" if (n.endswith(".c2") and blk in fused_levels[:4]) else "fused"
        assert v == want, (n, v, want)
    n_of = {k: sum(1 for v in plan["layers"].values() if v == k) for k in ("fused", "fused+pool", "plain+head")}
    assert kinds.get("conv3x3_pre16_act_kernel", 0) == passes * n_of["fused"] > 0, (kinds, plan)
    assert kinds.get("conv3x3_pre16_act_pool_kernel", 0) == passes * n_of["fused+pool"] > 0, (kinds, plan)
    assert kinds.get("conv3x3_split_pre_kernel", 0) == passes * n_of["plain+head"], (kinds, plan)
    assert kinds.get("convt_slot_fwd_kernel", 0) == passes * sum(1 for v in plan["convt"].values() if v == "slots"), (kinds, plan)


def test_m1_ragged_levels_replayed_and_labels_only_calls(dev):
    """M1: Onet(1, shared) at 2 x 1 x 48 x 80 (twin batch of 4): levels 48 x 80, 24 x 40 and 12 x 20 -- none made of full tiles -- are
    fused, the 6 x 10 level (W % 4) is the fall-back; the ConvTranspose2d of levels 0 and 1 on the ragged slot-operand entry, level 2's
    by the general kernel and one conversion pass.  The five outputs against the fp64 oracle with the run's roundings replayed
    (e16._check_replayed_run: its bounds); scores / segment(head="fused") against the forward (test_gpu_fused_head.py's bounds);
    validate's counts == counting its labels on the host.
    Measured on an MI355X: Lt 3.2e-7, Vt 2.0e-7, Ld 3.0e-7, Vd 1.8e-7, S 1.5e-6 (bound 2e-4); margin pixels 0.9932; worst
    |V_scores - V_out| / bound Vt 0.033, Vd 0.038; label margin pixels 1.0000."""
    import onet_amd
    r = _run(dev, 2, 1, 48, 80, True, 0.0, 201)
    plan, m, Xg = r["plan"], r["m"], r["Xg"]
    assert plan["fused"] and plan["depth"] == 3 and plan["operands"] == "bf16" and plan["twin"] and plan["batch"] == 4, plan
    assert plan["convt"] == {UNAMES[0]: "slots", UNAMES[1]: "slots", UNAMES[2]: "fp32->slots", UNAMES[3]: "fallback"}, plan
    assert plan["fallback_reason"].startswith("level 3: down3.c1"), plan
    _assert_plan(plan, 3, r["kinds"], 1)
    assert r["on_slots"] == {n for n, v in plan["layers"].items() if v in ("fused", "fused+pool", "plain+head")}, r["on_slots"]
    e16._check_replayed_run(r, "M1 ragged")
    out = r["out"]
    # the labels-only calls against the forward: fh._check_against_forward's value and label assertions on this shape
    (Vt, Vd, S), k_sc, _ = fh._mfma_kinds(lambda: onet_amd.scores(m, Xg))
    lab, k_lab, _ = fh._mfma_kinds(lambda: onet_amd.segment(m, Xg, head="fused"))
    for kk in (k_sc, k_lab):
        assert kk.get("conv3x3_pre16_head_kernel", 0) == 1 and "conv3x3_split_pre_kernel" not in kk, kk
    for got, ref, n in ((Vt, out[1], "Vt"), (Vd, out[3], "Vd")):
        assert tuple(got.shape) == tuple(ref.shape) and torch.isfinite(got).all() and bool((ref >= 0).all()), n
        bound = 2.1 * fh.DOT * ref.double().abs() + 1e-30
        ratio = float(((got.double() - ref.double()).abs() / bound).max())
        print(f"M1 ragged {n}: worst |V_scores - V_out| / (2.1 x 66 u |V_out|) = {ratio:.3f}")
        assert ratio <= 1.0, f"{n}: {ratio:.3f} x the bound"
    assert lab.dtype == torch.int64 and tuple(lab.shape) == (2, 48, 80) and torch.equal(lab, m.predict_label(S))
    ref_lab = onet_amd.segment(m, Xg)
    sure = ((out[1] - out[3]).abs() > 4 * fh.DOT * torch.maximum(out[1], out[3]))[:, 0]
    share = float(sure.double().mean())
    print(f"M1 ragged: label margin pixels {share:.4f}")
    assert share > 0.9 and torch.equal(lab[sure], ref_lab[sure])
    p1 = onet_amd.fused_eval_plan(m, Xg.shape, head="fused")
    assert p1["layers"]["up4.c2"] == "fused+head" and p1["depth"] == 3, p1
    # validate: the counts are those of its own labels, counted on the host
    gt = (orc.det_input(2, 1, 48, 80, seed=77)[:, 0] > 0.5).to(torch.uint8)
    v = onet_amd.validate(m, Xg, gt.to(dev), want_labels=True)
    torch.cuda.synchronize()
    assert torch.equal(v.labels, lab) and torch.equal(v.Vt, Vt) and torch.equal(v.Vd, Vd)
    p, g = v.labels.cpu() != 0, gt != 0
    want = torch.stack([(p & g).sum((1, 2)), (p & ~g).sum((1, 2)), (~p & g).sum((1, 2)), (~p & ~g).sum((1, 2))], dim=1)
    assert torch.equal(v.counts.cpu(), want.to(torch.int64)), (v.counts.cpu(), want)
    assert 0 < int(want[:, 0].sum()) and 0 < int(want[:, 3].sum())


def test_m2_full_tiles_are_the_pooled_plan_bit_for_bit(dev):
    """M2: 2 x 1 x 128^2 -- every level the plan takes is made of full tiles -- under the new value: the five outputs, scores and
    segment(head="fused") bit-identical to "bf16+pool", and the same launch records (MFMA kinds and every other entry point)"""
    import onet_amd
    from onet_amd import ops
    r = fh._recipe(dev, "A")
    m, Xg = r["m"], r["Xg"]
    got = {}
    m.settings = ops.Settings(conv="bf16", fused_eval="bf16+pool")
    with torch.no_grad():
        m(Xg)                   # (the weight packs are made on first use: not part of either record)
    for value in ("bf16+pool", VALUE):
        m.settings = ops.Settings(conv="bf16", fused_eval=value)
        got[value] = (fh._mfma_kinds(lambda: m(Xg)), fh._mfma_kinds(lambda: onet_amd.scores(m, Xg)),
                      fh._mfma_kinds(lambda: onet_amd.segment(m, Xg, head="fused")), onet_amd.fused_eval_plan(m, Xg.shape))
    a, b = got["bf16+pool"], got[VALUE]
    assert a[3] == b[3] and b[3]["fused"] and b[3]["depth"] == 3, (a[3], b[3])
    for (oa, ka, ra), (ob, kb, rb), what in zip(a[:3], b[:3], ("forward", "scores", "segment")):
        oa, ob = (oa, ob) if isinstance(oa, tuple) else ((oa,), (ob,))
        assert len(oa) == len(ob) and all(torch.equal(x, y) for x, y in zip(oa, ob)), what
        assert ka == kb and ra == rb and ka, (what, ka, kb, ra, rb)


def test_m3_unshared_rgb_224_replayed(dev):
    """M3: Onet(3, unshared), bias 0.1, at 1 x 3 x 224 x 224 -- the ZY-3 thumbnails' shape: level 0 is made of full tiles, 112 / 56 / 28
    are ragged, the 14-pixel level is the fall-back, whose output enters the 28-pixel concat buffer as "fp32->slots".  One run, the
    replay check of M1.
    Measured on an MI355X: Lt 3.6e-7, Vt 2.1e-7, Ld 3.5e-7, Vd 3.5e-7, S 1.5e-6 (bound 2e-4); margin pixels 0.9946.  (The fp64 oracle
    of two U-Nets at 224 x 224 on the host is this test's 7 s.)"""
    r = _run(dev, 1, 3, 224, 224, False, 0.1, 202)
    plan = r["plan"]
    assert plan["fused"] and plan["depth"] == 4 and plan["operands"] == "bf16" and not plan["twin"] and plan["batch"] == 1, plan
    assert plan["convt"] == {UNAMES[0]: "slots", UNAMES[1]: "slots", UNAMES[2]: "slots", UNAMES[3]: "fp32->slots"}, plan
    _assert_plan(plan, 4, r["kinds"], 2)
    e16._check_replayed_run(r, "M3 ragged 224")


def test_m4_depth_at_200_and_fall_back_at_w250(dev):
    """M4: 1 x 1 x 200 x 200 -- levels 200 and 100, the 50-pixel level is W % 4 -- reports depth 2 and runs (finite, repeatable, the
    announced launches); 2 x 1 x 256 x 250 reports depth 0 with a reason naming W and is the ordinary forward bit for bit"""
    import onet_amd
    from onet_amd import ops
    m = e16._onet(e16._prefixed(orc.det_state_dict(1, 1981)), 1, True, dev)
    st = ops.Settings(conv="bf16", fused_eval=VALUE)
    X = orc.det_input(1, 1, 200, 200, seed=113).to(dev)
    out, kinds = e16._eval(m, X, st)
    plan = onet_amd.fused_eval_plan(m, X.shape)
    assert plan["fused"] and plan["depth"] == 2 and "W = 50" in plan["fallback_reason"], plan
    assert plan["convt"] == {UNAMES[0]: "slots", UNAMES[1]: "fp32->slots", UNAMES[2]: "fallback", UNAMES[3]: "fallback"}, plan
    _assert_plan(plan, 2, kinds, 1)
    assert all(torch.isfinite(t).all() for t in out) and tuple(out[4].shape) == (1, 2, 200, 200)
    out2, _ = e16._eval(m, X)
    assert all(torch.equal(x, y) for x, y in zip(out, out2))
    X = orc.det_input(2, 1, 256, 250, seed=114).to(dev)
    got, kg = e16._eval(m, X, st)
    plan = onet_amd.fused_eval_plan(m, X.shape)
    assert not plan["fused"] and plan["depth"] == 0 and "W = 250" in plan["reason"], plan
    ref, kr = e16._eval(m, X, ops.Settings(conv="bf16"))
    assert kg == kr and all(torch.equal(x, y) for x, y in zip(got, ref)), (kg, kr)
