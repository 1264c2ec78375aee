"""The one-part fused eval plan at full depth, Settings(fused_eval="bf16+pool+anymap+pairs") (onet_amd/inference.py): level 4 -- down4.c1,
down4.c2 and the ConvTranspose2d of up1 -- on image-pair tiles (ops.conv3x3_plain16_pre_act_pairs).

P1 - P3 hold plans whose bottom level is 3 x 12, 2 x 16 and 8 x 16 to the fp64 oracle with the run's own roundings replayed -- the method,
the helpers and the bounds of tests/test_gpu_anymap_eval.py (TOL = 2e-4 of each output's largest magnitude, labels equal on the margin
pixels, those more than 0.9 of all; scores / segment(head="fused") / validate against the forward with 2.1 x 66 u |V|), nothing new.
The replay helpers cope with a plan without a fall-back level as they stand: the trace then holds down3.pool and down4.c1, the inputs
of the two convolutions of level 4, and all four ConvTranspose2d calls are the plan's.  What is this file's own is the launch record
(_assert_plan: two launches of the pair kind per pass, the stem the only convolution left outside the one-part kernels).
P4: on an input whose bottom level is narrower than the floor the new value launches what "bf16+pool+anymap" launches, the same bits.
The margin-pixel condition of the three recipes' seeds was checked on the fp64 oracle alone before any GPU run (P1 0.9934, P2 0.9954,
P3 0.9938 of the pixels of the unrounded oracle)."""
import pytest
import torch

from oracle import onet_oracle as orc
import test_gpu_fused_eval_bf16 as e16
import test_gpu_fused_head as fh
import test_gpu_ragged_eval as rge
from test_gpu_fused_eval_bf16 import dev  # noqa: F401  (the module-scoped fixture)

pytestmark = pytest.mark.gpu

VALUE = "bf16+pool+anymap+pairs"
ANYMAP = "bf16+pool+anymap"
UNAMES = e16.UNAMES
PAIRS_KIND = "conv3x3_pre16_act_pairs_kernel"
FP32_CONV_KINDS = ("conv_fwd_kernel", "conv_wino4_kernel", "conv3x3_split_kernel")


def _run(dev, B, C, H, W, share, bias, seed):
    """tests/test_gpu_anymap_eval.py's _run under the new value: model, plan, traced run and replay lists of one recipe under conv = "bf16" """
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
    out, kinds, trace, convt = rge._traced_run(m, Xg)
    replay, on_slots = e16._replay_lists(trace, convt, B, plan.get("twin", False))
    return dict(B=B, X=X, Xg=Xg, top=top, dwn=dwn, bias=bias, m=m, plan=plan, out=out, kinds=kinds, replay=replay, on_slots=on_slots)


def _assert_plan(plan, kinds, passes):
    """full depth of a 5-level U-Net under the new value: the kinds announced and the launch records -- rge._assert_plan with the two
    units of level 4 on the pair kind and no fall-back level"""
    assert plan["depth"] == 5 and plan["fallback_reason"] is None, plan
    for n, v in plan["layers"].items():
        blk = n.split(".")[0]
        want = "stem" if n == "inc.c1" else "plain+head" if n == "up4.c2" else \
            "fused+pool" if (n.endswith(".c2") and blk in e16.NAMES[:4]) else "fused"
        assert v == want, (n, v, want)
    assert plan["layers"]["down4.c1"] == plan["layers"]["down4.c2"] == "fused"
    n_of = {k: sum(1 for v in plan["layers"].values() if v == k) for k in ("fused", "fused+pool", "plain+head")}
    assert n_of == {"fused": 12, "fused+pool": 4, "plain+head": 1}, n_of
    assert kinds.get(PAIRS_KIND, 0) == passes * 2, (kinds, plan)
    assert kinds.get("conv3x3_pre16_act_kernel", 0) == passes * (n_of["fused"] - 2), (kinds, plan)
    assert kinds.get("conv3x3_pre16_act_pool_kernel", 0) == passes * n_of["fused+pool"], (kinds, plan)
    assert kinds.get("conv3x3_split_pre_kernel", 0) == passes * n_of["plain+head"], (kinds, plan)
    assert kinds.get("convt_slot_fwd_kernel", 0) == passes * sum(1 for v in plan["convt"].values() if v == "slots"), (kinds, plan)
    # no fp32 convolution but the stem's one launch per pass (whichever fp32 kernel the dispatch gives it): those of the fall-back level
    # -- F(4x4) Winograd at 16 pixels, the direct kernel below -- are gone with it
    assert sum(kinds.get(k, 0) for k in FP32_CONV_KINDS) == passes, kinds


def _check(r, convt, what):
    """tests/test_gpu_anymap_eval.py's _check at full depth: the plan's announcement and launch records, the replayed oracle (e16._check_replayed_run: its bounds),
    the labels-only calls against the forward (tests/test_gpu_fused_head.py's bounds) and validate's counts against its own labels
    counted on the host"""
    import onet_amd
    plan, m, Xg, out, B = r["plan"], r["m"], r["Xg"], r["out"], r["B"]
    passes = 1 if plan["twin"] else 2
    H, W = Xg.shape[2:]
    assert plan["fused"] and plan["depth"] == 5 and plan["operands"] == "bf16" and plan["batch"] == (2 * B if plan["twin"] else B), plan
    assert plan["convt"] == dict(zip(UNAMES, convt)), plan
    _assert_plan(plan, r["kinds"], passes)
    assert r["on_slots"] == {n for n, v in plan["layers"].items() if v in ("fused", "fused+pool", "plain+head")}, r["on_slots"]
    assert {"down4.c1", "down4.c2", "up1.c1"} <= r["on_slots"]
    e16._check_replayed_run(r, what)
    (Vt, Vd, S), k_sc, _ = fh._mfma_kinds(lambda: onet_amd.scores(m, Xg))
    lab, k_lab, _ = fh._mfma_kinds(lambda: onet_amd.segment(m, Xg, head="fused"))
    for kk in (k_sc, k_lab):
        assert kk.get("conv3x3_pre16_head_kernel", 0) == passes and "conv3x3_split_pre_kernel" not in kk, kk
        assert kk.get(PAIRS_KIND, 0) == 2 * passes and sum(kk.get(k, 0) for k in FP32_CONV_KINDS) == passes, kk
    for got, ref, n in ((Vt, out[1], "Vt"), (Vd, out[3], "Vd")):
        assert tuple(got.shape) == tuple(ref.shape) and torch.isfinite(got).all() and bool((ref >= 0).all()), n
        bound = 2.1 * fh.DOT * ref.double().abs() + 1e-30
        ratio = float(((got.double() - ref.double()).abs() / bound).max())
        print(f"{what} {n}: worst |V_scores - V_out| / (2.1 x 66 u |V_out|) = {ratio:.3f}")
        assert ratio <= 1.0, f"{n}: {ratio:.3f} x the bound"
    assert lab.dtype == torch.int64 and tuple(lab.shape) == (B, H, W) and torch.equal(lab, m.predict_label(S))
    ref_lab = onet_amd.segment(m, Xg)
    sure = ((out[1] - out[3]).abs() > 4 * fh.DOT * torch.maximum(out[1], out[3]))[:, 0]
    share = float(sure.double().mean())
    print(f"{what}: label margin pixels {share:.4f}")
    assert share > 0.9 and torch.equal(lab[sure], ref_lab[sure])
    p1 = onet_amd.fused_eval_plan(m, Xg.shape, head="fused")
    assert p1["layers"]["up4.c2"] == "fused+head" and p1["depth"] == 5, p1
    gt = (orc.det_input(B, 1, H, W, seed=77)[:, 0] > 0.5).to(torch.uint8)
    v = onet_amd.validate(m, Xg, gt.to(Xg.device), want_labels=True)
    torch.cuda.synchronize()
    assert torch.equal(v.labels, lab) and torch.equal(v.Vt, Vt) and torch.equal(v.Vd, Vd)
    p, g = v.labels.cpu() != 0, gt != 0
    want = torch.stack([(p & g).sum((1, 2)), (p & ~g).sum((1, 2)), (~p & g).sum((1, 2)), (~p & ~g).sum((1, 2))], dim=1)
    assert torch.equal(v.counts.cpu(), want.to(torch.int64)), (v.counts.cpu(), want)
    assert 0 < int(want[:, 0].sum()) and 0 < int(want[:, 3].sum())


def test_p1_pack_route_with_pad_and_keep_fp32_from_the_pair_launch(dev):
    """P1: Onet(1, shared) at 1 x 1 x 48 x 200 (twin batch of 2: one pair): levels 48 x 200, 24 x 100, 12 x 50, 6 x 25 and 3 x 12.  The
    bottom level's 6 x 24 up-sampled output is padded into the 6 x 25 concat buffer -- the `pack` route, so down4.c2's pair launch
    also writes fp32 (keep_fp32: rows of 12 floats under per-float guards) -- and level 3's odd-w map goes up by `pack` too; levels
    1 and 0 read 12 x 50 and 24 x 100 maps on the ragged slot GEMM (up_edge: w even, h w % 128 != 0).
    Measured on an MI355X: Lt 3.9e-7, Vt 1.8e-7, Ld 3.8e-7, Vd 1.9e-7, S 1.2e-6 (bound 2e-4); margin pixels 0.9946; worst
    |V_scores - V_out| / bound Vt 0.040, Vd 0.042; label margin pixels 0.9999."""
    r = _run(dev, 1, 1, 48, 200, True, 0.0, 301)
    assert r["plan"]["twin"], r["plan"]
    _check(r, ("slots", "slots", "fp32->slots", "fp32->slots"), "P1 pairs 48x200")


def test_p2_unshared_rgb_odd_image_count_and_ragged_slot_convt(dev):
    """P2: Onet(3, unshared), bias 0.1, at 1 x 3 x 32 x 256: two passes of ONE image each -- every pair tile of level 4 (2 x 16) holds
    one image, its second half staged out of range -- levels 32 x 256 (full tiles), 16 x 128, 8 x 64, 4 x 32 (ragged) and 2 x 16,
    whose 32 pixels per image go up on the ragged slot GEMM (up_edge: h w % 128 != 0, even w, no pad).
    Measured on an MI355X: Lt 3.5e-7, Vt 2.0e-7, Ld 3.8e-7, Vd 2.1e-7, S 1.4e-6 (bound 2e-4); margin pixels 0.9945; worst
    |V_scores - V_out| / bound Vt 0.035, Vd 0.038; label margin pixels 1.0000."""
    r = _run(dev, 1, 3, 32, 256, False, 0.1, 302)
    assert not r["plan"]["twin"], r["plan"]
    _check(r, ("slots", "slots", "slots", "slots"), "P2 pairs 32x256")


def test_p3_four_full_tile_levels_and_the_slot_convt(dev):
    """P3: Onet(1, shared) at 1 x 1 x 128 x 256 (twin batch of 2): levels 128 x 256, 64 x 128, 32 x 64 and 16 x 32 are made of full
    tiles, level 4 is 8 x 16 -- a full pair of half-height -- and its h w = 128 pixels per image go up on the slot GEMM itself.
    Measured on an MI355X: Lt 3.7e-7, Vt 2.1e-7, Ld 3.0e-7, Vd 1.9e-7, S 2.1e-6 (bound 2e-4); margin pixels 0.9938; worst
    |V_scores - V_out| / bound Vt 0.048, Vd 0.040; label margin pixels 1.0000."""
    r = _run(dev, 1, 1, 128, 256, True, 0.0, 303)
    assert r["plan"]["twin"], r["plan"]
    _check(r, ("slots", "slots", "slots", "slots"), "P3 pairs 128x256")


def test_p4_below_the_floor_is_the_anymap_plan_bit_for_bit(dev):
    """P4: 2 x 1 x 64 x 64 -- level 2 is 16 x 16, a level k < 4 the new value does not add, and level 4 (4 x 4) lies below its floor --
    under the new value: the five outputs, scores and segment(head="fused") bit-identical to "bf16+pool+anymap", the same plan and the same
    launch records (MFMA kinds and every other entry point)"""
    import onet_amd
    from onet_amd import ops
    m = e16._onet(e16._prefixed(orc.det_state_dict(1, 1981)), 1, True, dev)
    Xg = orc.det_input(2, 1, 64, 64, seed=304).to(dev)
    got = {}
    m.settings = ops.Settings(conv="bf16", fused_eval=ANYMAP)
    with torch.no_grad():
        m(Xg)                   # (the weight packs are made on first use: not part of either record)
    for value in (ANYMAP, VALUE):
        m.settings = ops.Settings(conv="bf16", fused_eval=value)
        got[value] = (fh._mfma_kinds(lambda: m(Xg)), fh._mfma_kinds(lambda: onet_amd.scores(m, Xg)),
                      fh._mfma_kinds(lambda: onet_amd.segment(m, Xg, head="fused")), onet_amd.fused_eval_plan(m, Xg.shape))
    a, b = got[ANYMAP], got[VALUE]
    assert a[3] == b[3] and b[3]["fused"] and b[3]["depth"] == 2, (a[3], b[3])
    for (oa, ka, ra), (ob, kb, rb), what in zip(a[:3], b[:3], ("forward", "scores", "segment")):
        oa, ob = (oa, ob) if isinstance(oa, tuple) else ((oa,), (ob,))
        assert len(oa) == len(ob) and all(torch.equal(x, y) for x, y in zip(oa, ob)), what
        assert ka == kb and ra == rb and ka and PAIRS_KIND not in kb, (what, ka, kb, ra, rb)
