"""The one-part fused eval plan on maps of any size, Settings(fused_eval="bf16+pool+anymap") (onet_amd/inference.py).

A1 - A3 hold the plan on levels outside the ragged domain (W % 4 != 0, odd H and W, a padded ConvTranspose2d output, floor pooling) to
the fp64 oracle with the run's own roundings replayed -- the method, the helpers and the bounds of tests/test_gpu_ragged_eval.py /
tests/test_gpu_fused_eval_bf16.py (TOL = 2e-4 of each output's largest magnitude, labels equal on the margin pixels, those more than
0.9 of all), nothing new -- and scores / segment(head="fused") / validate to the forward with the bounds of tests/test_gpu_fused_head.py
(2.1 x 66 u |V|).  A4: on inputs whose levels all lie in the ragged domain the new value launches what "bf16+pool+ragged" launches and
gives the same bits.  The margin-pixel condition of the three recipes' seeds was checked on the fp64 oracle alone before any GPU run
(A1 0.9953, A2 0.9945, A3 0.9933 of the pixels of the unrounded oracle)."""
import pytest
import torch

from oracle import onet_oracle as orc
import test_gpu_fused_eval_bf16 as e16
import test_gpu_fused_head as fh
import test_gpu_ragged_eval as rge
from test_gpu_fused_eval_bf16 import dev  # noqa: F401  (the module-scoped fixture)

pytestmark = pytest.mark.gpu

VALUE = "bf16+pool+anymap"
RAGGED = "bf16+pool+ragged"
UNAMES = e16.UNAMES


def _run(dev, B, C, H, W, share, bias, seed):
    """rge._run under the new value: model, plan, traced run and replay lists of one recipe under conv = "bf16" """
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


def _check(r, d, convt, what):
    """the plan's announcement and launch records, the replayed oracle (e16._check_replayed_run: its bounds), the labels-only calls
    against the forward (tests/test_gpu_fused_head.py's bounds) and validate's counts against its own labels counted on the host"""
    import onet_amd
    plan, m, Xg, out, B = r["plan"], r["m"], r["Xg"], r["out"], r["B"]
    passes = 1 if plan["twin"] else 2
    H, W = Xg.shape[2:]
    assert plan["fused"] and plan["depth"] == d and plan["operands"] == "bf16" and plan["batch"] == (2 * B if plan["twin"] else B), plan
    assert plan["convt"] == dict(zip(UNAMES, convt)), plan
    rge._assert_plan(plan, d, r["kinds"], passes)
    assert r["on_slots"] == {n for n, v in plan["layers"].items() if v in ("fused", "fused+pool", "plain+head")}, r["on_slots"]
    e16._check_replayed_run(r, what)
    (Vt, Vd, S), k_sc, _ = fh._mfma_kinds(lambda: onet_amd.scores(m, Xg))
    lab, k_lab, _ = fh._mfma_kinds(lambda: onet_amd.segment(m, Xg, head="fused"))
    for kk in (k_sc, k_lab):
        assert kk.get("conv3x3_pre16_head_kernel", 0) == passes and "conv3x3_split_pre_kernel" not in kk, kk
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
    assert p1["layers"]["up4.c2"] == "fused+head" and p1["depth"] == d, p1
    gt = (orc.det_input(B, 1, H, W, seed=77)[:, 0] > 0.5).to(torch.uint8)
    v = onet_amd.validate(m, Xg, gt.to(Xg.device), want_labels=True)
    torch.cuda.synchronize()
    assert torch.equal(v.labels, lab) and torch.equal(v.Vt, Vt) and torch.equal(v.Vd, Vd)
    p, g = v.labels.cpu() != 0, gt != 0
    want = torch.stack([(p & g).sum((1, 2)), (p & ~g).sum((1, 2)), (~p & g).sum((1, 2)), (~p & ~g).sum((1, 2))], dim=1)
    assert torch.equal(v.counts.cpu(), want.to(torch.int64)), (v.counts.cpu(), want)
    assert 0 < int(want[:, 0].sum()) and 0 < int(want[:, 3].sum())


def test_a1_w_mod_4_odd_w_pad_and_floor_pool_replayed(dev):
    """A1: Onet(1, shared) at 2 x 1 x 48 x 100 (twin batch of 4): levels 48 x 100 (ragged), 24 x 50 (W % 4 == 2) and 12 x 25 (odd W)
    are fused, the 6 x 12 level is the fall-back: its 12 x 24 up-sampled output is padded into the 12 x 25 concat buffer, down2.c2 pools
    12 x 25 to 6 x 12 (floor), and the ConvTranspose2d of level 1 reads an odd-w map -- both by the general kernel and one conversion
    pass ("fp32->slots").
    Measured on an MI355X: Lt 3.6e-7, Vt 1.9e-7, Ld 4.0e-7, Vd 2.0e-7, S 1.6e-6 (bound 2e-4); margin pixels 0.9933; worst
    |V_scores - V_out| / bound Vt 0.043, Vd 0.038; label margin pixels 1.0000."""
    r = _run(dev, 2, 1, 48, 100, True, 0.0, 201)
    assert r["plan"]["twin"] and r["plan"]["fallback_reason"].startswith("level 3: down3.c1"), r["plan"]
    _check(r, 3, ("slots", "fp32->slots", "fp32->slots", "fallback"), "A1 anymap 48x100")


def test_a2_unshared_rgb_100_odd_h_and_w_replayed(dev):
    """A2: Onet(3, unshared), bias 0.1, at 1 x 3 x 100 x 100: levels 100 (ragged), 50 and 25 (odd H and W) are fused; the 12-pixel level
    falls back and enters the 25 x 25 concat buffer padded.
    Measured on an MI355X: Lt 3.1e-7, Vt 1.6e-7, Ld 3.6e-7, Vd 1.7e-7, S 1.2e-6 (bound 2e-4); margin pixels 0.9940; worst
    |V_scores - V_out| / bound Vt 0.034, Vd 0.037; label margin pixels 1.0000."""
    r = _run(dev, 1, 3, 100, 100, False, 0.1, 202)
    assert not r["plan"]["twin"], r["plan"]
    _check(r, 3, ("slots", "fp32->slots", "fp32->slots", "fallback"), "A2 anymap 100")


def test_a3_200_is_fused_to_depth_4_replayed(dev):
    """A3: Onet(1, shared) at 1 x 1 x 200 x 200 -- the NAU-rain resolution: levels 200, 100, 50 and 25 are fused, the 12-pixel level is
    the fall-back.  (The fp64 oracle of two passes at 200 x 200 on the host is most of this test's time.)
    Measured on an MI355X: Lt 3.9e-7, Vt 2.3e-7, Ld 3.3e-7, Vd 2.2e-7, S 2.1e-6 (bound 2e-4); margin pixels 0.9933; worst
    |V_scores - V_out| / bound Vt 0.046, Vd 0.037; label margin pixels 1.0000."""
    r = _run(dev, 1, 1, 200, 200, True, 0.0, 203)
    assert r["plan"]["twin"] and r["plan"]["fallback_reason"].startswith("level 4: down4.c1"), r["plan"]
    _check(r, 4, ("slots", "slots", "fp32->slots", "fp32->slots"), "A3 anymap 200")


@pytest.mark.parametrize("B,H", [(4, 256), (1, 224)], ids=["4x1x256", "1x1x224"])
def test_a4_ragged_domain_inputs_are_the_ragged_plan_bit_for_bit(dev, B, H):
    """A4: 4 x 1 x 256^2 and 1 x 1 x 224^2 -- every level the plan takes lies in the ragged domain -- under the new value: the five
    outputs, scores and segment(head="fused") bit-identical to "bf16+pool+ragged", the same plan and the same launch records (MFMA
    kinds and every other entry point)"""
    import onet_amd
    from onet_amd import ops
    m = e16._onet(e16._prefixed(orc.det_state_dict(1, 1981)), 1, True, dev)
    Xg = orc.det_input(B, 1, H, H, seed=204).to(dev)
    got = {}
    m.settings = ops.Settings(conv="bf16", fused_eval=RAGGED)
    with torch.no_grad():
        m(Xg)                   # (the weight packs are made on first use: not part of either record)
    for value in (RAGGED, VALUE):
        m.settings = ops.Settings(conv="bf16", fused_eval=value)
        got[value] = (fh._mfma_kinds(lambda: m(Xg)), fh._mfma_kinds(lambda: onet_amd.scores(m, Xg)),
                      fh._mfma_kinds(lambda: onet_amd.segment(m, Xg, head="fused")), onet_amd.fused_eval_plan(m, Xg.shape))
    a, b = got[RAGGED], got[VALUE]
    assert a[3] == b[3] and b[3]["fused"] and b[3]["depth"] == 4, (a[3], b[3])
    for (oa, ka, ra), (ob, kb, rb), what in zip(a[:3], b[:3], ("forward", "scores", "segment")):
        oa, ob = (oa, ob) if isinstance(oa, tuple) else ((oa,), (ob,))
        assert len(oa) == len(ob) and all(torch.equal(x, y) for x, y in zip(oa, ob)), what
        assert ka == kb and ra == rb and ka, (what, ka, kb, ra, rb)
