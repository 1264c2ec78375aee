"""Fused eval-mode inference (Settings.fused_eval, onet_amd/inference.py).

Kernel level: onet_conv3x3_split_fwd_pre_act -- the pre-split forward convolution (32x32x16 kernel) with BatchNorm(eval) + ReLU in its
epilogue and the output as slots -- against the two-pass form built from existing entry points: the PLAIN pre-split forward launch
(the same device kernel without the epilogue) followed by onet_bn_relu_apply_split with the same coefficients and scale slots.  The
claim is bit identity, so there is no tolerance: the 16-bit words of the slots, the optional fp32 tensor and the recorded maximum are
compared with torch.equal.  onet_conv3x3_act_bound against its closed form in fp64.

Model level: the plan against the fp64 oracle (`orc.onet_forward(..., training=False)`) with the bounds and input recipes of
tests/test_gpu_inference.py (helpers copied from there): every output within 2e-4 of its tensor's largest magnitude, labels equal
where the fp64 margin |Vt - Vd| exceeds 1e-3 max |V|, those pixels more than 0.9 of all."""
import numpy as np
import pytest
import torch

from oracle import onet_oracle as orc

from multi_tile import multi_tile_cout

pytestmark = pytest.mark.gpu

TOL = 2e-4          # eval outputs, of each tensor's largest magnitude (tests/test_gpu_inference.py)
MARGIN = 1e-3       # labels compared where |Vt - Vd| exceeds this fraction of max |V| (fp64)
GAMMA_R1 = 1.0e5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from onet_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def rnd(*shape, seed=0, scale=1.0):
    g = np.random.Generator(np.random.PCG64([seed, *shape]))
    return torch.from_numpy((g.standard_normal(shape) * scale).astype(np.float32))


def _pack(w):
    from onet_amd import ops
    with ops.using(ops.Settings(conv="auto", split_f16=True)):
        qf, _ = ops.pack3x3_split(w)
    assert qf.dtype == torch.float16
    return qf


def _slot_max(slots):
    return float(slots.view(torch.float32).max())


def _save(Cout, seed, dev, gain=1.0):
    """[4][Cout] coefficients in bn_eval_coeffs' format (mean, invstd, sc = gamma invstd, sh = beta): about half of relu's inputs
    negative"""
    mean, sc, sh = rnd(Cout, seed=seed, scale=0.1), rnd(Cout, seed=seed + 1).abs() + 0.5, rnd(Cout, seed=seed + 2, scale=0.3)
    sc = sc * torch.where(rnd(Cout, seed=seed + 3) > 1.0, -1.0, 1.0)             # (a few negative BatchNorm weights)
    return torch.stack([mean, torch.ones(Cout), sc * gain, sh * gain]).contiguous().to(dev)


def _bound64(w, save, m1, m2, sc_ch):
    w, s = w.double().cpu().abs(), save.double().cpu()
    S1 = w[:, :sc_ch].sum((1, 2, 3)) if sc_ch else w.sum((1, 2, 3))
    S2 = w[:, sc_ch:].sum((1, 2, 3)) if sc_ch else torch.zeros_like(S1)
    return float((s[2].abs() * (S1 * m1 + S2 * m2) + (s[3] - s[0] * s[2]).abs()).max())


def _check_fused(dev, P, w, save, x_slots, x_slots2=None, split_ch=0, want_guard=False, what=""):
    """fused launch == plain launch + bn_relu_apply_split, bit for bit; bound and exact maximum -> max |a|"""
    from onet_amd import ops
    B, _, H, _, W, _ = P.shape
    Cout = w.shape[0]
    qf = _pack(w.to(dev))
    scale = ops.conv3x3_act_bound(w.to(dev), save, x_slots, x_slots2, split_ch)
    z = ops.conv3x3_split_pre(P, qf, Cout, out=torch.full((B, Cout, H, W), float("nan"), device=dev), slots=x_slots, slots2=x_slots2,
                              split_ch=split_ch)
    aP0 = torch.full((B, Cout // 8, H, 2, W, 8), float("nan"), dtype=torch.float16, device=dev)
    a0 = torch.full((B, Cout, H, W), float("nan"), device=dev)
    ops.bn_relu_apply_split(z, save, aP0, a=a0, slots=scale)
    aP1 = torch.full_like(aP0, float("nan"))
    a1 = torch.full_like(a0, float("nan"))
    am = torch.zeros(ops.AMAX_SLOTS, dtype=torch.int32, device=dev)
    got = ops.conv3x3_split_pre_act(P, qf, Cout, save, scale, out=aP1, slots=x_slots, slots2=x_slots2, split_ch=split_ch, a_amax=am, a=a1)
    torch.cuda.synchronize()
    assert got is aP1, what
    assert torch.isfinite(a0).all() and torch.isfinite(aP0.float()).all(), what
    assert torch.equal(aP1.view(torch.int16), aP0.view(torch.int16)), f"{what}: slots differ from the two-pass form"
    assert torch.equal(a1, a0), f"{what}: fp32 activation differs from the two-pass form"
    amax = float(a0.abs().max())
    assert _slot_max(am) == amax, (what, _slot_max(am), amax)
    assert bool((a0 == 0).any()) and bool((a0 > 0).any()), what
    # without the optional outputs: the same slots
    aP2 = torch.full_like(aP0, float("nan"))
    ops.conv3x3_split_pre_act(P, qf, Cout, save, scale, out=aP2, slots=x_slots, slots2=x_slots2, split_ch=split_ch)
    assert torch.equal(aP2.view(torch.int16), aP0.view(torch.int16)), what
    # the bound: >= the exact maximum, == the closed form in fp64 up to one fp32 rounding upward
    m1 = _slot_max(x_slots)
    m2 = _slot_max(x_slots2) if x_slots2 is not None else m1
    closed = _bound64(w, save, m1, m2, split_ch)
    v = _slot_max(scale)
    print(f"{what}: max a {amax:.4e}, bound {v:.4e} (closed form {closed:.4e}, looseness {v / amax:.1f}x)")
    assert v >= amax, (what, v, amax)
    assert closed <= v * (1 + 1e-12) and v <= closed * (1 + 2.0 ** -22), (what, v, closed)
    if want_guard:
        assert v >= 2.0 ** 15, (what, v)
    return v


@pytest.mark.parametrize("B,Cin,Cout,H,W", [(2, 64, 128, 128, 128), (1, 256, 256, 64, 64), (1, 1024, 512, 32, 32), (3, 32, None, 48, 96)],
                         ids=["64-128@128", "256-256@64", "1024-512@32", "multi-tile"])
def test_fused_epilogue_bit_identical(dev, B, Cin, Cout, H, W):
    """64 -> 128 at 128 x 128, 256 -> 256 at 64 x 64, 1024 -> 512 at 32 x 32.  Measured looseness of the bound (bound / max a): 29x, 69x,
    136x -- it grows with sum |w| over the effective gain, i.e. with sqrt(Cin).  multi-tile: Cout = multi_tile_cout(27), where blocks
    walk more than one tile and the coefficient double buffer turns over."""
    from onet_amd import ops
    if Cout is None:
        Cout = multi_tile_cout(B * (H // 16) * (W // 32))
    x = rnd(B, Cin, H, W, seed=200).abs().to(dev)
    w = rnd(Cout, Cin, 3, 3, seed=201, scale=(2.0 / (Cin * 9)) ** 0.5)
    s = ops.absmax_slots(x)
    P = ops.split_pack_act(x, f16=True, slots=s)
    _check_fused(dev, P, w, _save(Cout, 202, dev), s, what=f"fused {(B, Cin, Cout, H, W)}")


@pytest.mark.parametrize("big_first", [True, False], ids=["big-skip", "big-up"])
def test_fused_epilogue_two_producer_concat(dev, big_first):
    """A concat input with two producers' slot sets and split_ch (tests/test_gpu_presplit_kernels.py): one half at 1e5 (its guard
    exponent non-zero), the other at 1e-1."""
    from onet_amd import ops
    B, Cin, Cout, H, W, sc = 2, 128, 64, 32, 64, 64
    a = (rnd(B, sc, H, W, seed=210) * (1e5 if big_first else 1e-1)).to(dev)
    b = (rnd(B, Cin - sc, H, W, seed=211) * (1e-1 if big_first else 1e5)).to(dev)
    P = torch.empty((B, Cin // 8, H, 2, W, 8), dtype=torch.float16, device=dev)
    s1, s2 = ops.absmax_slots(a), ops.absmax_slots(b)
    ops.split_pack_act(a, f16=True, slots=s1, out=P[:, :sc // 8])
    ops.split_pack_act(b, f16=True, slots=s2, out=P[:, sc // 8:])
    w = rnd(Cout, Cin, 3, 3, seed=212, scale=(2.0 / (Cin * 9)) ** 0.5)
    save = _save(Cout, 213, dev, gain=1e-4)
    _check_fused(dev, P, w, save, s1, s2, sc, what=f"concat, big half {'first' if big_first else 'second'}")


def test_fused_epilogue_output_guard(dev):
    """`save` scaled so that the bound reaches 2^15: the output's guard exponent is non-zero and the slots stay finite."""
    from onet_amd import ops
    B, Cin, Cout, H, W = 1, 64, 64, 32, 64
    x = rnd(B, Cin, H, W, seed=220).abs().to(dev)
    w = rnd(Cout, Cin, 3, 3, seed=221, scale=(2.0 / (Cin * 9)) ** 0.5)
    s = ops.absmax_slots(x)
    P = ops.split_pack_act(x, f16=True, slots=s)
    _check_fused(dev, P, w, _save(Cout, 222, dev, gain=3.0e4), s, want_guard=True, what="output guard")


@pytest.mark.parametrize("Cout,H,W", [(64, 32, 48), (64, 24, 64), (96, 32, 64)], ids=["W48", "H24", "Cout96"])
def test_fused_epilogue_refuses(dev, Cout, H, W):
    """Outside the kernel's domain the entry point returns 1 and writes nothing."""
    from onet_amd import ops, _lib
    B, Cin = 1, 32
    x = rnd(B, Cin, H, W, seed=230).to(dev)
    s = ops.absmax_slots(x)
    P = ops.split_pack_act(x, f16=True, slots=s)
    w = rnd(Cout, Cin, 3, 3, seed=231, scale=0.1).to(dev)
    qf, save = _pack(w), _save(Cout, 232, dev)
    scale = ops.conv3x3_act_bound(w, save, s)
    aP = torch.full((B, Cout // 8, H, 2, W, 8), 7.0, dtype=torch.float16, device=dev)
    a = torch.full((B, Cout, H, W), 7.0, device=dev)
    am = torch.zeros(ops.AMAX_SLOTS, dtype=torch.int32, device=dev)
    rc = _lib.load().onet_conv3x3_split_fwd_pre_act(P.data_ptr(), Cin * H * W, s.data_ptr(), 0, None, 0, qf.data_ptr(), save.data_ptr(),
                                                    aP.data_ptr(), Cout * H * W, scale.data_ptr(), am.data_ptr(), a.data_ptr(), Cout * H * W,
                                                    B, Cin, Cout, H, W, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 1
    assert bool((aP == 7.0).all()) and bool((a == 7.0).all()) and int(am.abs().max()) == 0
    assert ops.conv3x3_split_pre_act(P, qf, Cout, save, scale, out=aP) is None


# ----------------------------------------------------------------------------- model level (helpers of tests/test_gpu_inference.py)
def close(a, b, tol, what=""):
    """-> max |a - b| / max |b|, asserted <= tol (b: the fp64 oracle)."""
    a = a.detach().cpu().double()
    b = b.detach().cpu().double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert torch.isfinite(a).all(), f"{what}: non-finite output"
    scale = float(b.abs().max()) + 1e-30
    err = float((a - b).abs().max()) / scale
    assert err <= tol, f"{what}: max err {err:.3e} of scale {scale:.3e} (tol {tol})"
    return err


def _f64(sd):
    return {k: (v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu().clone()) for k, v in sd.items()}


def _prefixed(top, dwn=None):
    sd = {"topu." + k: v for k, v in top.items()}
    sd.update({"dwnu." + k: v for k, v in (top if dwn is None else dwn).items()})
    return sd


def _gamma(sd, g):
    return {k: (v * g if k.endswith(".weight") and v.dim() == 1 else v) for k, v in sd.items()}


def _onet(sd, C, bshare, dev):
    import Onet_vanilla_20240606 as ov
    m = ov.Onet(in_chns=C, binit=True, bshare=bshare)
    m.load_state_dict(sd)
    return m.to(dev).eval()


def _oracle(X, top, dwn=None, bias=0.0):
    with torch.no_grad():
        return orc.onet_forward(X.double(), _f64(top), None if dwn is None else _f64(dwn), training=False, bias=bias)


def _calibrated(top, X, bias=0.0, crop=None):
    Xc = X if crop is None else X[..., :crop, :crop]
    return orc.calibrated_state(top, torch.cat([Xc, torch.clip(1 - Xc + bias, 0, 1)]))


def _eval(m, X, settings=None, grad=False):
    """-> (outputs, {kind: launches} of the MFMA kernels) of one eval forward"""
    from onet_amd import ops
    if settings is not None:
        m.settings = settings
    ops.profile_start(everything=False)
    try:
        with torch.set_grad_enabled(grad):
            out = m(X)
        torch.cuda.synchronize()
    finally:
        prof, _ = ops.profile_stop()
    return out, {k: len(v) for k, v in prof.items()}


def _margin(ref, margin=MARGIN):
    Vt, Vd = ref[1][:, 0], ref[3][:, 0]
    return (Vt - Vd).abs() > margin * float(torch.maximum(Vt.abs().max(), Vd.abs().max()))


def _compare(m, out, ref, tol, what):
    errs = {n: float((a.detach().cpu().double() - b).abs().max()) / (float(b.abs().max()) + 1e-30)
            for a, b, n in zip(out, ref, ("Lt", "Vt", "Ld", "Vd", "S"))}
    print(f"{what}: " + ", ".join(f"{n} {e:.2e}" for n, e in errs.items()))
    for a, b, n in zip(out, ref, ("Lt", "Vt", "Ld", "Vd", "S")):
        close(a, b, tol, f"{what} {n}")
        assert a.dtype == torch.float32 and a.is_cuda and a.grad_fn is None and tuple(a.shape) == tuple(b.shape), (what, n)
    sure = _margin(ref, max(MARGIN, 2 * tol))
    assert float(sure.double().mean()) > 0.9, what
    assert torch.equal(m.predict_label(out[4]).cpu().long()[sure], orc.predict_label(ref[4]).long()[sure]), what
    return max(errs.values())


def _fused():
    from onet_amd import ops
    return ops.Settings(fused_eval=True)


def _traced(m, X):
    """one fused forward with inference.TRACE on -> (outputs, [(layer, bound, exact max |a| of the slots)])"""
    import math
    from onet_amd import inference
    inference.TRACE = []
    try:
        with torch.no_grad():
            out = m(X)
        torch.cuda.synchronize()
        rows = []
        for name, t in inference.TRACE:
            bound = _slot_max(t.scale)
            k = 13 - math.floor(math.log2(bound)) if bound >= 2.0 ** 15 else 0        # the guard exponent the slots select
            exact = float(t.P.float().sum(3).abs().max()) * 2.0 ** -k
            rows.append((name, bound, exact))
    finally:
        inference.TRACE = None
    return out, rows


def _check_bounds(rows, what):
    """every tensor the plan wrote as slots lies under the bound it was scaled by -> the worst bound / exact ratio"""
    for name, bound, exact in rows:
        assert math_isfinite(bound) and bound >= exact * (1 - 1e-3), (what, name, bound, exact)
    worst = max(rows, key=lambda r: r[1] / max(r[2], 1e-30))
    print(f"{what}: bound / exact max per tensor: " + ", ".join(f"{n} {b / max(e, 1e-30):.0f}x" for n, b, e in rows))
    print(f"{what}: worst chained looseness {worst[1] / max(worst[2], 1e-30):.0f}x ({worst[0]})")
    return worst[1] / max(worst[2], 1e-30)


def math_isfinite(v):
    import math
    return math.isfinite(v)


def _assert_plan_matches(plan, kinds, what):
    """the launch records of a fused forward against what fused_eval_plan announced"""
    assert plan["fused"], (what, plan)
    n = {k: sum(1 for v in plan["layers"].values() if v == k) for k in ("fused", "two-pass", "plain+head")}
    passes = 1 if plan.get("twin", True) else 2
    assert kinds.get("conv3x3_split_pre_act_kernel", 0) == passes * n["fused"], (what, kinds, plan)
    assert kinds.get("conv3x3_split_pre_kernel", 0) == passes * (n["two-pass"] + n["plain+head"]), (what, kinds, plan)
    assert kinds.get("convt_slot_fwd_kernel", 0) == passes * sum(1 for v in plan["convt"].values() if v == "slots"), (what, kinds, plan)


def test_f1_fused_256_calibrated(dev):
    """F1: B = 2, 1 x 256^2, shared, calibrated (E1's recipe).  The 256- and 128-pixel levels are fused (depth 2): at this batch the
    default dispatch selects the in-staging split kernel on exactly those levels, so the fused forward must launch none; the
    launch records agree with fused_eval_plan; a second call is bit-equal; running statistics and counters are untouched;
    segment() == predict_label(S).  Then the same model under conv = "split": depth 4.  Every slot tensor of both runs lies under its
    bound.  Measured worst errors 5.6e-5 (S; logits 6.9e-6; the default path: 7.0e-5), depth 4: 7.0e-5; worst bound / exact maximum
    4159x (down1.c1: two chained bounds), depth 4: 11549x (up1.c1)."""
    import onet_amd
    B, H = 2, 256
    X = orc.det_input(B, 1, H, H, seed=101)
    top = _calibrated(orc.det_state_dict(1, 1981), X)
    ref = _oracle(X, top)
    m = _onet(_prefixed(top), 1, True, dev)
    Xg = X.to(dev)
    buf0 = {k: v.clone() for k, v in m.state_dict().items() if "running" in k or "num_batches" in k}
    m.settings = _fused()
    plan = onet_amd.fused_eval_plan(m, Xg.shape)
    assert plan["fused"] and plan["depth"] == 2 and plan["twin"] and plan["batch"] == 2 * B, plan
    assert plan["layers"]["down1.c1"] == "fused" and plan["layers"]["inc.c2"] == "two-pass" and plan["layers"]["down2.c1"] == "fallback"
    out, kinds = _eval(m, Xg)
    assert kinds.get("conv3x3_split_pre_act_kernel", 0) > 0 and kinds.get("convt_slot_fwd_kernel", 0) > 0, kinds
    assert "conv3x3_split_kernel" not in kinds, kinds
    _assert_plan_matches(plan, kinds, "F1")
    print(f"F1 worst error {_compare(m, out, ref, TOL, 'F1'):.2e}")
    with torch.no_grad():
        out2 = m(Xg)
    assert all(torch.equal(a, b) for a, b in zip(out, out2))
    for k, v in m.state_dict().items():
        if k in buf0:
            assert torch.equal(v, buf0[k]), k
    lab = onet_amd.segment(m, Xg)
    assert lab.dtype == torch.int64 and tuple(lab.shape) == (B, H, H)
    assert torch.equal(lab, m.predict_label(out[4]))
    out3, rows = _traced(m, Xg)
    assert all(torch.equal(a, b) for a, b in zip(out, out3))
    _check_bounds(rows, "F1")
    # depth 4 (what the B = 32 benchmark shape takes): conv = "split" takes the split kernels on every legal layer, so the 64- and
    # 32-pixel levels are fused too and the 16-pixel bottleneck crosses the fp32 boundary both ways
    from onet_amd import ops
    m.settings = ops.Settings(conv="split", fused_eval=True)
    plan4 = onet_amd.fused_eval_plan(m, Xg.shape)
    assert plan4["fused"] and plan4["depth"] == 4 and plan4["layers"]["down4.c1"] == "fallback", plan4
    assert plan4["convt"] == {"up4": "slots", "up3": "slots", "up2": "slots", "up1": "fp32->slots"}, plan4
    out4, kinds4 = _eval(m, Xg)
    _assert_plan_matches(plan4, kinds4, "F1 depth 4")
    print(f"F1 depth 4 worst error {_compare(m, out4, ref, TOL, 'F1 depth 4'):.2e}")
    _check_bounds(_traced(m, Xg)[1], "F1 depth 4")


def test_f2_fused_512_rgb(dev):
    """F2: B = 1, 3 x 512^2 (E2's ZY-3 tile), shared, calibrated.  The twin batch holds two images: the 512-, 256- and 128-pixel levels
    have the tiles the dispatch asks of the split kernels (depth 3); the 64- and 32-pixel levels (128 and 64 tiles, below three
    quarters of the compute units) stay on the existing kernels, as they do on the default path.  Then conv = "split": depth 5.  Measured worst errors 7.2e-5 (S; logits
    6.9e-6), depth 5: 6.5e-5; worst bound / exact maximum at depth 5: 13808x (up1.c1)."""
    import onet_amd
    B, C, H = 1, 3, 512
    X = orc.det_input(B, C, H, H, seed=102)
    top = _calibrated(orc.det_state_dict(C, 1981), X, crop=256)
    ref = _oracle(X, top)
    m = _onet(_prefixed(top), C, True, dev)
    m.settings = _fused()
    plan = onet_amd.fused_eval_plan(m, X.shape)
    assert plan["fused"] and plan["depth"] == 3, plan
    out, kinds = _eval(m, X.to(dev))
    _assert_plan_matches(plan, kinds, "F2")
    print(f"F2 worst error {_compare(m, out, ref, TOL, 'F2'):.2e}")
    # depth 5: under conv = "split" every level down to the 32-pixel bottleneck is fused (down4.c1 / down4.c2 fused, every
    # ConvTranspose2d on slot operands, no fp32 level)
    from onet_amd import ops
    m.settings = ops.Settings(conv="split", fused_eval=True)
    plan5 = onet_amd.fused_eval_plan(m, X.shape)
    assert plan5["fused"] and plan5["depth"] == 5 and plan5["fallback_reason"] is None, plan5
    assert "fallback" not in plan5["layers"].values() and set(plan5["convt"].values()) == {"slots"}, plan5
    out5, kinds5 = _eval(m, X.to(dev))
    _assert_plan_matches(plan5, kinds5, "F2 depth 5")
    assert "conv3x3_split_kernel" not in kinds5 and "convt_gemm_kernel" not in kinds5, kinds5
    print(f"F2 depth 5 worst error {_compare(m, out5, ref, TOL, 'F2 depth 5'):.2e}")
    _check_bounds(_traced(m, X.to(dev))[1], "F2 depth 5")


def test_f3_fused_unshared_bias(dev):
    """F3: bshare=False (two passes of B = 2: only the 256-pixel level has the tiles, depth 1), bias 0.3, the randomised running
    statistics of det_state_dict (E3's recipe).  Measured worst error 4.4e-6 (Vt)."""
    import onet_amd
    B, H = 2, 256
    X = orc.det_input(B, 1, H, H, seed=103)
    top, dwn = orc.det_state_dict(1, 1981), orc.det_state_dict(1, 1982)
    ref = _oracle(X, top, dwn, bias=0.3)
    m = _onet(_prefixed(top, dwn), 1, False, dev)
    m.bias = 0.3
    m.settings = _fused()
    plan = onet_amd.fused_eval_plan(m, X.shape)
    assert plan["fused"] and not plan["twin"] and plan["depth"] >= 1, plan
    out, kinds = _eval(m, X.to(dev))
    _assert_plan_matches(plan, kinds, "F3")
    print(f"F3 worst error {_compare(m, out, ref, TOL, 'F3'):.2e}")


def test_f4_fused_after_training_steps(dev):
    """F4: two FlatAdam steps (E6's recipe), then the fused eval against an oracle built from the model's state at that point: no
    pack, coefficient or bound is stale.  Measured worst error 5.9e-5 (S; logits 5.6e-6)."""
    from onet_amd.trainer import FlatAdam
    B, H = 2, 256
    X = orc.det_input(B, 1, H, H, seed=106)
    top = _calibrated(orc.det_state_dict(1, 1981), X)
    m = _onet(_prefixed(top), 1, True, dev)
    m.settings = _fused()
    Xg = X.to(dev)
    with torch.no_grad():
        before = m(Xg)                      # a fused forward BEFORE the steps: whatever it cached must not survive them
    m.train()
    opt = FlatAdam(m, lr=1e-4)
    Xt = orc.det_input(B, 1, H, H, seed=107).to(dev)
    for _ in range(2):
        opt.zero_grad()
        Lt, Vt, Ld, Vd, S = m(Xt)
        m.compute_loss(Lt, S[:, 0:1], Ld, S[:, 1:2]).backward()
        opt.step()
    m.eval()
    sd = {k[5:]: v for k, v in m.state_dict().items() if k.startswith("topu.")}
    assert int(sd["inc.double_conv.1.num_batches_tracked"]) == 4
    ref = _oracle(X, sd)
    out, kinds = _eval(m, Xg)
    assert kinds.get("conv3x3_split_pre_act_kernel", 0) > 0, kinds
    assert not torch.equal(out[1], before[1])
    print(f"F4 worst error {_compare(m, out, ref, TOL, 'F4'):.2e}")


def test_f5_fused_range_guard(dev):
    """F5: R1's recipe (B = 4, 1 x 128^2, every BatchNorm weight times 1e5, calibrated; the oracle's Lt passes 65504): every fused
    tensor's bound selects a non-zero guard exponent.  Outputs finite and within the same bound; S on the margin pixels only.  Measured worst error 7.4e-6 (depth 1)."""
    import onet_amd
    B, H = 4, 128
    X = orc.det_input(B, 1, H, H, seed=108)
    top = _calibrated(_gamma(orc.det_state_dict(1, 1981, head_gain=0.3), GAMMA_R1), X)
    ref = _oracle(X, top)
    assert float(ref[0].abs().max()) > 65504
    m = _onet(_prefixed(top), 1, True, dev)
    m.settings = _fused()
    plan = onet_amd.fused_eval_plan(m, X.shape)
    assert plan["fused"] and plan["depth"] >= 1, plan
    out, kinds = _eval(m, X.to(dev))
    _assert_plan_matches(plan, kinds, "F5")
    errs = [close(a, b, TOL, f"F5 {n}") for a, b, n in zip(out[:4], ref[:4], ("Lt", "Vt", "Ld", "Vd"))]
    sure = _margin(ref)
    assert torch.isfinite(out[4]).all()
    assert float((out[4].cpu().double() - ref[4]).abs().permute(1, 0, 2, 3)[:, sure].max()) <= TOL
    print(f"F5 worst error {max(errs):.2e} (depth {plan['depth']})")
    rows = _traced(m, X.to(dev))[1]
    assert all(b >= 2.0 ** 15 for _, b, _ in rows), rows           # every fused tensor's guard exponent is non-zero
    _check_bounds(rows, "F5")


def test_f8_unet_alone(dev):
    """F8: UNet.forward on its own (no Onet, no head: the last activation is materialised by one BatchNorm + ReLU pass), B = 4,
    1 x 256^2, calibrated, against orc.unet_pass(..., training=False); the default path of the same module for comparison.
    Measured: y1 9.0e-6 fused, 9.9e-6 default; x1 9.0e-7 both."""
    import Onet_vanilla_20240606 as ov
    from onet_amd import ops
    B, H = 4, 256
    X = orc.det_input(B, 1, H, H, seed=114)
    sd = orc.calibrated_state(orc.det_state_dict(1, 1981), X)
    with torch.no_grad():
        ref = orc.unet_pass(X.double(), _f64(sd), training=False)
    u = ov.UNet(n_channels=1, bilinear=False)
    u.load_state_dict(sd)
    u = u.to(dev).eval()
    res = {}
    for name, st in (("default", ops.Settings()), ("fused", ops.Settings(fused_eval=True))):
        ops.profile_start(everything=False)
        try:
            with torch.no_grad(), ops.using(st):
                res[name] = u(X.to(dev))
            torch.cuda.synchronize()
        finally:
            kinds = set(ops.profile_stop()[0])
        assert ("conv3x3_split_pre_act_kernel" in kinds) == (name == "fused"), (name, sorted(kinds))
        errs = [close(a, b, TOL, f"F8 {name} {n}") for a, b, n in zip(res[name], ref, ("x1", "y1"))]
        print(f"F8 {name}: x1 {errs[0]:.2e}, y1 {errs[1]:.2e}")
    assert all(t.grad_fn is None and t.dtype == torch.float32 for t in res["fused"])


def test_f6_fallbacks_are_the_default_path(dev):
    """F6: where a precondition fails the call runs today's path: outputs torch.equal to the default Settings()', no fused launch.
    A 120 x 200 input (no level made of full tiles), a registered forward hook, conv = "bf16", and a call with grad enabled."""
    import onet_amd
    from onet_amd import ops
    sd = _prefixed(orc.det_state_dict(1, 1981))
    m = _onet(sd, 1, True, dev)
    Xs = {"120x200": orc.det_input(2, 1, 120, 200, seed=111).to(dev), "256": orc.det_input(2, 1, 256, 256, seed=112).to(dev)}

    def both(X, st_default, st_fused, grad=False, what=""):
        a, ka = _eval(m, X, st_default, grad=grad)
        b, kb = _eval(m, X, st_fused, grad=grad)
        assert "conv3x3_split_pre_act_kernel" not in kb and "convt_slot_fwd_kernel" not in kb, (what, kb)
        assert ka == kb, (what, ka, kb)
        assert all(torch.equal(x.detach(), y.detach()) for x, y in zip(a, b)), what

    both(Xs["120x200"], ops.Settings(), _fused(), what="120x200")
    m.settings = _fused()
    p = onet_amd.fused_eval_plan(m, Xs["120x200"].shape)
    assert not p["fused"] and "level 0" in p["reason"], p
    both(Xs["256"], ops.Settings(conv="bf16"), ops.Settings(conv="bf16", fused_eval=True), what="bf16")
    both(Xs["256"], ops.Settings(), _fused(), grad=True, what="grad enabled")
    h = m.topu.down1.register_forward_hook(lambda mod, inp, out: None)
    try:
        both(Xs["256"], ops.Settings(), _fused(), what="hook")
        m.settings = _fused()
        assert "hook" in onet_amd.fused_eval_plan(m, Xs["256"].shape)["reason"]
    finally:
        h.remove()
    # ... and with nothing in the way the same model and input take the plan
    _, k = _eval(m, Xs["256"], _fused())
    assert k.get("conv3x3_split_pre_act_kernel", 0) > 0, k


def test_f7_default_settings_keep_the_eval_path(dev):
    """F7: the setting is off by default: with Settings() an eval forward launches exactly the kinds, and as many of each, as the
    existing path -- no pre-split kernel at all -- and is bit-equal to Settings(fused_eval=False)."""
    from onet_amd import ops
    assert ops.FUSED_EVAL is False and ops.Settings().fused_eval is None
    m = _onet(_prefixed(orc.det_state_dict(1, 1981)), 1, True, dev)
    X = orc.det_input(2, 1, 256, 256, seed=113).to(dev)
    a, ka = _eval(m, X, ops.Settings())
    b, kb = _eval(m, X, ops.Settings(fused_eval=False))
    print("F7 kinds:", ka)
    assert ka == kb and all(torch.equal(x, y) for x, y in zip(a, b))
    # the launches of the existing eval path at this shape, counted on the commit before the setting existed: the stem and the 64-,
    # 32- and 16-pixel levels on the direct kernel (11), the 256- and 128-pixel levels on the in-staging split kernel (7), the four
    # ConvTranspose2d GEMMs -- and nothing else
    assert ka == {"conv_fwd_kernel": 11, "conv3x3_split_kernel": 7, "convt_gemm_kernel": 4}, ka


def _slot_writers(plan):
    """The names inference.TRACE must list for one pass, in execution order, from the plan dictionary alone: going down, every unit of a
    fused level that writes slots (on the one-part plan also `<block>.pool` where the pooled tensor leaves as slots, i.e. where the
    next level is fused); coming back up, deepest fused Up block first, the ConvTranspose2d's channel groups, c1, and c2 where it is a
    fused launch (the last unit writes no slots)."""
    layers, convt = plan["layers"], plan["convt"]
    enc = [n for n in layers if n.split(".")[0] not in convt]
    names = []
    for i, n in enumerate(enc):
        if layers[n] == "fallback":
            break
        names.append(n)
        if layers[n] == "two-pass" and plan["operands"] == "bf16" and i + 1 < len(enc) and layers[enc[i + 1]] != "fallback":
            names.append(n.split(".")[0] + ".pool")
    for u in reversed([u for u, kind in convt.items() if kind != "fallback"]):
        names += [u + ".up", u + ".c1"] + ([u + ".c2"] if layers[u + ".c2"] == "fused" else [])
    return names


@pytest.mark.parametrize("conv,fused_eval", [("split", True), ("bf16", "bf16"), (None, True)])
def test_f9_trace_and_launches_follow_the_plan_dictionary(dev, conv, fused_eval):
    """The executor does what the query announces, on the smallest input whose level-4 map is one full 16 x 32 tile (B = 1, 1 x 256 x
    512, shared: a twin batch of 2): conv = "split" / "bf16" fuse every level with every ConvTranspose2d on slot operands on a
    256-compute-unit device, the default dispatch leaves a fall-back tail.  Every expected value comes from the dictionary:
    inference.TRACE lists, per pass and in order, the slot-writing units the dictionary lists; the launch records of m(X) and of
    segment(m, X, head="fused") match it (_assert_plan_matches' rule on either format's kinds), with exactly one head-epilogue launch
    per pass and no plain launch for the last unit where it says "fused+head"."""
    import onet_amd
    from onet_amd import inference, ops
    m = _onet(_prefixed(orc.det_state_dict(1, 1981)), 1, True, dev)
    m.settings = ops.Settings(fused_eval=fused_eval) if conv is None else ops.Settings(conv=conv, fused_eval=fused_eval)
    X = orc.det_input(1, 1, 256, 512, seed=131).to(dev)
    act, head_kind = {"fp16x2": ("conv3x3_split_pre_act_kernel", "conv3x3_split_pre_head_kernel"),
                      "bf16": ("conv3x3_pre16_act_kernel", "conv3x3_pre16_head_kernel")}[onet_amd.fused_eval_plan(m, X.shape)["operands"]]
    for head in (None, "fused"):
        plan = onet_amd.fused_eval_plan(m, X.shape, head=head)
        assert plan["fused"] and plan["depth"] >= 1, plan
        passes = 1 if plan["twin"] else 2
        n = {k: sum(1 for v in plan["layers"].values() if v == k) for k in ("fused", "two-pass", "plain+head", "fused+head")}
        assert n["plain+head"] + n["fused+head"] == 1 and (n["fused+head"] == 1) == (head == "fused"), plan
        inference.TRACE = []
        ops.profile_start(everything=False)
        try:
            with torch.no_grad():
                if head is None:
                    m(X)
                else:
                    onet_amd.segment(m, X, head="fused")
            torch.cuda.synchronize()
            traced = [name for name, _ in inference.TRACE]
        finally:
            kinds = {k: len(v) for k, v in ops.profile_stop()[0].items()}
            inference.TRACE = None
        what = (conv, fused_eval, head, plan["depth"])
        assert traced == _slot_writers(plan) * passes, (what, traced, _slot_writers(plan))
        assert kinds.get(act, 0) == passes * n["fused"], (what, kinds, plan)
        assert kinds.get("conv3x3_split_pre_kernel", 0) == passes * (n["two-pass"] + n["plain+head"]), (what, kinds, plan)
        assert kinds.get("convt_slot_fwd_kernel", 0) == passes * sum(1 for v in plan["convt"].values() if v == "slots"), (what, kinds, plan)
        assert kinds.get(head_kind, 0) == passes * n["fused+head"], (what, kinds, plan)
        other = {"conv3x3_split_pre_act_kernel", "conv3x3_pre16_act_kernel", "conv3x3_split_pre_head_kernel", "conv3x3_pre16_head_kernel"}
        assert not (other - {act, head_kind}) & set(kinds), (what, kinds)
