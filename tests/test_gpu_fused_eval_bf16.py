"""The one-part (plain bf16) fused eval plan, Settings(fused_eval="bf16") (onet_amd/inference.py).

Kernel level (K1 - K3): onet_conv3x3_plain16_fwd_pre_act -- conv3x3_pre16_kernel on plain bf16 operands with BatchNorm(eval) + ReLU in
its epilogue and the output as one-part bf16 slots -- against the two-pass form built from existing entry points (the plain launch of
the same kernel with an fp32 z, then onet_bn_relu_apply_split with nparts = 1): bit identity, torch.equal on the 16-bit words, the
optional fp32 tensor and the recorded maximum; and against fp64 with the plain-bf16 bounds of tests/test_gpu_presplit_kernels.py.

Model level (M1 - M3): the plan against the fp64 oracle.  bf16 operand rounding is a chaotic DECISION (oracle/onet_oracle.py,
`operand_rounding`): two evaluations whose activations differ in the last fp32 bits round a few 1e-4 of them to different bf16
neighbours, and that noise grows layer by layer to full bf16 level.  M1 therefore REPLAYS the run's own roundings: every slot tensor
the plan wrote is taken from inference.TRACE and handed to the oracle as the rounded input of the layer that read it (the oracle's
_check_replayed holds each to one bf16 ulp of its own fp64 value), after which the outputs must agree to the eval tolerance of
tests/test_gpu_fused_eval.py.  M2 measures the free-rounding noise of the oracle itself and bounds the HIP run's by twice that."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import onet_oracle as orc

pytestmark = pytest.mark.gpu

TOL = 2e-4          # eval outputs, of each tensor's largest magnitude (tests/test_gpu_fused_eval.py)
MARGIN = 1e-3       # labels compared where |Vt - Vd| exceeds this fraction of max |V| (fp64)
TOL_A = 2e-6        # plain bf16 forward against fp64 of the ROUNDED operands, of the term scale (tests/test_gpu_presplit_kernels.py)
NAMES = ("inc", "down1", "down2", "down3", "down4")
UNAMES = ("up4", "up3", "up2", "up1")            # inference.py's names: the Up block of level k (up4: the 256-pixel level's)


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


def _slot_max(slots):
    return float(slots.view(torch.float32).max())


def unslot(P):
    """one-part slots [B][C/8][H][1][W][8] bf16 -> fp64 [B][C][H][W] on the host (exact)"""
    B, C8, H, one, W, _ = P.shape
    assert one == 1 and P.dtype == torch.bfloat16
    return P.detach().cpu().double()[:, :, :, 0].permute(0, 1, 4, 2, 3).reshape(B, C8 * 8, H, W)


# ----------------------------------------------------------------------------------------------------------------- kernel level
K_SHAPES = [(2, 64, 64, 16, 32),          # one tile per image
            (2, 96, 64, 48, 96),          # 3 x 3 tiles: halos on every side, an odd chunk count
            (1, 512, 128, 32, 64),        # 16 chunks, two channel tiles
            (3, 32, 192, 128, 128)]       # one chunk per tile, 288 tiles: more than one per persistent block (the coefficient double buffer)
K_IDS = ["one-tile", "3x3-tiles", "16-chunks", "288-tiles"]
_K_CACHE = {}


def _k_case(dev, shape):
    """inputs, the two-pass form and the fused launch of one shape, computed once for K1 and K2"""
    from onet_amd import ops
    if shape in _K_CACHE:
        return _K_CACHE[shape]
    B, Cin, Cout, H, W = shape
    x = rnd(B, Cin, H, W, seed=300).to(torch.bfloat16).float()                        # bf16-exact: the one-part pack is lossless
    w = rnd(Cout, Cin, 3, 3, seed=301, scale=(2.0 / (Cin * 9)) ** 0.5)
    gamma = (rnd(Cout, seed=302).abs() + 0.5) * torch.where(rnd(Cout, seed=303) > 0.5, -1.0, 1.0)     # (mixed-sign sc)
    save = ops.bn_eval_coeffs(gamma.to(dev), rnd(Cout, seed=304, scale=0.3).to(dev), rnd(Cout, seed=305, scale=0.1).to(dev),
                              (rnd(Cout, seed=306) ** 2 + 0.5).to(dev), 1e-5)
    P = ops.split_pack_act(x.to(dev), parts=1)
    assert P.dtype == torch.bfloat16 and torch.equal(unslot(P), x.double())
    wq = ops.pack3x3_plain16(w.to(dev))[0]
    z = ops.conv3x3_split_pre(P, wq, Cout, out=torch.full((B, Cout, H, W), float("nan"), device=dev))
    assert z.dtype == torch.float32
    aP0 = torch.full((B, Cout // 8, H, 1, W, 8), float("nan"), dtype=torch.bfloat16, device=dev)
    ops.bn_relu_apply_split(z, save, aP0)
    a0 = ops.bn_relu_apply(z, save, out=torch.full((B, Cout, H, W), float("nan"), device=dev))
    aP1, a1 = torch.full_like(aP0, float("nan")), torch.full_like(a0, float("nan"))
    am = torch.zeros(ops.AMAX_SLOTS, dtype=torch.int32, device=dev)
    ops.profile_start(everything=False)
    try:
        got = ops.conv3x3_plain16_pre_act(P, wq, Cout, save, out=aP1, a_amax=am, a=a1)
        torch.cuda.synchronize()
    finally:
        kinds = {k: len(v) for k, v in ops.profile_stop()[0].items()}
    assert got is aP1 and kinds == {"conv3x3_pre16_act_kernel": 1}, kinds
    _K_CACHE[shape] = dict(x=x, w=w, save=save, P=P, wq=wq, aP0=aP0, a0=a0, aP1=aP1, a1=a1, am=am)
    return _K_CACHE[shape]


@pytest.mark.parametrize("shape", K_SHAPES, ids=K_IDS)
def test_k1_fused_epilogue_bit_identical(dev, shape):
    """K1: fused launch == plain launch (fp32 z) + bn_relu_apply_split (one part) on the slots, == bn_relu_apply on the fp32 tensor,
    recorded maximum == max a; without the optional outputs the same slots."""
    from onet_amd import ops
    c = _k_case(dev, shape)
    B, Cin, Cout, H, W = shape
    assert torch.isfinite(c["a0"]).all() and torch.isfinite(c["aP0"].float()).all()
    assert bool((c["a0"] == 0).any()) and bool((c["a0"] > 0).any())
    cut = float((c["a0"] == 0).double().mean())
    assert 0.3 < cut < 0.7, cut                                     # ReLU cuts about half
    assert torch.equal(c["aP1"].view(torch.int16), c["aP0"].view(torch.int16)), f"{shape}: slots differ from the two-pass form"
    assert torch.equal(c["a1"], c["a0"]), f"{shape}: fp32 activation differs from the two-pass form"
    assert _slot_max(c["am"]) == float(c["a0"].max()), (shape, _slot_max(c["am"]), float(c["a0"].max()))
    aP2 = torch.full_like(c["aP0"], float("nan"))
    assert ops.conv3x3_plain16_pre_act(c["P"], c["wq"], Cout, c["save"], out=aP2) is aP2
    torch.cuda.synchronize()
    assert torch.equal(aP2.view(torch.int16), c["aP0"].view(torch.int16)), shape


def test_k1_concat_groups_and_strided_fp32(dev):
    """K1: aP into the leading channel groups of a wider concat buffer, a into a batch-strided view: the same bits as the dense launch,
    the other groups and the gaps keep their fill pattern."""
    from onet_amd import ops
    shape = K_SHAPES[1]
    c = _k_case(dev, shape)
    B, Cin, Cout, H, W = shape
    cat = torch.full((B, (Cout + 64) // 8, H, 1, W, 8), 7.0, dtype=torch.bfloat16, device=dev)
    wide = torch.full((B, Cout + 8, H, W), 7.0, device=dev)
    out, a = cat[:, :Cout // 8], wide[:, :Cout]
    assert ops.conv3x3_plain16_pre_act(c["P"], c["wq"], Cout, c["save"], out=out, a=a) is out
    torch.cuda.synchronize()
    assert torch.equal(out.contiguous().view(torch.int16), c["aP0"].view(torch.int16))
    assert torch.equal(a.contiguous(), c["a0"])
    assert bool((cat[:, Cout // 8:] == 7.0).all()) and bool((wide[:, Cout:] == 7.0).all())


@pytest.mark.parametrize("shape", K_SHAPES, ids=K_IDS)
def test_k2_fused_epilogue_against_fp64(dev, shape):
    """K2: relu(bn(conv64(x, bf16(w)))) in fp64.  The fp32 activation within 2e-6 of the per-channel term scale
    |sc| (max |z64| + |mean|) + |sh|; the slots within one bf16 rounding, 2^-8 |a64|, plus that term.
    Measured on an MI355X, worst element as a fraction of its bound, K_SHAPES' order: fp32 a 0.20 / 0.22 / 0.67 / 0.14; slots 0.99 /
    0.99 / 0.99 / 1.00 (0.995: one bf16 rounding of a value just above a power of two uses the whole 2^-8 |a64|)."""
    c = _k_case(dev, shape)
    s = c["save"].detach().cpu().double()
    z64 = F.conv2d(c["x"].double(), c["w"].to(torch.bfloat16).double(), None, 1, 1)
    mean, sc, sh = (s[k].view(1, -1, 1, 1) for k in (0, 2, 3))
    a64 = torch.relu((z64 - mean) * sc + sh)
    term = TOL_A * (sc.abs() * (z64.abs().amax((0, 2, 3), keepdim=True) + mean.abs()) + sh.abs())
    ea = (c["a1"].detach().cpu().double() - a64).abs()
    eP = (unslot(c["aP1"]) - a64).abs()
    bound_P = 2.0 ** -8 * a64.abs() + term
    print(f"K2 {shape}: fp32 a worst {float((ea / term).max()):.3f} of its bound, slots worst {float((eP / bound_P).max()):.3f} of theirs")
    assert bool((ea <= term).all()), f"{shape}: fp32 activation {float((ea / term).max()):.3f} x the bound"
    assert bool((eP <= bound_P).all()), f"{shape}: slots {float((eP / bound_P).max()):.3f} x the bound"


@pytest.mark.parametrize("Cin,Cout,H,W", [(32, 64, 32, 48), (32, 64, 24, 64), (32, 96, 32, 64), (48, 64, 32, 64)],
                         ids=["W48", "H24", "Cout96", "Cin48"])
def test_k3_fused_epilogue_refuses(dev, Cin, Cout, H, W):
    """K3: outside the kernel's domain the entry point returns 1 and the wrapper None; nothing is written."""
    from onet_amd import ops, _lib
    B = 1
    P = ops.split_pack_act(rnd(B, Cin, H, W, seed=330).to(dev), parts=1)
    w = rnd(Cout, Cin, 3, 3, seed=331, scale=0.1).to(dev)
    wq = torch.zeros(Cin * 9 * Cout + 8, dtype=torch.bfloat16, device=dev) if Cin % 32 else ops.pack3x3_plain16(w)[0]
    save = ops.bn_eval_coeffs(torch.ones(Cout, device=dev), torch.zeros(Cout, device=dev), torch.zeros(Cout, device=dev),
                              torch.ones(Cout, device=dev), 1e-5)
    aP = torch.full((B, Cout // 8, H, 1, W, 8), 7.0, dtype=torch.bfloat16, device=dev)
    a = torch.full((B, Cout, H, W), 7.0, device=dev)
    am = torch.zeros(ops.AMAX_SLOTS, dtype=torch.int32, device=dev)
    rc = _lib.load().onet_conv3x3_plain16_fwd_pre_act(P.data_ptr(), Cin * H * W // 2, wq.data_ptr(), save.data_ptr(), aP.data_ptr(),
                                                      Cout * H * W // 2, am.data_ptr(), a.data_ptr(), Cout * H * W, B, Cin, Cout, H, W,
                                                      torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 1
    assert ops.conv3x3_plain16_pre_act(P, wq, Cout, save, out=aP, a_amax=am, a=a) is None
    torch.cuda.synchronize()
    assert bool((aP == 7.0).all()) and bool((a == 7.0).all()) and int(am.abs().max()) == 0


# ----------------------------------------------------------------------------------------------------------------- model level
def _f64(sd):
    return {k: (v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu().clone()) for k, v in sd.items()}


def _prefixed(top, dwn=None):
    sd = {"topu." + k: v for k, v in top.items()}
    sd.update({"dwnu." + k: v for k, v in (top if dwn is None else dwn).items()})
    return sd


def _onet(sd, C, bshare, dev):
    import Onet_vanilla_20240606 as ov
    m = ov.Onet(in_chns=C, binit=True, bshare=bshare)
    m.load_state_dict(sd)
    return m.to(dev).eval()


def _calibrated(top, X, bias=0.0):
    return orc.calibrated_state(top, torch.cat([X, torch.clip(1 - X + bias, 0, 1)]))


def _oracle(X, top, dwn=None, bias=0.0, rule=None, replay=None):
    with torch.no_grad():
        if rule is None:
            return orc.onet_forward(X.double(), _f64(top), None if dwn is None else _f64(dwn), training=False, bias=bias)
        with orc.operand_rounding(rule, replay):
            return orc.onet_forward(X.double(), _f64(top), None if dwn is None else _f64(dwn), training=False, bias=bias)


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


def _rel(a, b):
    """max |a - b| / max |b| (b: an fp64 oracle)"""
    return float((a.detach().cpu().double() - b).abs().max()) / (float(b.abs().max()) + 1e-30)


def _traced_run(m, Xg):
    """One forward with inference.TRACE on and the three ConvTranspose2d wrappers watched -> (outputs, {kind: launches},
    {name: [slot tensor per pass, in order]}, [per ConvTranspose2d call, in order: its bf16-rounded input as fp64 NCHW on the host, or
    None where the GEMM ran at fp32 level])."""
    from onet_amd import inference, ops
    convt = []
    real = {n: getattr(ops, n) for n in ("convT2x2_fwd", "convT2x2_fwd_p", "convT2x2_fwd_slots")}

    def fp32_input(x, Ct):
        # operand_bf16 = 1: the GEMM rounds its fp32 input to bf16 on load (to nearest even); 0 / 2: fp32-level arithmetic
        B, _, h, w = x.shape
        return x.detach().to(torch.bfloat16).cpu().double() if ops.convt_operand_bf16(B, h, w, Ct) == 1 else None

    def fwd(x, wq, bias, out, Ct, pt, pl):
        # onet_convT2x2_fwd takes the GEMM on its fast path only (convt_gemm_fwd's shape conditions); elsewhere -- the 8 x 8 bottleneck
        # map of a 128 x 128 input -- the direct fp32 kernel runs whatever operand_bf16 says
        B, Cin, h, w = x.shape
        gemm = (pt, pl) == (0, 0) and tuple(out.shape[2:]) == (2 * h, 2 * w) and Cin % 16 == 0 and Ct % 32 == 0 and (h * w) % 128 == 0 and w % 2 == 0
        convt.append(fp32_input(x, Ct) if gemm else None)
        return real["convT2x2_fwd"](x, wq, bias, out, Ct, pt, pl)

    def fwd_p(x, wq, bias, outP, Ct, pt, pl, slots=None):
        done = real["convT2x2_fwd_p"](x, wq, bias, outP, Ct, pt, pl, slots=slots)
        if done:
            convt.append(fp32_input(x, Ct))
        return done

    def fwd_slots(xP, wP, bias, outP, Ct, **kw):
        done = real["convT2x2_fwd_slots"](xP, wP, bias, outP, Ct, **kw)
        if done:
            convt.append(unslot(xP) if xP.shape[3] == 1 else None)
        return done

    inference.TRACE = []
    ops.convT2x2_fwd, ops.convT2x2_fwd_p, ops.convT2x2_fwd_slots = fwd, fwd_p, fwd_slots
    ops.profile_start(everything=False)
    try:
        with torch.no_grad():
            out = m(Xg)
        torch.cuda.synchronize()
        trace = {}
        for name, t in inference.TRACE:
            assert t.P is not None and t.P.shape[3] == 1 and t.scale is None and t.amax is None, name     # one part, no magnitude slots
            trace.setdefault(name, []).append(unslot(t.P))
    finally:
        kinds = {k: len(v) for k, v in ops.profile_stop()[0].items()}
        inference.TRACE = None
        for n, f in real.items():
            setattr(ops, n, f)
    return out, kinds, trace, convt


def _replay_lists(trace, convt, B, twin):
    """-> operand_rounding's replay lists in the ORACLE's call order -- per pass (X, then 1 - X) the 18 convolutions inc.c1 .. down4.c2,
    up1.c1 .. up4.c2 (deepest Up block first) and the four ConvTranspose2d layers up1 .. up4: (the run's rounded input | None, None) --
    plus the names of the convolutions that have one."""
    def get(name, p):
        ts = trace.get(name)
        if ts is None:
            return None
        return ts[0][p * B:(p + 1) * B] if twin else ts[p]

    def cat(a, b):
        assert (a is None) == (b is None)
        return None if a is None else torch.cat([a, b], dim=1)

    order = []
    for k, n in enumerate(NAMES):
        order.append((n + ".c1", lambda p, k=k: get(NAMES[k - 1] + ".pool", p) if k else None))
        order.append((n + ".c2", lambda p, n=n: get(n + ".c1", p)))
    for k in (3, 2, 1, 0):
        u = UNAMES[k]
        order.append((u + ".c1", lambda p, k=k, u=u: cat(get(NAMES[k] + ".c2", p), get(u + ".up", p))))
        order.append((u + ".c2", lambda p, u=u: get(u + ".c1", p)))
    replay = {"conv3x3": [], "convT2x2": []}
    on_slots = set()
    assert len(convt) == (4 if twin else 8), len(convt)
    for p in range(2):
        for name, src in order:
            x_r = src(p)
            replay["conv3x3"].append((x_r, None))
            if x_r is not None:
                on_slots.add(name)
        for i in range(4):
            x_r = convt[i] if twin else convt[4 * p + i]
            replay["convT2x2"].append((x_r[p * B:(p + 1) * B] if (twin and x_r is not None) else x_r, None))
    return replay, on_slots


def _rule_of(replay):
    """The rule that rounds exactly the layers that have a replayed (rounded) input: their forward product.  The oracle asks once per
    layer call, in call order, so the rule counts its calls per kind (a fresh rule per evaluation)."""
    calls = {"conv3x3": 0, "convT2x2": 0}

    def rule(kind, x_shape, w_shape):
        i = calls[kind]
        calls[kind] = i + 1
        x_r = replay[kind][i][0]
        assert x_r is None or tuple(x_r.shape) == tuple(x_shape), (kind, i, tuple(x_r.shape), x_shape)
        return {"fwd"} if x_r is not None else False
    return rule


def _expected_plan(m, plan, d):
    """the kinds fused_eval_plan must announce at depth d, from the names of inference._level_layers: the last decoder unit feeds the
    head, an encoder block's second unit is followed by the pooling pass, everything else on a fused level is one launch"""
    from onet_amd import inference
    layers = {"inc.c1": "stem"}
    levels = inference._level_layers(m.topu)
    assert [n for n, _ in levels[0]] == ["inc.c2", UNAMES[0] + ".c1", UNAMES[0] + ".c2"] and len(levels) == 5
    for k, lv in enumerate(levels):
        for n, _ in lv:
            layers[n] = "fallback" if k >= d else "plain+head" if n == UNAMES[0] + ".c2" else \
                "two-pass" if (n.endswith(".c2") and n.split(".")[0] in NAMES[:4]) else "fused"
    assert plan["layers"] == layers, (plan["layers"], layers)
    return layers


def _assert_launches(plan, kinds, what):
    n = {k: sum(1 for v in plan["layers"].values() if v == k) for k in ("fused", "two-pass", "plain+head")}
    passes = 1 if plan.get("twin", True) else 2
    assert kinds.get("conv3x3_pre16_act_kernel", 0) == passes * n["fused"] > 0, (what, kinds, plan)
    assert kinds.get("conv3x3_split_pre_kernel", 0) == passes * (n["two-pass"] + n["plain+head"]), (what, kinds, plan)
    assert kinds.get("convt_slot_fwd_kernel", 0) == passes * sum(1 for v in plan["convt"].values() if v == "slots"), (what, kinds, plan)
    assert "conv3x3_split_pre_act_kernel" not in kinds, (what, kinds)


_RUNS = {}


def _recipe(dev, which):
    """The HIP run of a recipe with its trace, and the fp64 oracle WITHOUT rounding: computed once, shared, never modified.
    A: 2 x 1 x 128^2, shared (twin batch of 4), conv = "bf16".  B: 1 x 3 x 128^2, unshared, bias 0.1, conv = "bf16".
    C: 2 x 1 x 256^2, shared, conv = "auto" (the fill rule decides the depth)."""
    from onet_amd import ops
    if which in _RUNS:
        return _RUNS[which]
    if which == "A":
        B, C, H, share, bias, st = 2, 1, 128, True, 0.0, ops.Settings(conv="bf16", fused_eval="bf16")
        X = orc.det_input(B, C, H, H, seed=201)
    elif which == "B":
        B, C, H, share, bias, st = 1, 3, 128, False, 0.1, ops.Settings(conv="bf16", fused_eval="bf16")
        X = orc.det_input(B, C, H, H, seed=202)
    else:
        B, C, H, share, bias, st = 2, 1, 256, True, 0.0, ops.Settings(fused_eval="bf16")
        X = orc.det_input(B, C, H, H, seed=201)
    top = _calibrated(orc.det_state_dict(C, 1981), X, bias)
    dwn = None if share else _calibrated(orc.det_state_dict(C, 1982), X, bias)
    m = _onet(_prefixed(top, dwn), C, share, dev)
    m.bias = bias
    m.settings = st
    import onet_amd
    Xg = X.to(dev)
    plan = onet_amd.fused_eval_plan(m, Xg.shape)
    out, kinds, trace, convt = _traced_run(m, Xg)
    replay, on_slots = _replay_lists(trace, convt, B, plan.get("twin", False))
    _RUNS[which] = dict(B=B, X=X, Xg=Xg, top=top, dwn=dwn, bias=bias, m=m, plan=plan, out=out, kinds=kinds, replay=replay,
                        on_slots=on_slots, exact=_oracle(X, top, dwn, bias))
    return _RUNS[which]


def _check_replayed_run(r, what):
    """M1's comparison: the oracle on the run's own rounded operands (every slot tensor within one bf16 ulp of the oracle's value: its
    _check_replayed), all five outputs within TOL, labels equal on the margin pixels, those more than 0.9 of all."""
    ref = _oracle(r["X"], r["top"], r["dwn"], r["bias"], _rule_of(r["replay"]), r["replay"])
    errs = {n: _rel(a, b) for a, b, n in zip(r["out"], ref, ("Lt", "Vt", "Ld", "Vd", "S"))}
    print(f"{what}: " + ", ".join(f"{n} {e:.2e}" for n, e in errs.items()))
    for a, b, n in zip(r["out"], ref, ("Lt", "Vt", "Ld", "Vd", "S")):
        assert torch.isfinite(a).all(), (what, n)
        assert a.dtype == torch.float32 and a.is_cuda and a.grad_fn is None and tuple(a.shape) == tuple(b.shape), (what, n)
        assert errs[n] <= TOL, f"{what} {n}: max err {errs[n]:.3e} of the tensor's largest magnitude (tol {TOL})"
    sure = _margin(ref)
    share = float(sure.double().mean())
    print(f"{what}: margin pixels {share:.4f}")
    assert share > 0.9, (what, share)
    assert torch.equal(r["m"].predict_label(r["out"][4]).cpu().long()[sure], orc.predict_label(ref[4]).long()[sure]), what
    return ref


def test_m1_recipe_a_replayed(dev):
    """M1, recipe A: depth 3 under conv = "bf16"; the ConvTranspose2d of levels 0 and 1 (inference.py's up4, up3) on slot operands, level
    2's (up2) from the fp32 tensor of the fall-back level, up1 in the fall-back part; launch records == the announcement; the oracle
    with the run's roundings replayed.  (The names are inference._level_layers': `up4` is the Up block of level 0, the LAST one the
    forward applies, `up1` the deepest.  The issue's wording -- "up2 and up1 as slots, up3 as fp32->slots" -- counts the other way
    round; the expected kinds are derived from the code's names, level by level.)  Also: a second call is bit-equal, the BatchNorm buffers are untouched, segment() ==
    predict_label(S).
    The replay covers every layer the run evaluated on rounded operands: the convolutions and ConvTranspose2d layers on slots (from
    inference.TRACE) and, under conv = "bf16", the ConvTranspose2d GEMMs that read an fp32 tensor and round it on load
    (convt_operand_bf16 = 1: up2; up1 in the fall-back part reads an 8 x 8 map, which the GEMM does not take: the direct fp32 kernel
    runs there, unrounded) -- their inputs are taken where the wrappers are called.
    Measured on an MI355X: Lt 3.0e-7, Vt 1.9e-7, Ld 2.7e-7, Vd 2.0e-7, S 1.7e-6 (bound 2e-4); margin pixels 0.9932."""
    import onet_amd
    r = _recipe(dev, "A")
    plan, m = r["plan"], r["m"]
    assert plan["fused"] and plan["depth"] == 3 and plan["operands"] == "bf16" and plan["twin"] and plan["batch"] == 4, plan
    layers = _expected_plan(m, plan, 3)
    assert plan["convt"] == {UNAMES[0]: "slots", UNAMES[1]: "slots", UNAMES[2]: "fp32->slots", UNAMES[3]: "fallback"}, plan
    _assert_launches(plan, r["kinds"], "M1 A")
    assert r["on_slots"] == {n for n, v in layers.items() if v in ("fused", "two-pass", "plain+head")}, r["on_slots"]
    buf0 = {k: v.clone() for k, v in m.state_dict().items() if "running" in k or "num_batches" in k}
    _check_replayed_run(r, "M1 A")
    with torch.no_grad():
        out2 = m(r["Xg"])
    assert all(torch.equal(a, b) for a, b in zip(r["out"], out2))
    for k, v in m.state_dict().items():
        if k in buf0:
            assert torch.equal(v, buf0[k]), k
    lab = onet_amd.segment(m, r["Xg"])
    assert lab.dtype == torch.int64 and tuple(lab.shape) == (r["B"], 128, 128)
    assert torch.equal(lab, m.predict_label(r["out"][4]))


def test_m1_recipe_b_unshared_rgb(dev):
    """M1, recipe B: the unshared two-pass form (two U-Nets, B = 1 each, bias 0.1) and the RGB stem.
    Measured on an MI355X: Lt 3.4e-7, Vt 1.7e-7, Ld 2.8e-7, Vd 2.4e-7, S 1.2e-6 (bound 2e-4); margin pixels 0.9935."""
    r = _recipe(dev, "B")
    plan = r["plan"]
    assert plan["fused"] and plan["depth"] == 3 and plan["operands"] == "bf16" and not plan["twin"] and plan["batch"] == 1, plan
    _expected_plan(r["m"], plan, 3)
    _assert_launches(plan, r["kinds"], "M1 B")
    _check_replayed_run(r, "M1 B")


def _free_rounding_check(r, what):
    """M2's comparison.  e_ref: how far the oracle under FREE rounding of the same layers lies from the unrounded oracle, per output, of
    the output's largest magnitude.  The HIP run is another free rounding sequence of the same function, so it must lie within 2 e_ref
    (two independent chaotic sequences one e_ref from the truth each; the maximum over pixels is an extreme-value statistic; a wrong
    channel, pixel or coefficient gives O(1)); its labels differ from the unrounded oracle's on at most twice the share of pixels the
    rounded oracle's do."""
    exact = r["exact"]
    free = _oracle(r["X"], r["top"], r["dwn"], r["bias"], _rule_of(r["replay"]))
    lab0 = orc.predict_label(exact[4]).long()
    flips_ref = float((orc.predict_label(free[4]).long() != lab0).double().mean())
    flips = float((r["m"].predict_label(r["out"][4]).cpu().long() != lab0).double().mean())
    rows = []
    for i, n in ((0, "Lt"), (1, "Vt"), (2, "Ld"), (3, "Vd")):
        rows.append((n, _rel(r["out"][i], exact[i]), _rel(free[i], exact[i])))
    print(f"{what}: " + ", ".join(f"{n} {e:.2e} (e_ref {er:.2e})" for n, e, er in rows) +
          f"; labels differing {100 * flips:.2f} % (rounded oracle {100 * flips_ref:.2f} %)")
    for n, e, er in rows:
        assert er > 0 and e <= 2 * er, f"{what} {n}: {e:.3e} from the unrounded oracle, the rounded oracle {er:.3e}"
    assert flips <= 2 * flips_ref, (what, flips, flips_ref)


def test_m2_recipe_a_free_rounding(dev):
    """M2: recipe A against the UNROUNDED oracle, bounded by twice the rounded oracle's own deviation.
    Measured on an MI355X (e_ref computed in the test, on the host): Lt 3.21e-3 (e_ref 3.21e-3), Vt 3.25e-2 (3.35e-2), Ld 3.19e-3
    (3.19e-3), Vd 2.71e-2 (2.75e-2); labels differing from the unrounded oracle's 1.32 % (rounded oracle 1.29 %)."""
    _free_rounding_check(_recipe(dev, "A"), "M2 A")


def test_m3_other_settings_keep_their_paths(dev):
    """M3: Settings() and Settings(fused_eval=True) launch the kinds recorded on the commit before the one-part plan existed
    (tests/test_gpu_fused_eval.py: F7's counts; F1's depth-2 announcement) and no one-part kernel; conv = "bf16" with fused_eval=True
    still falls back to the default path (no fused launch of either kind, outputs equal to Settings(conv="bf16"))."""
    import onet_amd
    from onet_amd import ops
    m = _onet(_prefixed(orc.det_state_dict(1, 1981)), 1, True, dev)
    X = orc.det_input(2, 1, 256, 256, seed=113).to(dev)
    a, ka = _eval(m, X, ops.Settings())
    assert ka == {"conv_fwd_kernel": 11, "conv3x3_split_kernel": 7, "convt_gemm_kernel": 4}, ka
    b, kb = _eval(m, X, ops.Settings(fused_eval=False))
    assert ka == kb and all(torch.equal(x, y) for x, y in zip(a, b))
    f, kf = _eval(m, X, ops.Settings(fused_eval=True))
    plan = onet_amd.fused_eval_plan(m, X.shape)
    assert plan["fused"] and plan["depth"] == 2 and plan["operands"] == "fp16x2", plan
    n = {k: sum(1 for v in plan["layers"].values() if v == k) for k in ("fused", "two-pass", "plain+head")}
    assert kf.get("conv3x3_split_pre_act_kernel", 0) == n["fused"] > 0 and "conv3x3_pre16_act_kernel" not in kf, (kf, plan)
    assert kf.get("conv3x3_split_pre_kernel", 0) == n["two-pass"] + n["plain+head"], (kf, plan)
    assert kf.get("convt_slot_fwd_kernel", 0) == sum(1 for v in plan["convt"].values() if v == "slots") > 0, (kf, plan)
    assert "conv3x3_split_kernel" not in kf, kf
    f2, _ = _eval(m, X)
    assert all(torch.equal(x, y) for x, y in zip(f, f2))
    c, kc = _eval(m, X, ops.Settings(conv="bf16"))
    d, kd = _eval(m, X, ops.Settings(conv="bf16", fused_eval=True))
    assert kc == kd and all(torch.equal(x, y) for x, y in zip(c, d)), (kc, kd)
    assert not {"conv3x3_pre16_act_kernel", "conv3x3_split_pre_act_kernel", "convt_slot_fwd_kernel"} & set(kd), kd
    m.settings = ops.Settings(conv="bf16", fused_eval=True)
    p = onet_amd.fused_eval_plan(m, X.shape)
    assert not p["fused"] and p["operands"] == "fp16x2" and "fp16-split" in p["reason"], p


def test_m3_auto_dispatch_fuses_to_the_fill_rule(dev):
    """M3: Settings(fused_eval="bf16") under conv = "auto" at 2 x 1 x 256^2 (twin batch of 4): the 256- and 128-pixel levels have the 192
    tiles the fill rule asks on 256 compute units (512 and 256), the 64-pixel level has 128 -- depth 2, everything below on the existing
    eval kernels.  The outputs then pass M2's bounds with the rule restricted to the layers that ran on slots.
    Measured on an MI355X: Lt 3.96e-3 (e_ref 3.96e-3), Vt 2.94e-2 (2.80e-2), Ld 3.83e-3 (3.83e-3), Vd 2.51e-2 (2.59e-2); labels
    differing 1.28 % (rounded oracle 1.31 %).  (The three fp64 evaluations at 256 x 256 on the host are this test's 16 s.)"""
    r = _recipe(dev, "C")
    plan = r["plan"]
    assert plan["fused"] and plan["depth"] == 2 and plan["operands"] == "bf16" and plan["twin"], plan
    layers = _expected_plan(r["m"], plan, 2)
    assert all(v == "fallback" for n, v in layers.items() if n.split(".")[0] in ("down2", "down3", "down4", "up2", "up1"))
    assert plan["convt"] == {UNAMES[0]: "slots", UNAMES[1]: "fp32->slots", UNAMES[2]: "fallback", UNAMES[3]: "fallback"}, plan
    _assert_launches(plan, r["kinds"], "M3 auto")
    assert r["on_slots"] == {n for n, v in layers.items() if v in ("fused", "two-pass", "plain+head")}, r["on_slots"]
    assert all(x is None for x, _ in r["replay"]["convT2x2"][:3]) and r["replay"]["convT2x2"][3][0] is not None      # only up4 reads slots
    _free_rounding_check(r, "M3 auto")
