"""The unit in front of a max-pool as ONE launch (Settings.fused_eval = "fp16x2+pool" | "bf16+pool"; onet_amd/inference.py).

Kernel level (K1 - K3): onet_conv3x3_plain16_fwd_pre_act_pool / onet_conv3x3_split_fwd_pre_act_pool -- the _act entries' convolution
with BatchNorm(eval) + ReLU and the 2 x 2 max-pooling in the epilogue -- against the two-pass form built from existing entry points (the
plain launch with an fp32 z, then onet_bn_relu_apply_pool_split with the same coefficients and scale slots): bit identity, torch.equal
on the 16-bit words of the skip and pooled slots, the pooled fp32 tensor, the fp32 activation and the recorded maximum; and the pooled
fp32 tensor against fp64.

Model level (M1 - M3): the plan with "+pool" against the same plan without it -- the claim is that nothing but the number of launches
changes, so every output, every traced tensor and the labels-only calls are compared with torch.equal, and the launch records with the
plan's announcement."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import onet_oracle as orc

pytestmark = pytest.mark.gpu

TOL = 2e-4          # fp16 parts: of the tensor's largest magnitude (tests/test_gpu_fused_eval.py's bound on every eval output)
TOL_A = 2e-6        # one part: plain bf16 forward against fp64 of the ROUNDED operands, of the term scale (tests/test_gpu_fused_eval_bf16.py)
FORMATS = ("bf16", "fp16x2")


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


def _bits(P):
    return P.contiguous().view(torch.int16)


# ----------------------------------------------------------------------------------------------------------------- kernel level
K_SHAPES = [(2, 64, 64, 16, 32),          # one tile per image
            (2, 96, 64, 48, 96),          # 3 x 3 tiles: halos on every side, an odd chunk count
            (1, 512, 128, 32, 64),        # 16 chunks, two channel tiles
            (3, 32, 192, 128, 128)]       # 288 tiles: more than one per persistent block (the coefficient double buffer)
K_IDS = ["one-tile", "3x3-tiles", "16-chunks", "288-tiles"]
_K_IN, _K_CACHE = {}, {}


def _k_inputs(shape):
    """x, w (both bf16-exact, so that either format packs them without loss and one fp64 reference serves both), the BatchNorm
    parameters and the fp64 pooled activation of a shape: computed once, shared, never modified"""
    if shape not in _K_IN:
        B, Cin, Cout, H, W = shape
        x = rnd(B, Cin, H, W, seed=400).to(torch.bfloat16).float()
        w = rnd(Cout, Cin, 3, 3, seed=401, scale=(2.0 / (Cin * 9)) ** 0.5).to(torch.bfloat16).float()
        gamma = (rnd(Cout, seed=402).abs() + 0.5) * torch.where(rnd(Cout, seed=403) > 0.5, -1.0, 1.0)     # (mixed-sign sc)
        bn = (gamma, rnd(Cout, seed=404, scale=0.3), rnd(Cout, seed=405, scale=0.1), rnd(Cout, seed=406) ** 2 + 0.5)
        _K_IN[shape] = dict(x=x, w=w, bn=bn)
    return _K_IN[shape]


def _fp64(shape, save):
    """-> (max_pool2d(relu(bn(conv64))), per-channel term scale |sc| (max |z64| + |mean|) + |sh|) from the packed operands"""
    c = _k_inputs(shape)
    if "y64" not in c:
        s = save.detach().cpu().double()
        z64 = F.conv2d(c["x"].double(), c["w"].double(), None, 1, 1)
        mean, sc, sh = (s[k].view(1, -1, 1, 1) for k in (0, 2, 3))
        c["y64"] = F.max_pool2d(torch.relu((z64 - mean) * sc + sh), 2)
        c["term"] = sc.abs() * (z64.abs().amax((0, 2, 3), keepdim=True) + mean.abs()) + sh.abs()
    return c["y64"], c["term"]


def _operands(dev, fmt, shape):
    from onet_amd import ops
    c = _k_inputs(shape)
    xg, wg = c["x"].to(dev), c["w"].to(dev)
    save = ops.bn_eval_coeffs(*(t.to(dev) for t in c["bn"]), 1e-5)
    if fmt == "bf16":
        return dict(P=ops.split_pack_act(xg, parts=1), wq=ops.pack3x3_plain16(wg)[0], save=save, scale=None, xkw={}, parts=1,
                    dtype=torch.bfloat16)
    xs = ops.absmax_slots(xg)
    with ops.using(ops.Settings(conv="auto", split_f16=True)):
        wq = ops.pack3x3_split(wg)[0]
    assert wq.dtype == torch.float16
    return dict(P=ops.split_pack_act(xg, f16=True, slots=xs), wq=wq, save=save, scale=ops.conv3x3_act_bound(wg, save, xs),
                xkw=dict(slots=xs), parts=2, dtype=torch.float16)


def _fused(fmt, o, Cout, **kw):
    """the fused launch of either format on the operands `o`"""
    from onet_amd import ops
    if fmt == "bf16":
        return ops.conv3x3_plain16_pre_act_pool(o["P"], o["wq"], Cout, o["save"], **kw)
    return ops.conv3x3_split_pre_act_pool(o["P"], o["wq"], Cout, o["save"], o["scale"], **o["xkw"], **kw)


def _nan_slots(o, B, C, H, W, dev):
    return torch.full((B, C // 8, H, o["parts"], W, 8), float("nan"), dtype=o["dtype"], device=dev)


def _k_case(dev, fmt, shape):
    """operands, the two-pass form and the fused launch (every output) of one format and shape, computed once for K1 - K3"""
    from onet_amd import ops
    if (fmt, shape) in _K_CACHE:
        return _K_CACHE[fmt, shape]
    B, Cin, Cout, H, W = shape
    o = _operands(dev, fmt, shape)
    nan = lambda *s: torch.full(s, float("nan"), device=dev)
    z = ops.conv3x3_split_pre(o["P"], o["wq"], Cout, out=nan(B, Cout, H, W), **o["xkw"])
    assert z.dtype == torch.float32
    ref = dict(skip=_nan_slots(o, B, Cout, H, W, dev), a=nan(B, Cout, H, W), yP=_nan_slots(o, B, Cout, H // 2, W // 2, dev),
               y=nan(B, Cout, H // 2, W // 2))
    assert ops.bn_relu_apply_pool_split(z, o["save"], ref["skip"], ref["a"], ref["yP"], ref["y"], slots=o["scale"])
    got = {k: torch.full_like(v, float("nan")) for k, v in ref.items()}
    am = torch.zeros(ops.AMAX_SLOTS, dtype=torch.int32, device=dev)
    ops.profile_start(everything=False)
    try:
        ret = _fused(fmt, o, Cout, out=got["skip"], a_amax=am, a=got["a"], yP=got["yP"], y=got["y"])
        torch.cuda.synchronize()
    finally:
        kinds = {k: len(v) for k, v in ops.profile_stop()[0].items()}
    assert ret is got["skip"]
    assert kinds == {"conv3x3_pre16_act_pool_kernel" if fmt == "bf16" else "conv3x3_split_pre_act_pool_kernel": 1}, kinds
    _K_CACHE[fmt, shape] = dict(o=o, ref=ref, got=got, am=am)
    return _K_CACHE[fmt, shape]


def _same(got, ref, what):
    for k in ("skip", "yP"):
        if got.get(k) is not None:
            assert torch.equal(_bits(got[k]), _bits(ref[k])), f"{what}: {k} slots differ from the two-pass form"
    for k in ("a", "y"):
        if got.get(k) is not None:
            assert torch.equal(got[k].contiguous(), ref[k]), f"{what}: fp32 {k} differs from the two-pass form"


@pytest.mark.parametrize("shape", K_SHAPES, ids=K_IDS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_k1_pooled_epilogue_bit_identical(dev, fmt, shape):
    """K1: one launch of the new kind == plain launch (fp32 z) + bn_relu_apply_pool_split on the skip slots, the pooled slots, the
    pooled fp32 tensor and the fp32 activation; recorded maximum == max a; with the pooled slots alone and with the pooled fp32 tensor
    alone the same bits."""
    c = _k_case(dev, fmt, shape)
    B, Cin, Cout, H, W = shape
    ref, got, o = c["ref"], c["got"], c["o"]
    for k, v in ref.items():
        assert torch.isfinite(v.float()).all(), (fmt, shape, k)
    cut = float((ref["a"] == 0).double().mean())
    assert 0.3 < cut < 0.7, cut                                     # ReLU cuts about half: the comparison is not vacuous
    assert bool((ref["y"] > 0).any()) and bool((ref["y"] == 0).any())
    _same(got, ref, f"{fmt} {shape}")
    assert _slot_max(c["am"]) == float(ref["a"].max()), (fmt, shape, _slot_max(c["am"]), float(ref["a"].max()))
    only_P = dict(skip=_nan_slots(o, B, Cout, H, W, dev), yP=_nan_slots(o, B, Cout, H // 2, W // 2, dev))
    assert _fused(fmt, o, Cout, out=only_P["skip"], yP=only_P["yP"]) is only_P["skip"]
    only_y = dict(skip=_nan_slots(o, B, Cout, H, W, dev), y=torch.full_like(ref["y"], float("nan")))
    assert _fused(fmt, o, Cout, out=only_y["skip"], y=only_y["y"]) is only_y["skip"]
    torch.cuda.synchronize()
    _same(only_P, ref, f"{fmt} {shape}, pooled slots only")
    _same(only_y, ref, f"{fmt} {shape}, pooled fp32 only")


@pytest.mark.parametrize("fmt", FORMATS)
def test_k2_strided_destinations(dev, fmt):
    """K2: skip slots into the leading channel groups of a wider concat buffer, a / pooled slots / pooled fp32 into batch-strided views:
    the same bits as the dense launch, the other groups and the gaps keep their fill value."""
    shape = K_SHAPES[1]
    c = _k_case(dev, fmt, shape)
    B, Cin, Cout, H, W = shape
    o, ref = c["o"], c["ref"]
    cat = torch.full((B, (Cout + 64) // 8, H, o["parts"], W, 8), 7.0, dtype=o["dtype"], device=dev)
    wide_a = torch.full((B, Cout + 8, H, W), 7.0, device=dev)
    wide_P = torch.full((B, (Cout + 16) // 8, H // 2, o["parts"], W // 2, 8), 7.0, dtype=o["dtype"], device=dev)
    wide_y = torch.full((B, Cout + 4, H // 2, W // 2), 7.0, device=dev)
    got = dict(skip=cat[:, :Cout // 8], a=wide_a[:, :Cout], yP=wide_P[:, :Cout // 8], y=wide_y[:, :Cout])
    assert _fused(fmt, o, Cout, out=got["skip"], a=got["a"], yP=got["yP"], y=got["y"]) is got["skip"]
    torch.cuda.synchronize()
    _same(got, ref, f"{fmt} strided")
    assert bool((cat[:, Cout // 8:] == 7.0).all()) and bool((wide_a[:, Cout:] == 7.0).all())
    assert bool((wide_P[:, Cout // 8:] == 7.0).all()) and bool((wide_y[:, Cout:] == 7.0).all())


@pytest.mark.parametrize("shape", K_SHAPES, ids=K_IDS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_k3_pooled_fp32_against_fp64(dev, fmt, shape):
    """K3: the pooled fp32 output against max_pool2d(relu(bn(conv64))) of the packed operands (x and w are bf16-exact: both packs hold
    them without loss).  Max-pooling is 1-Lipschitz, so the activation's bounds carry over: one part -- every element within TOL_A of
    its channel's term scale |sc| (max |z64| + |mean|) + |sh| (tests/test_gpu_fused_eval_bf16.py's K2); fp16 parts -- the largest
    error within TOL of the tensor's largest magnitude (tests/test_gpu_fused_eval.py's bound on an eval output).
    Measured on an MI355X, K_SHAPES' order: one part, worst element 0.21 / 0.26 / 0.51 / 0.15 of its bound; fp16 parts, 2.8e-7 / 4.5e-7 /
    8.7e-7 / 2.1e-7 of the largest magnitude."""
    c = _k_case(dev, fmt, shape)
    y64, term = _fp64(shape, c["o"]["save"])
    err = (c["got"]["y"].detach().cpu().double() - y64).abs()
    worst_term, worst_rel = float((err / (TOL_A * term)).max()), float(err.max()) / float(y64.abs().max())
    print(f"K3 {fmt} {shape}: worst {worst_term:.3f} of the one-part bound, {worst_rel:.2e} of the largest magnitude")
    if fmt == "bf16":
        assert bool((err <= TOL_A * term).all()), f"{shape}: {worst_term:.3f} x the bound"
    else:
        assert worst_rel <= TOL, f"{shape}: {worst_rel:.3e} of the largest magnitude (tol {TOL})"


@pytest.mark.parametrize("fmt", FORMATS)
def test_k4_wrapper_refuses_outside_the_domain_and_without_a_pooled_destination(dev, fmt):
    """outside the _act entries' domain the wrapper returns None and nothing is written; without yP and y it raises"""
    shape = K_SHAPES[0]
    B, Cin, Cout, H, W = shape
    o = _k_case(dev, fmt, shape)["o"]
    with pytest.raises(ValueError, match="pooled"):
        _fused(fmt, o, Cout)
    skip = torch.full((B, 96 // 8, H, o["parts"], W, 8), 7.0, dtype=o["dtype"], device=dev)
    y = torch.full((B, 96, H // 2, W // 2), 7.0, device=dev)
    assert _fused(fmt, o, 96, out=skip, y=y) is None                # Cout = 96
    torch.cuda.synchronize()
    assert bool((skip == 7.0).all()) and bool((y == 7.0).all())


# ----------------------------------------------------------------------------------------------------------------- model level
def _prefixed(top, dwn=None):
    sd = {"topu." + k: v for k, v in top.items()}
    sd.update({"dwnu." + k: v for k, v in (top if dwn is None else dwn).items()})
    return sd


def _onet(sd, C, bshare, dev):
    import Onet_vanilla_20240606 as ov
    m = ov.Onet(in_chns=C, binit=True, bshare=bshare)
    m.load_state_dict(sd)
    return m.to(dev).eval()


def _settings(fmt, pool):
    from onet_amd import ops
    if fmt == "bf16":
        return ops.Settings(conv="bf16", fused_eval="bf16+pool" if pool else "bf16")
    return ops.Settings(conv="split", fused_eval="fp16x2+pool" if pool else True)


POOL_KIND = {"bf16": "conv3x3_pre16_act_pool_kernel", "fp16x2": "conv3x3_split_pre_act_pool_kernel"}
ACT_KIND = {"bf16": "conv3x3_pre16_act_kernel", "fp16x2": "conv3x3_split_pre_act_kernel"}
HEAD_KIND = {"bf16": "conv3x3_pre16_head_kernel", "fp16x2": "conv3x3_split_pre_head_kernel"}


def _run(m, Xg, fmt, pool):
    """One traced and profiled forward, then scores and segment(head="fused"), under the plan with or without "+pool" -> outputs, the
    trace, {kind: launches} of the forward, the plan, and the names of the units whose skip slots a pooled launch wrote (each call of
    the pooled wrapper is matched to the traced tensor that starts at its `out`)."""
    import onet_amd
    from onet_amd import inference, ops
    m.settings = _settings(fmt, pool)
    name = "conv3x3_plain16_pre_act_pool" if fmt == "bf16" else "conv3x3_split_pre_act_pool"
    real, outs = getattr(ops, name), []

    def watched(*a, **kw):
        outs.append(kw["out"].data_ptr())
        return real(*a, **kw)

    setattr(ops, name, watched)
    inference.TRACE = []
    ops.profile_start(everything=False)
    try:
        with torch.no_grad():
            out = m(Xg)
        torch.cuda.synchronize()
        trace = inference.TRACE
    finally:
        kinds = {k: len(v) for k, v in ops.profile_stop()[0].items()}
        inference.TRACE = None
        setattr(ops, name, real)
    by_ptr = {t.P.data_ptr(): n for n, t in trace if not n.endswith((".up", ".pool"))}
    return dict(out=out, trace=trace, kinds=kinds, plan=onet_amd.fused_eval_plan(m, Xg.shape), pooled_by=[by_ptr[p] for p in outs],
                scores=onet_amd.scores(m, Xg), labels=onet_amd.segment(m, Xg, head="fused"))


M_CASES = {"bf16-depth5": ("bf16", (2, 1, 256, 512), True, 0.0, 5), "fp16-depth5": ("fp16x2", (2, 1, 256, 512), True, 0.0, 5),
           "bf16-depth3": ("bf16", (2, 1, 128, 128), True, 0.0, 3), "fp16-depth3": ("fp16x2", (2, 1, 128, 128), True, 0.0, 3),
           "bf16-unshared-rgb": ("bf16", (1, 3, 128, 128), False, 0.1, 3), "fp16-unshared-rgb": ("fp16x2", (1, 3, 128, 128), False, 0.1, 3)}
_M_RUNS = {}


def _m_case(dev, case):
    """both runs of a case (the plan without and with "+pool" on one model and input): computed once for M1 - M3, never modified"""
    if case not in _M_RUNS:
        fmt, shape, share, bias, depth = M_CASES[case]
        C = shape[1]
        top = orc.det_state_dict(C, 1981)
        m = _onet(_prefixed(top, None if share else orc.det_state_dict(C, 1982)), C, share, dev)
        m.bias = bias
        Xg = orc.det_input(*shape, seed=141).to(dev)
        _M_RUNS[case] = dict(fmt=fmt, depth=depth, passes=1 if share else 2, base=_run(m, Xg, fmt, False), pool=_run(m, Xg, fmt, True))
    return _M_RUNS[case]


def _eq(a, b):
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, tuple):
        return len(a) == len(b) and all(_eq(x, y) for x, y in zip(a, b))
    if not torch.is_tensor(a):
        return a == b
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int16 if a.element_size() == 2 else a.dtype),
                                                                     b.contiguous().view(torch.int16 if b.element_size() == 2 else b.dtype))


@pytest.mark.parametrize("case", list(M_CASES))
def test_m1_plan_with_pool_is_bit_identical(dev, case):
    """M1: the five forward outputs, scores, segment(head="fused") and every tensor of inference.TRACE (name, order, slots, fp32 tensor,
    both sets of magnitude slots) are equal with and without "+pool".  depth 5: all four pooled units leave slots; depth 3: the pooled
    tensor of level 2 leaves as fp32 into the fall-back levels; unshared: two passes."""
    r = _m_case(dev, case)
    base, pool = r["base"], r["pool"]
    for p in (base["plan"], pool["plan"]):
        assert p["fused"] and p["depth"] == r["depth"] and p["twin"] == (r["passes"] == 1), p
    for a, b, n in zip(pool["out"], base["out"], ("Lt", "Vt", "Ld", "Vd", "S")):
        assert torch.isfinite(b).all() and float(b.abs().max()) > 0, (case, n)
        assert torch.equal(a, b), f"{case}: {n} differs"
    assert float(base["out"][4].std()) > 0, case                   # (S is not a constant map: the run is not degenerate)
    for a, b, n in zip(pool["scores"], base["scores"], ("Vt", "Vd", "S")):
        assert torch.equal(a, b), f"{case}: scores {n} differs"
    assert torch.equal(pool["labels"], base["labels"]) and base["labels"].dtype == torch.int64, case
    assert [n for n, _ in pool["trace"]] == [n for n, _ in base["trace"]] and len(base["trace"]) > 0, case
    for (n, a), (_, b) in zip(pool["trace"], base["trace"]):
        assert a.P is not None and bool((a.P != 0).any()), (case, n)
        for f in ("P", "F", "scale", "amax"):
            assert _eq(getattr(a, f), getattr(b, f)), f"{case}: traced {n}.{f} differs"


def _counts(plan):
    return {k: sum(1 for v in plan["layers"].values() if v == k) for k in ("fused", "two-pass", "fused+pool", "plain+head")}


@pytest.mark.parametrize("case", list(M_CASES))
def test_m2_launch_audit(dev, case):
    """M2: with "+pool" the new kind is launched passes x (number of "fused+pool" layers) times and conv3x3_split_pre_kernel that many
    times less; without it the kinds and counts are those tests/test_gpu_fused_eval.py and tests/test_gpu_fused_eval_bf16.py assert of
    a fused forward (their _assert_plan_matches / _assert_launches rule) and no new kind appears."""
    r = _m_case(dev, case)
    fmt, passes = r["fmt"], r["passes"]
    kb, kp = r["base"]["kinds"], r["pool"]["kinds"]
    nb, npl = _counts(r["base"]["plan"]), _counts(r["pool"]["plan"])
    assert nb["fused+pool"] == 0 and nb["two-pass"] == min(r["depth"], 4) and npl["two-pass"] == 0 and npl["fused+pool"] == nb["two-pass"]
    # without "+pool": what the parent commit launches
    assert kb.get(ACT_KIND[fmt], 0) == passes * nb["fused"] > 0, (case, kb)
    assert kb.get("conv3x3_split_pre_kernel", 0) == passes * (nb["two-pass"] + nb["plain+head"]), (case, kb)
    assert kb.get("convt_slot_fwd_kernel", 0) == passes * sum(1 for v in r["base"]["plan"]["convt"].values() if v == "slots"), (case, kb)
    assert not (set(POOL_KIND.values()) | set(HEAD_KIND.values()) | {ACT_KIND["bf16" if fmt == "fp16x2" else "fp16x2"]}) & set(kb), (case, kb)
    # with it
    assert kp.get(POOL_KIND[fmt], 0) == passes * npl["fused+pool"] > 0, (case, kp)
    assert kp.get("conv3x3_split_pre_kernel", 0) == kb["conv3x3_split_pre_kernel"] - passes * npl["fused+pool"] == passes, (case, kp, kb)
    assert {k: v for k, v in kp.items() if k not in (POOL_KIND[fmt], "conv3x3_split_pre_kernel")} == \
        {k: v for k, v in kb.items() if k != "conv3x3_split_pre_kernel"}, (case, kp, kb)


@pytest.mark.parametrize("case", list(M_CASES))
def test_m3_query_names_the_units_the_executor_fused(dev, case):
    """M3: fused_eval_plan on the GPU says "fused+pool" for exactly the units whose skip slots a pooled launch wrote (the names from
    M1's trace, the number from its profile), once per pass and in the encoder's order; without "+pool" the executor fuses none."""
    r = _m_case(dev, case)
    said = [n for n, v in r["pool"]["plan"]["layers"].items() if v == "fused+pool"]
    assert said == ["inc.c2", "down1.c2", "down2.c2", "down3.c2"][:min(r["depth"], 4)], said
    assert r["pool"]["pooled_by"] == said * r["passes"], (case, r["pool"]["pooled_by"], said)
    assert r["pool"]["kinds"][POOL_KIND[r["fmt"]]] == len(r["pool"]["pooled_by"])
    assert r["base"]["pooled_by"] == [] and "fused+pool" not in r["base"]["plan"]["layers"].values()
    assert r["pool"]["plan"]["operands"] == r["base"]["plan"]["operands"] == r["fmt"]
