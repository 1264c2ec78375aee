"""The one-part fused eval plan with every ConvTranspose2d edge on slot operands, Settings(fused_eval="bf16+pool+anymap+pairs+up")
(onet_amd/inference.py): an edge whose input map has odd w, or whose output is padded into an odd concat map, runs
ops.convT2x2_fwd_slots_anymap (include/onet_hip_upmap.h) where "bf16+pool+anymap+pairs" takes the `pack` route.

U1 / U2 hold plans with both kinds of edge to the fp64 oracle with the run's own roundings replayed -- the method, the helpers and the
bounds of tests/test_gpu_pairs_eval.py (TOL = 2e-4 of each output's largest magnitude, labels equal on the margin pixels, those more than
0.9 of all; scores / segment(head="fused") / validate against the forward with 2.1 x 66 u |V|), nothing new.  What is this file's own:
the traced run also watches the new wrapper (_traced_run: a slot-route ConvTranspose2d hands its bf16 input to the replay, as the other
slot routes do; the padded output needs nothing -- the trace's up.* tensor is the concat map's groups either way), and the launch record
(_assert_routes: four launches of the slot GEMM per pass, no general ConvTranspose2d kernel, no conversion pass, no unit that keeps fp32).
U3: on an input without such an edge the new value launches what "bf16+pool+anymap+pairs" launches, the same bits.
U4: at U1's shape the two values both hold the replay bound and differ in bits: the route really changed.
The margin-pixel condition of the recipes' seeds was checked on the fp64 oracle alone before any GPU run (U1 = P1's recipe: 0.9934;
U2: see its docstring)."""
import pytest
import torch

from oracle import onet_oracle as orc
import test_gpu_fused_eval_bf16 as e16
import test_gpu_fused_head as fh
import test_gpu_pairs_eval as pe
from test_gpu_fused_eval_bf16 import dev  # noqa: F401  (the module-scoped fixture)

pytestmark = pytest.mark.gpu

VALUE = "bf16+pool+anymap+pairs+up"
PAIRS = "bf16+pool+anymap+pairs"
SLOTS4 = ("slots",) * 4
_RUNS = {}


def _traced_run(m, Xg):
    """tests/test_gpu_ragged_eval.py's _traced_run with the any-map slot-operand entry watched beside the four that function knows
    -> (outputs, {kind: launches}, {name: [slot tensor per pass]}, [per ConvTranspose2d call, in order: its bf16-rounded input as fp64 on
    the host, or None where the layer ran at fp32 level])"""
    from onet_amd import inference, ops
    convt = []
    names = ("convT2x2_fwd", "convT2x2_fwd_p", "convT2x2_fwd_slots", "convT2x2_fwd_slots_ragged", "convT2x2_fwd_slots_anymap")
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
    for n, f in zip(names, (fwd, fwd_p, on_slots(names[2]), on_slots(names[3]), on_slots(names[4]))):
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


def _run(dev, B, C, H, W, share, bias, seed, value=VALUE):
    """tests/test_gpu_pairs_eval.py's _run under `value`: model, plan, traced run and replay lists of one recipe under conv = "bf16";
    computed once per recipe and value, shared, never modified"""
    import onet_amd
    from onet_amd import ops
    key = (B, C, H, W, share, bias, seed, value)
    if key in _RUNS:
        return _RUNS[key]
    X = orc.det_input(B, C, H, W, seed=seed)
    top = e16._calibrated(orc.det_state_dict(C, 1981), X, bias)
    dwn = None if share else e16._calibrated(orc.det_state_dict(C, 1982), X, bias)
    m = e16._onet(e16._prefixed(top, dwn), C, share, dev)
    m.bias = bias
    m.settings = ops.Settings(conv="bf16", fused_eval=value)
    Xg = X.to(dev)
    plan = onet_amd.fused_eval_plan(m, Xg.shape)
    out, kinds, trace, convt = _traced_run(m, Xg)
    replay, on_slots = e16._replay_lists(trace, convt, B, plan.get("twin", False))
    _RUNS[key] = dict(B=B, X=X, Xg=Xg, top=top, dwn=dwn, bias=bias, m=m, plan=plan, out=out, kinds=kinds, replay=replay, on_slots=on_slots)
    return _RUNS[key]


def _assert_routes(r):
    """all four edges on the slot GEMM: 4 x passes launches of its kind, every one fed its bf16 slots (a replayed input each), no launch
    of the general ConvTranspose2d kind and no conversion pass inside a pass, no unit of the plan that keeps an fp32 copy"""
    import onet_amd
    from onet_amd import inference, ops
    m, Xg, plan = r["m"], r["Xg"], r["plan"]
    passes = 1 if plan["twin"] else 2
    assert tuple(plan["convt"][u] for u in pe.UNAMES) == SLOTS4, plan
    assert r["kinds"].get("convt_slot_fwd_kernel", 0) == 4 * passes and "convt_gemm_kernel" not in r["kinds"], r["kinds"]
    assert len(r["replay"]["convT2x2"]) == 8 and all(x_r is not None for x_r, _ in r["replay"]["convT2x2"])
    for call in (lambda: m(Xg), lambda: onet_amd.scores(m, Xg), lambda: onet_amd.segment(m, Xg, head="fused")):
        _, kinds, rest = fh._mfma_kinds(call)
        assert kinds.get("convt_slot_fwd_kernel", 0) == 4 * passes and "convt_gemm_kernel" not in kinds, kinds
        assert "onet_split_pack_act" not in rest and "onet_convT2x2_fwd" not in rest, rest
    with ops.using(m.settings):
        records, _ = inference._gate(m, tuple(Xg.shape))
    assert len(records) == passes
    for _, rec in records:
        assert rec.reason is None and rec.depth == 5
        assert not any(u.keep_fp32 for lv in rec.levels for u in lv.enc + lv.dec)
        assert [lv.route for lv in rec.levels[:4]][2:] == ["slots_anymap", "slots_anymap"], [lv.route for lv in rec.levels]


def test_u1_padded_edge_and_odd_w_edge_on_the_slot_gemm(dev):
    """U1: Onet(1, shared) at 1 x 1 x 48 x 200 (twin batch of 2), seed 301 -- P1's recipe: levels 48 x 200, 24 x 100, 12 x 50, 6 x 25 and
    3 x 12.  up1 reads the 3 x 12 map of the pair launch and pads its 6 x 24 block into 6 x 25 (the pad column); up2 reads the odd-w
    6 x 25 map; both by the any-map slot GEMM, and down4.c2 / up1.c2 write slots alone.  Margin pixels of the unrounded oracle: 0.9934
    (recorded with P1).
    Measured on an MI355X: Lt 3.9e-7, Vt 1.8e-7, Ld 3.8e-7, Vd 1.7e-7, S 1.3e-6 (bound 2e-4); margin pixels 0.9936; worst
    |V_scores - V_out| / bound Vt 0.042, Vd 0.036; label margin pixels 1.0000."""
    r = _run(dev, 1, 1, 48, 200, True, 0.0, 301)
    assert r["plan"]["twin"], r["plan"]
    _assert_routes(r)
    pe._check(r, SLOTS4, "U1 upmap 48x200")


def test_u2_unshared_rgb_both_pads_and_odd_w(dev):
    """U2: Onet(3, unshared), bias 0.1, at 1 x 3 x 40 x 200, seed 311: two passes of one image; levels 40 x 200, 20 x 100, 10 x 50, 5 x 25
    and 2 x 12.  up1 pads its 4 x 24 block BOTH ways into 5 x 25 (row, column and corner), up2 reads the odd-w 5 x 25 map.
    Margin pixels of the unrounded fp64 oracle, checked on the CPU before any GPU run: 0.9955 of all (seeds 312, 313: 0.9935, 0.9952).
    Measured on an MI355X: Lt 2.7e-7, Vt 2.1e-7, Ld 2.9e-7, Vd 1.9e-7, S 1.5e-6 (bound 2e-4); margin pixels 0.9951; worst
    |V_scores - V_out| / bound Vt 0.041, Vd 0.043; label margin pixels 1.0000."""
    r = _run(dev, 1, 3, 40, 200, False, 0.1, 311)
    assert not r["plan"]["twin"], r["plan"]
    _assert_routes(r)
    pe._check(r, SLOTS4, "U2 upmap 40x200")


def test_u3_without_such_an_edge_is_the_pairs_plan_bit_for_bit(dev):
    """U3: 1 x 1 x 128 x 256 (P3's shape: no pad, no odd w) under the new value: the same plan dictionary (`convt` included), the same
    launch records (MFMA kinds and every other entry point) and bit-identical five outputs, scores and segment(head="fused") as
    "bf16+pool+anymap+pairs" """
    import onet_amd
    from onet_amd import ops
    m = e16._onet(e16._prefixed(orc.det_state_dict(1, 1981)), 1, True, dev)
    Xg = orc.det_input(1, 1, 128, 256, seed=303).to(dev)
    got = {}
    m.settings = ops.Settings(conv="bf16", fused_eval=PAIRS)
    with torch.no_grad():
        m(Xg)                   # (the weight packs are made on first use: not part of either record)
    for value in (PAIRS, VALUE):
        m.settings = ops.Settings(conv="bf16", fused_eval=value)
        got[value] = (fh._mfma_kinds(lambda: m(Xg)), fh._mfma_kinds(lambda: onet_amd.scores(m, Xg)),
                      fh._mfma_kinds(lambda: onet_amd.segment(m, Xg, head="fused")), onet_amd.fused_eval_plan(m, Xg.shape))
    a, b = got[PAIRS], got[VALUE]
    assert a[3] == b[3] and b[3]["fused"] and b[3]["depth"] == 5 and b[3]["convt"] == dict(zip(pe.UNAMES, SLOTS4)), (a[3], b[3])
    for (oa, ka, ra), (ob, kb, rb), what in zip(a[:3], b[:3], ("forward", "scores", "segment")):
        oa, ob = (oa, ob) if isinstance(oa, tuple) else ((oa,), (ob,))
        assert len(oa) == len(ob) and all(torch.equal(x, y) for x, y in zip(oa, ob)), what
        assert ka == kb and ra == rb and ka.get("convt_slot_fwd_kernel", 0) == 4, (what, ka, kb, ra, rb)


def test_u4_the_route_really_changed(dev):
    """U4: at U1's shape the outputs under the new value and under "bf16+pool+anymap+pairs" both hold the replay bound and are NOT
    bit-equal: the two edges read bf16 slots where `pack` read the unrounded fp32 activation.  Guards against a silent fall-back.
    Measured on an MI355X: S 1.3e-6 under the new value, 1.2e-6 under "bf16+pool+anymap+pairs" (bound 2e-4); margin pixels 0.9936 / 0.9946."""
    new = _run(dev, 1, 1, 48, 200, True, 0.0, 301)
    old = _run(dev, 1, 1, 48, 200, True, 0.0, 301, value=PAIRS)
    assert tuple(old["plan"]["convt"][u] for u in pe.UNAMES) == ("slots", "slots", "fp32->slots", "fp32->slots"), old["plan"]
    assert old["kinds"].get("convt_slot_fwd_kernel", 0) == 2 and old["kinds"].get("convt_gemm_kernel", 0) == 2, old["kinds"]
    e16._check_replayed_run(new, "U4 new value")
    e16._check_replayed_run(old, "U4 pairs value")
    assert not all(torch.equal(a, b) for a, b in zip(new["out"], old["out"]))
    assert not torch.equal(new["out"][1], old["out"][1]), "Vt is bit-equal under both values: the route did not change"
