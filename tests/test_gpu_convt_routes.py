"""The fused eval plan's ConvTranspose2d edges follow the plan record (inference._ROUTES, ops.CONVT_ENTRIES): every edge launches what
its route names and nothing else -- also where the switches keep the slot GEMM off and the record says "gemm" out of a fused level.

Onet(1, shared) at 2 x 1 x 64 x 64 (twin batch of 4), depth 2 on either slot format: the smallest input with both kinds of edge -- up4
reads the slots of the fused 32 x 32 level (h w = 1024: route "slots"), up3 the fp32 output of the fall-back 16 x 16 level (h w = 256:
route "gemm").  Values and bounds are those of tests/test_gpu_fused_eval_bf16.py (the oracle with the run's roundings replayed, TOL)
and tests/test_gpu_fused_eval.py (_compare, TOL); nothing new."""
import pytest
import torch

from oracle import onet_oracle as orc
import test_gpu_fused_eval as e32
import test_gpu_fused_eval_bf16 as e16
from test_gpu_fused_eval_bf16 import dev  # noqa: F401  (the module-scoped fixture)

pytestmark = pytest.mark.gpu

B, H = 2, 64
SETTINGS = {"bf16": dict(conv="bf16", fused_eval="bf16+pool"), "fp16x2": dict(conv="split", fused_eval=True)}
_MODEL = {}


def _model(dev):
    """the calibrated model, its input and the unrounded fp64 oracle: built once, shared, never modified"""
    if not _MODEL:
        X = orc.det_input(B, 1, H, H, seed=201)
        top = e16._calibrated(orc.det_state_dict(1, 1981), X)
        _MODEL.update(X=X, Xg=X.to(dev), top=top, m=e16._onet(e16._prefixed(top), 1, True, dev), exact=e32._oracle(X, top))
    return _MODEL


def _run(dev, fmt):
    """One forward under SETTINGS[fmt] with every call of inference._conv_t watched -> (r: the run as e16._check_replayed_run takes it,
    the plan record, [(route, {kind: launches recorded inside the call})] in execution order)"""
    import onet_amd
    from onet_amd import inference, ops
    c = _model(dev)
    m, Xg = c["m"], c["Xg"]
    m.settings = ops.Settings(**SETTINGS[fmt])
    plan = onet_amd.fused_eval_plan(m, Xg.shape)
    with ops.using(m.settings):
        record = inference._query(m.topu, (plan["batch"], 1, H, H), None, dev)
    edges, real = [], inference._conv_t

    def watched(f, lv, *args):
        before = {k: len(v) for k, v in ops.PROFILE.items()}
        out = real(f, lv, *args)
        edges.append((lv.route, {k: len(v) - before.get(k, 0) for k, v in ops.PROFILE.items() if len(v) != before.get(k, 0)}))
        return out
    inference._conv_t = watched
    try:
        if fmt == "bf16":
            out, kinds, trace, convt = e16._traced_run(m, Xg)
            replay, _ = e16._replay_lists(trace, convt, B, plan["twin"])
        else:
            (out, kinds), replay = e32._eval(m, Xg), None
    finally:
        inference._conv_t = real
    return dict(c, B=B, dwn=None, bias=0.0, out=out, kinds=kinds, replay=replay, plan=plan), record, edges


def _check_values(r, fmt, what):
    if fmt == "bf16":
        e16._check_replayed_run(r, what)
    else:
        print(f"{what} worst error {e32._compare(r['m'], r['out'], r['exact'], e32.TOL, what):.2e}")


@pytest.mark.parametrize("fmt", sorted(SETTINGS))
def test_edges_launch_what_their_routes_name(dev, fmt):
    """default switches: routes "slots" (up4) and "gemm" (up3); one convt_slot_fwd_kernel launch inside the slot edge, one
    convt_gemm_kernel inside the fp32 edge, and no other launch of the slot GEMM in the whole forward"""
    from onet_amd import inference, ops
    r, record, edges = _run(dev, fmt)
    assert record.reason is None and record.depth == 2 and r["plan"]["depth"] == 2 and r["plan"]["twin"], r["plan"]
    routes = [lv.route for lv in record.levels]
    assert routes == ["slots", "gemm", None, None, None] and [lv.convt for lv in record.levels[:2]] == ["slots", "fp32->slots"], routes
    assert not any(u.keep_fp32 for lv in record.levels for u in lv.enc + lv.dec)
    assert [e[0] for e in edges] == routes[1::-1], edges                      # (executed deepest first, one pass over the twin batch)
    for route, launched in edges:
        mode = inference._ROUTES[route].mode
        assert launched == ({"convt_gemm_kernel": 1} if mode is None else {"convt_slot_fwd_kernel": 1}), (route, launched)
        assert mode is None or ops.eval_convt_name(fmt, mode) == "convT2x2_fwd_slots"
    assert r["kinds"].get("convt_slot_fwd_kernel", 0) == routes.count("slots"), r["kinds"]
    _check_values(r, fmt, f"routes {fmt}")


@pytest.mark.parametrize("fmt", sorted(SETTINGS))
def test_switched_off_slot_gemm_follows_the_record(dev, fmt):
    """ops.CONVT_SLOTS = False: every edge of the fused levels is "gemm", up3.c2 keeps the fp32 copy up4 reads, the fp32-operand GEMM
    runs once per edge and the slot GEMM is never launched; the values stay inside the same bounds"""
    from onet_amd import ops
    real = ops.CONVT_SLOTS
    ops.CONVT_SLOTS = False
    try:
        r, record, edges = _run(dev, fmt)
    finally:
        ops.CONVT_SLOTS = real
    assert record.reason is None and record.depth == 2, record
    assert [lv.route for lv in record.levels] == ["gemm", "gemm", None, None, None]
    assert [lv.convt for lv in record.levels[:2]] == ["fp32->slots", "fp32->slots"]
    assert [u.name for lv in record.levels for u in lv.enc + lv.dec if u.keep_fp32] == ["up3.c2"]
    assert edges == [("gemm", {"convt_gemm_kernel": 1})] * 2, edges
    assert "convt_slot_fwd_kernel" not in r["kinds"], r["kinds"]
    _check_values(r, fmt, f"routes {fmt}, CONVT_SLOTS off")
