"""Labels-only inference: the head in the last convolution's epilogue (onet_amd.scores, onet_amd.segment(head="fused")).

Kernel level (K1 - K4): onet_conv3x3_plain16_fwd_pre_head / onet_conv3x3_split_fwd_pre_head -- conv3x3_pre16_kernel's HEAD instances,
V = sum_c L[c] relu(bn(z))[c] as the launch's only store -- against the two-launch form built from existing entry points (the plain
convolution, then bn_relu_apply) summed in fp64 on the host, with DERIVED bounds: u = 2^-24, a 64-term fp32 dot product in any order
is within 64 u (1 + O(u)) sum |terms| of the exact sum of its fp32 terms, 66 u leaves one rounding to spare.  onet_softmax2_labels
against the head kernel's own S and argmax2, bit for bit.

Model level (M1 - M4): scores() / segment(head="fused") against the forward of the same model and settings (one-part plan: the
activations are bit-equal, only the 64-term sum's order differs), against the fp64 oracle (fp16 plan), the launch records, the plan
report, and the fall-backs."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from multi_tile import multi_tile_cout
from oracle import onet_oracle as orc

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
DOT = 66 * U        # any-order rounding bound of a 64-term fp32 dot product, of sum |terms|, one rounding to spare
TOL = 2e-4          # eval outputs, of each tensor's largest magnitude (tests/test_gpu_fused_eval.py)
MARGIN = 1e-3       # labels compared where |Vt - Vd| exceeds this fraction of max |V| (fp64)
NEW_KINDS = {"conv3x3_pre16_head_kernel", "conv3x3_split_pre_head_kernel"}


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


def _save(Cout, seed, dev, gain=1.0):
    """[4][Cout] coefficients in bn_eval_coeffs' format (mean, invstd, sc = gamma invstd, sh = beta): about half of relu's inputs
    negative"""
    mean, sc, sh = rnd(Cout, seed=seed, scale=0.1), rnd(Cout, seed=seed + 1).abs() + 0.5, rnd(Cout, seed=seed + 2, scale=0.3)
    sc = sc * torch.where(rnd(Cout, seed=seed + 3) > 1.0, -1.0, 1.0)             # (a few negative BatchNorm weights)
    return torch.stack([mean, torch.ones(Cout), sc * gain, sh * gain]).contiguous().to(dev)


def unsplit(P):
    """pre-split slots [B][C/8][H][parts][W][8] -> fp64 [B][C][H][W] (the parts summed; still times the producer's power of two)"""
    B, C8, H, _, W, _ = P.shape
    v = P.detach().cpu().double().sum(3)
    return v.permute(0, 1, 4, 2, 3).reshape(B, C8 * 8, H, W)


def _mfma_kinds(fn):
    """-> (fn(), {kind: launches} of the MFMA kernels, {entry point: launches} of every other launch)"""
    from onet_amd import ops
    ops.profile_start(everything=True)
    try:
        with torch.no_grad():
            out = fn()
        torch.cuda.synchronize()
    finally:
        prof, rest = ops.profile_stop()
    return out, {k: len(v) for k, v in prof.items()}, {k: len(v) for k, v in rest.items()}


# ----------------------------------------------------------------------------------------------------------------- kernel level
def _multi_tile_batch():
    return multi_tile_cout(27) // 64          # T / 27 images of 27 tiles each (T = 270 on 256 compute units: 10 images)


def _k_shape(name, cins):
    """(B, Cin, H, W) of a named K case; cins = the Cin of (one-tile, model, odd-batch, multi-tile)"""
    return {"one-tile": (1, cins[0], 16, 32), "model": (2, cins[1], 32, 64), "odd-batch": (3, cins[2], 48, 96),
            "multi-tile": (_multi_tile_batch(), cins[3], 48, 288)}[name]


def _check_head(dev, pm, shape, what, twin=False, x_scale=1.0, gain=1.0):
    """One HEAD launch against the two-launch form; -> worst error / bound.  pm 2: plain bf16, the accumulators are the plain
    launch's (same kernel, same main loop): the 64-term bound alone.  pm 1: fp16 (hi | mid) -- the HEAD instance runs the 16x16x32
    main loop, conv3x3_split_pre's plain launch the 32x32x16 one: the two z differ by fp32 accumulation order over the 27 Cin product
    terms, |dz_c| <= 2 (27 Cin) u (|x| * |w|)_c, which reaches V through |L_c| |sc_c| (relu and the shift do not amplify)."""
    from onet_amd import ops
    B, Cin, H, W = shape
    Cout = 64
    x = (rnd(B, Cin, H, W, seed=400).abs() * x_scale).to(dev)
    w = rnd(Cout, Cin, 3, 3, seed=401, scale=(2.0 / (9 * Cin)) ** 0.5)
    save = _save(Cout, 402, dev, gain=gain)
    if pm == 2:
        P, wq, kw, kind = ops.split_pack_act(x, parts=1), ops.pack3x3_plain16(w.to(dev))[0], {}, "conv3x3_pre16_head_kernel"
        head = ops.conv3x3_plain16_pre_head
    else:
        s = ops.absmax_slots(x)
        P, wq, kw, kind = ops.split_pack_act(x, f16=True, slots=s), _pack(w.to(dev)), dict(slots=s), "conv3x3_split_pre_head_kernel"
        head = ops.conv3x3_split_pre_head
    if twin:                                   # L and V: the second half of tensors of 2B images (the twin batch's layout)
        LL = rnd(2 * B, Cout, H, W, seed=403).to(dev)
        VV = torch.full((2 * B, 1, H, W), float("nan"), device=dev)
        L, V = LL[B:], VV[B:]
    else:
        L = rnd(B, Cout, H, W, seed=403).to(dev)
        V = torch.full((B, 1, H, W), float("nan"), device=dev)
    assert bool((L < 0).any()) and bool((L > 0).any())
    z0 = ops.conv3x3_split_pre(P, wq, Cout, out=torch.full((B, Cout, H, W), float("nan"), device=dev), **kw)
    H0 = ops.bn_relu_apply(z0, save)
    assert torch.isfinite(H0).all() and bool((H0 == 0).any()) and bool((H0 > 0).any()), what
    got, kinds, _ = _mfma_kinds(lambda: head(P, wq, Cout, save, L, out=V, **kw))
    assert got is V and kinds == {kind: 1}, (what, kinds)
    if twin:
        assert bool(torch.isnan(VV[:B]).all()), what           # the other half is not this launch's
    terms = L.detach().cpu().double() * H0.detach().cpu().double()
    V64, A = terms.sum(1, keepdim=True), terms.abs().sum(1, keepdim=True)
    bound = DOT * A + 1e-30
    assert float(V64.abs().max()) > 1e3 * float(bound.max()), (what, float(V64.abs().max()), float(bound.max()))
    if pm == 1:
        xq = unsplit(P)
        k = round(float(torch.log2(xq.abs().max() / x.detach().cpu().double().abs().max())))          # the producer's 2^k
        xq = xq / 2.0 ** k
        assert float((xq - x.detach().cpu().double()).abs().max()) <= 2.0 ** -20 * float(xq.abs().max()), what
        # (the fp16 weight parts hold w to 2^-21 relative -- 22 bits in two parts: |w| (1 + 2^-21) bounds the dequantised |w|)
        aw = F.conv2d(xq.abs(), w.double().abs() * (1 + 2.0 ** -21), None, 1, 1)
        sc = save[2].detach().cpu().double().abs().view(1, -1, 1, 1)
        bound = bound + (L.detach().cpu().double().abs() * sc * (2 * 27 * Cin * U) * aw).sum(1, keepdim=True)
    Vh = V.detach().cpu().double()
    assert torch.isfinite(Vh).all(), what
    ratio = float(((Vh - V64).abs() / bound).max())
    print(f"{what}: worst error / bound {ratio:.2e} (max |V64| {float(V64.abs().max()):.3e}, largest bound {float(bound.max()):.3e})")
    assert ratio <= 1.0, f"{what}: {ratio:.3f} x the bound"
    V2 = torch.full_like(V, float("nan"))
    assert head(P, wq, Cout, save, L, out=V2, **kw) is V2
    torch.cuda.synchronize()
    assert torch.equal(V2, V), f"{what}: a second launch differs"
    return ratio


@pytest.mark.parametrize("name", ["one-tile", "model", "odd-batch", "multi-tile"])
def test_k1_plain_bf16_head_against_two_launch_form(dev, name):
    """K1: the plain bf16 instance.  |V - V64| <= 66 u sum_c |L H0| + 1e-30 for every pixel, V64 = sum_c L H0 in fp64 of the device's
    own H0 = bn_relu_apply(conv3x3_split_pre(P, wq)); max |V64| > 1e3 x the largest bound; a second launch bit-equal.
    Measured on an MI355X, worst error / bound: one-tile 0.017, model 0.023, odd-batch 0.028, multi-tile 0.030."""
    shape = _k_shape(name, (32, 64, 128, 32))
    _check_head(dev, 2, shape, f"K1 {name} {shape}")


def test_k1_plain_bf16_head_twin_layout(dev):
    """K1: L and V as the second half of tensors of 2B images (L_bs = that tensor's batch stride); the first half of V stays NaN.
    Measured on an MI355X: 0.024."""
    shape = _k_shape("model", (32, 64, 128, 32))
    _check_head(dev, 2, shape, f"K1 twin layout {shape}", twin=True)


@pytest.mark.parametrize("name", ["one-tile", "model", "odd-batch", "multi-tile"])
def test_k2_fp16_head_against_two_launch_form(dev, name):
    """K2: the fp16 (hi | mid) instance.  It does NOT share the plain launch's main loop (16x16x32 here, 32x32x16 there), so the bound
    is K1's plus sum_c |L_c| |sc_c| 2 (27 Cin) u (|x| * |w|)_c, the fp64 convolution of the absolute dequantised operands.
    Measured on an MI355X, worst error / bound: one-tile 2.1e-4, model 5.0e-5, odd-batch 2.4e-5, multi-tile 4.2e-4 (the accumulation-
    order term is a worst case over 27 Cin terms and dominates the bound: 5e-2 .. 1.3 against max |V64| of 35 .. 68; the measured
    error is of the size of K1's)."""
    shape = _k_shape(name, (16, 64, 128, 16))
    _check_head(dev, 1, shape, f"K2 {name} {shape}")


def test_k2_fp16_head_input_guard_and_twin_layout(dev):
    """K2: x at 1e5 (beyond fp16: the input's guard exponent is non-zero) with the coefficients scaled by 1e-4, L and V in the twin
    layout.  Measured on an MI355X: 4.6e-5."""
    shape = _k_shape("model", (16, 64, 128, 16))
    B, Cin, H, W = shape
    assert float((rnd(B, Cin, H, W, seed=400).abs() * 1e5).max()) >= 2 ** 15
    _check_head(dev, 1, shape, f"K2 guard {shape}", twin=True, x_scale=1e5, gain=1e-4)


@pytest.mark.parametrize("pm,Cin,Cout,H,W", [(2, 32, 64, 32, 48), (2, 32, 64, 24, 64), (2, 32, 128, 32, 64), (2, 48, 64, 32, 64),
                                             (1, 32, 64, 32, 48), (1, 32, 64, 24, 64), (1, 32, 128, 32, 64)],
                         ids=["bf16-W48", "bf16-H24", "bf16-Cout128", "bf16-Cin48", "fp16-W48", "fp16-H24", "fp16-Cout128"])
def test_k3_head_refuses(dev, pm, Cin, Cout, H, W):
    """K3: outside the domain the entry point returns 1, the wrapper None, and V is still all NaN."""
    from onet_amd import ops, _lib
    B = 1
    x = rnd(B, Cin, H, W, seed=430).abs().to(dev)
    w = rnd(Cout, Cin, 3, 3, seed=431, scale=0.1).to(dev)
    save = _save(Cout, 432, dev)
    L = rnd(B, Cout, H, W, seed=433).to(dev)
    V = torch.full((B, 1, H, W), float("nan"), device=dev)
    st = torch.cuda.current_stream().cuda_stream
    lib = _lib.load()
    if pm == 2:
        P = ops.split_pack_act(x, parts=1)
        wq = torch.zeros(Cin * 9 * Cout + 8, dtype=torch.bfloat16, device=dev) if Cin % 32 else ops.pack3x3_plain16(w)[0]
        rc = lib.onet_conv3x3_plain16_fwd_pre_head(P.data_ptr(), Cin * H * W // 2, wq.data_ptr(), save.data_ptr(), L.data_ptr(),
                                                   Cout * H * W, V.data_ptr(), B, Cin, Cout, H, W, st)
        got = ops.conv3x3_plain16_pre_head(P, wq, Cout, save, L, out=V)
    else:
        s = ops.absmax_slots(x)
        P, wq = ops.split_pack_act(x, f16=True, slots=s), _pack(w)
        rc = lib.onet_conv3x3_split_fwd_pre_head(P.data_ptr(), Cin * H * W, s.data_ptr(), 0, None, 0, wq.data_ptr(), save.data_ptr(),
                                                 L.data_ptr(), Cout * H * W, V.data_ptr(), B, Cin, Cout, H, W, st)
        got = ops.conv3x3_split_pre_head(P, wq, Cout, save, L, out=V, slots=s)
    torch.cuda.synchronize()
    assert rc == 1 and got is None
    assert bool(torch.isnan(V).all())


def test_k4_softmax2_labels(dev):
    """K4: S bit-equal to head_softmax_fwd_kernel's own (C = 1 with H = 1: fmaf(v, 1, 0) is exact, so that kernel reproduces V and
    yields its S), Y == argmax2(S) exactly, ties -> 0, each output alone."""
    from onet_amd import ops
    B, H, W = 3, 40, 25                                    # HW = 1000: not a multiple of the block size
    Vt, Vd = rnd(B, 1, H, W, seed=440, scale=50.0), rnd(B, 1, H, W, seed=441, scale=50.0)
    Vd[:, :, ::7, ::3] = Vt[:, :, ::7, ::3]                # exact ties
    Vd[:, :, 1::7, 1::3] = Vt[:, :, 1::7, 1::3] + 1e4      # pairs 1e4 apart, both ways
    Vd[:, :, 2::7, 2::3] = Vt[:, :, 2::7, 2::3] - 1e4
    Vt, Vd = Vt.to(dev), Vd.to(dev)
    one = torch.ones_like(Vt)
    Vt0, Vd0, S0 = ops.head_softmax_fwd(Vt, one, Vd, one)
    assert torch.equal(Vt0, Vt) and torch.equal(Vd0, Vd)
    Y0 = ops.argmax2(S0)
    S, Y = ops.softmax2_labels(Vt, Vd)
    torch.cuda.synchronize()
    assert S.dtype == torch.float32 and tuple(S.shape) == (B, 2, H, W) and Y.dtype == torch.int64 and tuple(Y.shape) == (B, H, W)
    assert torch.equal(S, S0), float((S - S0).abs().max())
    assert torch.equal(Y, Y0)
    tie = (Vt == Vd)[:, 0]
    assert int(tie.sum()) >= B * 6 * 9 and bool((Y[tie] == 0).all())
    assert bool(((S0[:, 1] > S0[:, 0]) == (Y == 1)).all())
    assert 0.3 < float(Y.double().mean()) < 0.7
    S1, none = ops.softmax2_labels(Vt, Vd, want_labels=False)
    assert none is None and torch.equal(S1, S0)
    none, Y1 = ops.softmax2_labels(Vt, Vd, want_S=False)
    assert none is None and torch.equal(Y1, Y0)
    with pytest.raises(ValueError):
        ops.softmax2_labels(Vt, Vd, want_S=False, want_labels=False)


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


_MODELS = {}


def _recipe(dev, which):
    """A: 2 x 1 x 128^2, shared (twin batch of 4).  B: 1 x 3 x 128^2, unshared, bias 0.1 (tests/test_gpu_fused_eval_bf16.py's recipes);
    the settings are the caller's.  Built once, the state never modified."""
    if which not in _MODELS:
        if which == "A":
            B, C, share, bias, seed = 2, 1, True, 0.0, 201
        else:
            B, C, share, bias, seed = 1, 3, False, 0.1, 202
        X = orc.det_input(B, C, 128, 128, seed=seed)
        top = _calibrated(orc.det_state_dict(C, 1981), X, bias)
        dwn = None if share else _calibrated(orc.det_state_dict(C, 1982), X, bias)
        m = _onet(_prefixed(top, dwn), C, share, dev)
        m.bias = bias
        _MODELS[which] = dict(B=B, X=X, Xg=X.to(dev), top=top, dwn=dwn, bias=bias, m=m, passes=1 if share else 2)
    return _MODELS[which]


def _check_against_forward(r, settings, new_kind, what, same_h):
    """scores / segment(head="fused") against the forward of the same model under the same settings: values (same_h: the activations of
    the two forms are bit-equal, L, H >= 0 make sum |L H| = V, and each form's V is within 66 u (1 + O(u)) V of the exact sum of the
    same fp32 terms: |V_scores - V_out| <= 2.1 x 66 u |V_out|), labels, launch records, plan report, determinism, buffers."""
    import onet_amd
    from onet_amd import ops
    m, Xg, B, passes = r["m"], r["Xg"], r["B"], r["passes"]
    m.settings = settings
    buf0 = {k: v.clone() for k, v in m.state_dict().items() if "running" in k or "num_batches" in k}
    out, k_fwd, o_fwd = _mfma_kinds(lambda: m(Xg))
    (Vt, Vd, S), k_sc, o_sc = _mfma_kinds(lambda: onet_amd.scores(m, Xg))
    lab, k_lab, o_lab = _mfma_kinds(lambda: onet_amd.segment(m, Xg, head="fused"))
    for got, ref, n in ((Vt, out[1], "Vt"), (Vd, out[3], "Vd"), (S, out[4], "S")):
        assert got.dtype == ref.dtype and tuple(got.shape) == tuple(ref.shape) and got.is_cuda and got.grad_fn is None, (what, n)
        assert torch.isfinite(got).all(), (what, n)
    if same_h:
        for got, ref, n in ((Vt, out[1], "Vt"), (Vd, out[3], "Vd")):
            assert bool((ref >= 0).all()), (what, n)
            bound = 2.1 * DOT * ref.double().abs() + 1e-30
            ratio = float(((got.double() - ref.double()).abs() / bound).max())
            print(f"{what} {n}: worst |V_scores - V_out| / (2.1 x 66 u |V_out|) = {ratio:.3f}")
            assert ratio <= 1.0, f"{what} {n}: {ratio:.3f} x the bound"
    # labels
    assert lab.dtype == torch.int64 and tuple(lab.shape) == (B, 128, 128)
    assert torch.equal(lab, m.predict_label(S)), what
    ref_lab = onet_amd.segment(m, Xg)
    if same_h:
        sure = ((out[1] - out[3]).abs() > 4 * DOT * torch.maximum(out[1], out[3]))[:, 0]
        share = float(sure.double().mean())
        print(f"{what}: label margin pixels {share:.4f}, labels differing anywhere {float((lab != ref_lab).double().mean()):.2e}")
        assert share > 0.9, (what, share)
        assert torch.equal(lab[sure], ref_lab[sure]), what
    # launch records, per pass: one launch of the new kind, one plain launch fewer, no head launch
    for kk, oo, n_lab in ((k_sc, o_sc, "scores"), (k_lab, o_lab, "segment")):
        assert kk.get(new_kind, 0) == passes and len(NEW_KINDS & set(kk)) == 1, (what, n_lab, kk)
        assert kk.get("conv3x3_split_pre_kernel", 0) == k_fwd["conv3x3_split_pre_kernel"] - passes, (what, n_lab, kk, k_fwd)
        assert {k: v for k, v in kk.items() if k not in NEW_KINDS | {"conv3x3_split_pre_kernel"}} == \
            {k: v for k, v in k_fwd.items() if k != "conv3x3_split_pre_kernel"}, (what, n_lab, kk, k_fwd)
        assert "onet_head_softmax_fwd" not in oo and oo.get("onet_softmax2_labels", 0) == 1, (what, n_lab, oo)
        assert "onet_argmax2" not in oo, (what, n_lab, oo)
    assert o_fwd.get("onet_head_softmax_fwd", 0) == 1 and not NEW_KINDS & set(k_fwd) and "onet_softmax2_labels" not in o_fwd, (k_fwd, o_fwd)
    # the plan report
    p0 = onet_amd.fused_eval_plan(m, Xg.shape)
    p1 = onet_amd.fused_eval_plan(m, Xg.shape, head="fused")
    assert p0["fused"] and p0["layers"]["up4.c2"] == "plain+head" and p1["layers"]["up4.c2"] == "fused+head", (p0, p1)
    assert sorted(p0) == sorted(p1) and {k: v for k, v in p1.items() if k != "layers"} == {k: v for k, v in p0.items() if k != "layers"}
    assert {k: v for k, v in p1["layers"].items() if k != "up4.c2"} == {k: v for k, v in p0["layers"].items() if k != "up4.c2"}
    # determinism, buffers
    Vt2, Vd2, S2 = onet_amd.scores(m, Xg)
    assert torch.equal(Vt2, Vt) and torch.equal(Vd2, Vd) and torch.equal(S2, S), what
    assert torch.equal(onet_amd.segment(m, Xg, head="fused"), lab), what
    for k, v in m.state_dict().items():
        if k in buf0:
            assert torch.equal(v, buf0[k]), k
    return out, (Vt, Vd, S), lab


def test_m1_one_part_plan_shared(dev):
    """M1: recipe A under Settings(conv="bf16", fused_eval="bf16").
    Measured on an MI355X: worst |V_scores - V_out| / bound Vt 0.042, Vd 0.041; label margin pixels 1.0000, no label differs anywhere."""
    from onet_amd import ops
    _check_against_forward(_recipe(dev, "A"), ops.Settings(conv="bf16", fused_eval="bf16"), "conv3x3_pre16_head_kernel", "M1 A", True)


def test_m2_one_part_plan_unshared_rgb(dev):
    """M2: recipe B (two U-Nets, two passes, bias 0.1, RGB stem), the same assertions.
    Measured on an MI355X: Vt 0.038, Vd 0.039; label margin pixels 1.0000, no label differs anywhere."""
    from onet_amd import ops
    _check_against_forward(_recipe(dev, "B"), ops.Settings(conv="bf16", fused_eval="bf16"), "conv3x3_pre16_head_kernel", "M2 B", True)


def test_m3_fp16_plan_against_the_oracle(dev):
    """M3: recipe A's model under Settings(conv="split", fused_eval=True): the fp16 HEAD instance (its main loop is not the plain
    launch's: no bit-level statement against the forward).  scores against the fp64 oracle within TOL of each tensor's largest
    magnitude, labels equal to the oracle's on the MARGIN pixels (more than 0.9 of all); launch records and plan as in M1.
    Measured on an MI355X: Vt 5.0e-6, Vd 4.1e-6, S 4.1e-5 (bound 2e-4); margin pixels 0.9940."""
    from onet_amd import ops
    r = _recipe(dev, "A")
    out, (Vt, Vd, S), lab = _check_against_forward(r, ops.Settings(conv="split", fused_eval=True), "conv3x3_split_pre_head_kernel",
                                                   "M3", False)
    with torch.no_grad():
        ref = orc.onet_forward(r["X"].double(), _f64(r["top"]), None, training=False, bias=r["bias"])
    errs = {}
    for got, b, n in ((Vt, ref[1], "Vt"), (Vd, ref[3], "Vd"), (S, ref[4], "S")):
        errs[n] = float((got.detach().cpu().double() - b).abs().max()) / (float(b.abs().max()) + 1e-30)
    print("M3: " + ", ".join(f"{n} {e:.2e}" for n, e in errs.items()))
    for n, e in errs.items():
        assert e <= TOL, f"M3 {n}: max err {e:.3e} of the tensor's largest magnitude (tol {TOL})"
    rVt, rVd = ref[1][:, 0], ref[3][:, 0]
    sure = (rVt - rVd).abs() > MARGIN * float(torch.maximum(rVt.abs().max(), rVd.abs().max()))
    share = float(sure.double().mean())
    print(f"M3: margin pixels {share:.4f}")
    assert share > 0.9, share
    assert torch.equal(lab.cpu().long()[sure], orc.predict_label(ref[4]).long()[sure])


@pytest.mark.parametrize("case", ["default", "direct", "depth0"])
def test_m4_fall_backs_are_the_forward(dev, case):
    """M4: where the fused plan does not apply -- Settings(), Settings(conv="direct", fused_eval="bf16") (no pre-split storage), a
    2 x 1 x 40 x 40 input (depth 0) -- scores / segment(head="fused") are the forward's tensors bit for bit and launch none of the new
    kinds."""
    import onet_amd
    from onet_amd import ops
    m = _onet(_prefixed(orc.det_state_dict(1, 1981)), 1, True, dev)
    side = 40 if case == "depth0" else 128
    m.settings = {"default": ops.Settings(), "direct": ops.Settings(conv="direct", fused_eval="bf16"),
                  "depth0": ops.Settings(conv="bf16", fused_eval="bf16")}[case]
    X = orc.det_input(2, 1, side, side, seed=113).to(dev)
    with torch.no_grad():
        out = m(X)
    (Vt, Vd, S), kinds, rest = _mfma_kinds(lambda: onet_amd.scores(m, X))
    lab, kinds2, rest2 = _mfma_kinds(lambda: onet_amd.segment(m, X, head="fused"))
    assert torch.equal(Vt, out[1]) and torch.equal(Vd, out[3]) and torch.equal(S, out[4]), case
    assert torch.equal(lab, onet_amd.segment(m, X)) and torch.equal(lab, m.predict_label(out[4])), case
    assert not NEW_KINDS & (set(kinds) | set(kinds2)), (kinds, kinds2)
    assert "onet_softmax2_labels" not in rest and "onet_softmax2_labels" not in rest2, (rest, rest2)
    p = onet_amd.fused_eval_plan(m, X.shape, head="fused")
    assert not p["fused"] and p == onet_amd.fused_eval_plan(m, X.shape), p
