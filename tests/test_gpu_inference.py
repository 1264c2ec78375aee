"""Eval-mode inference (`m.eval()`, `torch.no_grad()`, `m(X)`, `predict_label(S)`: what the reference's trainers run after every epoch
and on their test sets) against the fp64 CPU oracle, at the shapes where eval takes its own kernels.

In eval no concat buffer is pre-split (DoubleConv.pre_capable is false): the 256- and 128-pixel levels run the fp32-operand split
kernel (conv3x3_split_kernel, fp16 parts of x staged in the kernel), BatchNorm takes bn_eval_coeffs, the ConvTranspose2d the split
GEMM on fp32 inputs, and the head reads materialised activations.  Each case is compared element by element with
`orc.onet_forward(..., training=False)` evaluated in fp64 from the same state dict, and first proves -- from the launch records of
ops.profile_start(everything=False) -- that it ran the path it targets.

Bounds: every output within 2e-4 of its tensor's largest magnitude.  Eval has no batch statistics and ReLU / max-pooling are
continuous, so the outputs are a continuous function of the arithmetic and need no routing (tests/test_oracle_routing.py); labels
equal wherever the fp64 margin |Vt - Vd| exceeds 1e-3 max |V|.

The range-guard cases (R1-R3) scale every BatchNorm weight by 3e4 (tests/test_gpu_model.py::test_presplit_range_guard_large_gamma), so
that activations pass fp16's 65504 where the fp32 concat buffers of the decoder and the normalise-on-load operands feed the fp16
split kernels."""
import pytest
import torch

from oracle import onet_oracle as orc

pytestmark = pytest.mark.gpu

TOL = 2e-4          # eval outputs, of each tensor's largest magnitude
MARGIN = 1e-3       # labels compared where |Vt - Vd| exceeds this fraction of max |V| (fp64)
GAMMA = 3.0e4       # range-guard cases: every BatchNorm weight times this
BF16_TOL = 5e-3     # E1 under conv = "bf16" (see there)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from onet_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


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
    """every BatchNorm weight (the only 1-D weights) times g"""
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
    """Running statistics of a trained checkpoint for a shared-weight Onet: one fp64 training pass over both of its inputs, X and
    clip(1 - X + bias, 0, 1) (crop: of a corner of them -- the statistics of these i.i.d. pixel inputs hardly depend on the size)"""
    Xc = X if crop is None else X[..., :crop, :crop]
    return orc.calibrated_state(top, torch.cat([Xc, torch.clip(1 - Xc + bias, 0, 1)]))


def _eval(m, X, settings=None):
    """-> (outputs, kinds of the MFMA kernels launched) of one no_grad eval forward"""
    from onet_amd import ops
    if settings is not None:
        m.settings = settings
    ops.profile_start(everything=False)
    try:
        with torch.no_grad():
            out = m(X)
        torch.cuda.synchronize()
    finally:
        prof, _ = ops.profile_stop()
    return out, set(prof)


def _assert_eval_path(kinds, convt=True):
    """the default eval path: the in-staging split kernel on the fp32 tensors, the ConvTranspose2d GEMM, no pre-split kernel"""
    assert "conv3x3_split_kernel" in kinds, sorted(kinds)
    if convt:
        assert "convt_gemm_kernel" in kinds, sorted(kinds)
    assert not [k for k in kinds if k.endswith("_pre_kernel")], sorted(kinds)


def _margin(ref, margin=MARGIN):
    """pixels whose fp64 logits differ by more than `margin` of their scale: there the label is determined"""
    Vt, Vd = ref[1][:, 0], ref[3][:, 0]
    return (Vt - Vd).abs() > margin * float(torch.maximum(Vt.abs().max(), Vd.abs().max()))


def _compare(m, out, ref, tol, what, s_tol=None):
    """Lt, Vt, Ld, Vd, S element by element (S to s_tol when given); predict_label on the pixels with an fp64 margin of at least twice
    the logits' bound.  -> worst error"""
    errs = {n: float((a.detach().cpu().double() - b).abs().max()) / (float(b.abs().max()) + 1e-30)
            for a, b, n in zip(out, ref, ("Lt", "Vt", "Ld", "Vd", "S"))}
    print(f"{what}: " + ", ".join(f"{n} {e:.2e}" for n, e in errs.items()))
    for a, b, n in zip(out, ref, ("Lt", "Vt", "Ld", "Vd", "S")):
        close(a, b, tol if (n != "S" or s_tol is None) else s_tol, f"{what} {n}")
    sure = _margin(ref, max(MARGIN, 2 * tol))
    assert float(sure.double().mean()) > 0.9, what
    assert torch.equal(m.predict_label(out[4]).cpu().long()[sure], orc.predict_label(ref[4]).long()[sure]), what
    return max(errs.values())


def test_e1_eval_256_calibrated(dev):
    """E1: B = 2, 1 x 256^2, shared weights, calibrated statistics; one oracle evaluation, three Settings.  Also: a second eval
    forward with autograd enabled is bit-equal to the no_grad one; eval leaves the running statistics and num_batches_tracked alone;
    get_label (OV:204-219) is argmax / softmax of cat(Vt, Vd).
    conv = "bf16" keeps the 3x3 convolutions fp32 in eval (ops._fp32_algo) but gives the four ConvTranspose2d GEMMs bf16 operands (8
    significant bits: 2^-9 relative per operand); that rounding passes through the decoder into the logits -- measured 2.9e-3 of
    their scale, Lt untouched (7.9e-7) -- so the bound is 5e-3: the operand rounding with headroom, short of a wrong result (1e-2).
    Measured worst errors (all five outputs): default 7.0e-5 (S; logits 7.4e-6), split=False 1.5e-4 (S; logits 1.6e-5), bf16 logits
    2.9e-3, S 2.7e-2 (its bound: see below)."""
    from onet_amd import ops
    B, H = 2, 256
    X = orc.det_input(B, 1, H, H, seed=101)
    top = _calibrated(orc.det_state_dict(1, 1981), X)
    ref = _oracle(X, top)
    m = _onet(_prefixed(top), 1, True, dev)
    Xg = X.to(dev)
    buf0 = {k: v.clone() for k, v in m.state_dict().items() if "running" in k or "num_batches" in k}
    worst = {}
    for name, st, tol in (("default", ops.Settings(), TOL), ("split=False", ops.Settings(split=False), TOL),
                          ("bf16", ops.Settings(conv="bf16"), BF16_TOL)):
        out, kinds = _eval(m, Xg, st)
        if name == "default":
            _assert_eval_path(kinds)
            m.settings = st
            out2 = m(Xg)                                  # autograd enabled: the same kernels, the same bits
            assert all(torch.equal(a, b.detach()) for a, b in zip(out, out2))
            del out2
            lab, V = m.get_label(out[1], out[3])
            V64 = torch.softmax(torch.cat([out[1], out[3]], 1).double().cpu(), 1)
            assert float((V.double().cpu() - V64).abs().max()) <= 1e-6
            gap = (out[1] - out[3])[:, 0].abs().cpu()
            clear = gap > 1e-5 * float(gap.max())
            assert torch.equal(lab.cpu().long()[clear], (out[3] > out[1])[:, 0].long().cpu()[clear])
        else:
            assert not [k for k in kinds if k.endswith("_pre_kernel")], (name, sorted(kinds))
            if name == "split=False":
                assert "conv3x3_split_kernel" not in kinds, sorted(kinds)
        # (S = softmax(Vt - Vd) changes by at most a quarter of the logits' difference change: under bf16 operands |dV| ~ 1e-1 on
        # logits ~ 45 moves S by ~ 1e-2 where the softmax is not saturated -- S is held to that consequence of the logits' bound)
        s_tol = None if name != "bf16" else 0.25 * 2 * BF16_TOL * float(torch.maximum(ref[1].abs().max(), ref[3].abs().max()))
        worst[name] = _compare(m, out, ref, tol, f"E1 {name}", s_tol=s_tol)
    for k, v in m.state_dict().items():
        if k in buf0:
            assert torch.equal(v, buf0[k]), k
    print("E1 worst errors: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))


def test_e2_eval_512_rgb(dev):
    """E2: ZY-3 inference (test_pre_processing_on_zy3_testset: one 3-channel tile, img.unsqueeze(0)): B = 1, 3 x 512^2, shared,
    calibrated.  Measured worst error 7.9e-5 (S; logits 8.0e-6)."""
    B, C, H = 1, 3, 512
    X = orc.det_input(B, C, H, H, seed=102)
    top = _calibrated(orc.det_state_dict(C, 1981), X, crop=256)
    ref = _oracle(X, top)
    m = _onet(_prefixed(top), C, True, dev)
    out, kinds = _eval(m, X.to(dev))
    _assert_eval_path(kinds)
    print(f"E2 worst error {_compare(m, out, ref, TOL, 'E2'):.2e}")


def test_e3_eval_unshared_bias(dev):
    """E3: B = 2, 1 x 256^2, bshare=False (two passes, no twin batch), the randomised running statistics of det_state_dict,
    background bias 0.3 (OV:180).  Measured worst error 4.4e-6 (Vt)."""
    B, H = 2, 256
    X = orc.det_input(B, 1, H, H, seed=103)
    top, dwn = orc.det_state_dict(1, 1981), orc.det_state_dict(1, 1982)
    ref = _oracle(X, top, dwn, bias=0.3)
    m = _onet(_prefixed(top, dwn), 1, False, dev)
    m.bias = 0.3
    out, kinds = _eval(m, X.to(dev))
    _assert_eval_path(kinds)
    print(f"E3 worst error {_compare(m, out, ref, TOL, 'E3'):.2e}")


def test_e4_eval_odd_levels(dev):
    """E4: B = 3, 1 x 120 x 200 -- level sizes 60 x 100, 30 x 50, 15 x 25, 7 x 12: F.pad before the up1 concat, no concat buffer
    a multiple of 16.  Shared, calibrated.  Measured worst error 4.1e-5 (S; logits 3.6e-6)."""
    B, H, W = 3, 120, 200
    X = orc.det_input(B, 1, H, W, seed=104)
    top = _calibrated(orc.det_state_dict(1, 1981), X)
    ref = _oracle(X, top)
    m = _onet(_prefixed(top), 1, True, dev)
    out, kinds = _eval(m, X.to(dev))
    _assert_eval_path(kinds)
    print(f"E4 worst error {_compare(m, out, ref, TOL, 'E4'):.2e}")


def test_e5_eval_bilinear_unet(dev):
    """E5: UNet(bilinear=True) (OV:83-84: nn.Upsample, halved decoder channels, no ConvTranspose2d), B = 2, 1 x 256^2, calibrated;
    (x1, y1) against orc.unet_pass(..., training=False, bilinear=True).  Measured worst error 4.7e-6."""
    import Onet_vanilla_20240606 as ov
    B, H = 2, 256
    X = orc.det_input(B, 1, H, H, seed=105)
    sd = orc.calibrated_state(orc.det_state_dict(1, 1981, bilinear=True), X, bilinear=True)
    with torch.no_grad():
        ref = orc.unet_pass(X.double(), _f64(sd), training=False, bilinear=True)
    m = ov.UNet(n_channels=1, bilinear=True)
    m.load_state_dict(sd)
    m = m.to(dev).eval()
    out, kinds = _eval(m, X.to(dev))
    _assert_eval_path(kinds, convt=False)
    errs = [close(a, b, TOL, f"E5 {n}") for a, b, n in zip(out, ref, ("x1", "y1"))]
    print(f"E5 worst error {max(errs):.2e}")


def test_e6_eval_after_training_steps(dev):
    """E6: B = 2, 1 x 256^2, shared, calibrated; two training steps with FlatAdam (lr 1e-4: every parameter moves), then eval.  The
    oracle is built from the GPU model's parameters and buffers as they are then.  Measured worst error 7.4e-5 (S; logits 5.8e-6)."""
    from onet_amd.trainer import FlatAdam
    B, H = 2, 256
    X = orc.det_input(B, 1, H, H, seed=106)
    top = _calibrated(orc.det_state_dict(1, 1981), X)
    m = _onet(_prefixed(top), 1, True, dev).train()
    opt = FlatAdam(m, lr=1e-4)
    Xg = X.to(dev)
    Xt = orc.det_input(B, 1, H, H, seed=107).to(dev)
    for _ in range(2):
        opt.zero_grad()
        Lt, Vt, Ld, Vd, S = m(Xt)
        m.compute_loss(Lt, S[:, 0:1], Ld, S[:, 1:2]).backward()
        opt.step()
    m.eval()
    sd = {k[5:]: v for k, v in m.state_dict().items() if k.startswith("topu.")}
    moved = [k for k in top if "running" not in k and "num_batches" not in k and not torch.equal(sd[k].cpu(), top[k])]
    assert len(moved) == sum(1 for k in top if "running" not in k and "num_batches" not in k)
    assert int(sd["inc.double_conv.1.num_batches_tracked"]) == 4
    ref = _oracle(X, sd)
    out, kinds = _eval(m, Xg)
    _assert_eval_path(kinds)
    print(f"E6 worst error {_compare(m, out, ref, TOL, 'E6'):.2e}")


GAMMA_R1 = 1.0e5    # calibrated statistics keep |xhat| <~ 1.6 at level 0: 3e4 leaves the skip at 4.7e4, inside fp16's range


def test_r1_eval_range_guard(dev):
    """R1: eval at B = 4, 1 x 128^2 with every BatchNorm weight times 1e5 and statistics calibrated on the scaled network: the level-0
    skip half of the decoder's fp32 concat buffer passes 65504 (asserted on the oracle), and the fp16 parts of the in-staging split
    kernel need the guard exponent of the buffer's magnitude.  Outputs finite and within E1's bound of the oracle; S, a step function
    of logits ~4e10, on the pixels with an fp64 margin only.  Measured worst error 6.7e-6; without the guard (fp32 concat buffers
    without magnitude slots) Vt was off by 0.78 of its scale."""
    B, H = 4, 128
    X = orc.det_input(B, 1, H, H, seed=108)
    top = _calibrated(_gamma(orc.det_state_dict(1, 1981, head_gain=0.3), GAMMA_R1), X)
    ref = _oracle(X, top)
    assert float(ref[0].abs().max()) > 65504
    out, kinds = _eval(_onet(_prefixed(top), 1, True, dev), X.to(dev))
    _assert_eval_path(kinds)
    errs = [close(a, b, TOL, f"R1 {n}") for a, b, n in zip(out[:4], ref[:4], ("Lt", "Vt", "Ld", "Vd"))]
    sure = _margin(ref)
    assert torch.isfinite(out[4]).all()
    assert float((out[4].cpu().double() - ref[4]).abs().permute(1, 0, 2, 3)[:, sure].max()) <= TOL
    print(f"R1 worst error {max(errs):.2e}")


def _train_unet(st, X, bilinear=False):
    """one U-Net forward + backward of the test_presplit_range_guard_large_gamma loss at gamma 3e4 -> (x1, y1, gradients)"""
    from onet_amd import ops
    import Onet_vanilla_20240606 as ov
    if bilinear:
        m = ov.UNet(n_channels=1, bilinear=True)
        sd = orc.det_state_dict(1, 1981, head_gain=0.3, bilinear=True)
    else:
        m = ov.Onet(in_chns=1, binit=True, bshare=True)
        sd = orc.onet_state_dict(1, 1981, True, head_gain=0.3)
    m.load_state_dict(_gamma(sd, GAMMA))
    m = m.to(X.device).train()
    u = m if bilinear else m.topu
    with ops.using(st):
        x1, y1 = u(X)
        (x1 * y1).mean().mul(1.0 / GAMMA ** 2).backward()
    return x1.detach().clone(), y1.detach().clone(), {k: p.grad.detach().clone() for k, p in u.named_parameters()}


R2 = [("default", (4, 120, 200)), ("split-fp32", (8, 128, 128))]


@pytest.mark.parametrize("name,shape", R2 + [("bilinear", (8, 128, 128))], ids=["r2-default-120x200", "r2-split-fp32", "r3-bilinear"])
def test_r2_r3_training_range_guard(dev, name, shape):
    """R2: training where fp32 tensors above 65504 feed the fp16 split kernels -- default Settings at 120 x 200 (no level a multiple of
    16: every concat buffer fp32, the first two levels normalise on load), Settings(conv="split", presplit=False) at 128^2 -- and R3:
    UNet(bilinear=True) under default Settings (its concat buffers are never pre-split).  Every BatchNorm weight times 3e4; each held
    to the fp32 direct kernels (Settings(conv="direct", presplit=False)) with the bounds of test_presplit_range_guard_large_gamma:
    outputs to 2e-5 of their scale, every parameter gradient to 2e-2 (free ReLU / pooling decisions).  Measured worst relative
    gradient differences 8.1e-3 (120 x 200), 7.6e-3 (split, fp32 storage), 6.4e-3 (bilinear); without the guard the outputs were
    off by their whole scale."""
    from onet_amd import ops
    B, H, W = shape
    X = orc.det_input(B, 1, H, W, seed=109).to(dev)
    st = ops.Settings(conv="split", presplit=False) if name == "split-fp32" else ops.Settings()
    bil = name == "bilinear"
    a = _train_unet(ops.Settings(conv="direct", presplit=False), X, bil)
    ops.profile_start(everything=False)
    try:
        b = _train_unet(st, X, bil)
        torch.cuda.synchronize()
    finally:
        kinds = set(ops.profile_stop()[0])
    assert "conv3x3_split_kernel" in kinds, sorted(kinds)
    for i in range(2):
        assert torch.isfinite(b[i]).all(), (name, i)
        e = float((a[i] - b[i]).abs().max() / a[i].abs().max())
        assert e <= 2e-5, (name, i, e)
    worst = max((float((a[2][k] - b[2][k]).norm() / (a[2][k].norm() + 1e-30)), k) for k in a[2])
    print(f"{name}: outputs within 2e-5, worst relative gradient difference {worst[0]:.2e} ({worst[1]})")
    assert worst[0] <= 2e-2, worst


def test_benchmark_forward_takes_no_magnitude_pass(dev):
    """The fp32 split convolutions compute their input's magnitude slots themselves where its producer recorded none (eval and the
    fp32 concat buffers above).  At the benchmark shape (B = 32, 256^2, default Settings) every concat buffer is pre-split and every
    fp32 operand carries its producer's slots: the training forward must not launch that extra pass."""
    from onet_amd import ops
    import Onet_vanilla_20240606 as ov
    m = ov.Onet(in_chns=1, binit=True, bshare=True)
    m.load_state_dict(orc.onet_state_dict(1, 1981, True))
    m = m.to(dev).train()
    X = orc.det_input(32, 1, 256, 256, seed=110).to(dev)
    ops.profile_start(everything=True)
    try:
        m(X)
        torch.cuda.synchronize()
    finally:
        mfma, other = ops.profile_stop()
    assert "conv3x3_split_pre_kernel" in mfma, sorted(mfma)
    assert "onet_absmax_slots" not in other, len(other["onet_absmax_slots"])
