"""Ordinary PyTorch use of the Onet module beyond `zero_grad -> forward -> compute_loss -> one backward`: a second backward through a
retained graph, torch.autograd.grad (alone, then .backward(); with FlatAdam attached; with respect to part of the inputs), losses that
leave outputs without a gradient, parameters edited in place between forward and backward, an eval forward in between, gradient
accumulation through FlatAdam's flat buffer, create_graph.

The layers hand state to each other outside autograd (handoff.py: the link records of DoubleConv, the pooling and the head, the
decoder's up_link; placeholders for tensors that exist only pre-split; lazily built ConvTranspose2d input-gradient packs; gradients
written straight into FlatAdam's buffer).  Every test first checks, by counting the launches, that the hand-offs it targets really
run at its shape, then holds the gradients to the fp64 oracle under the HIP run's own ReLU / pooling decisions
(tests/test_gpu_gradients.py: GRAD_TOL on every element of every parameter) or bit for bit to a plain run.

Shapes: B = 2, one channel.  The slot-operand ConvTranspose2d backward (and with it the decoder's up_link) needs a 3x3 layer of the
finest decoder level that fills the chip with split tiles: 128 x 256 under the twin batch.  The fp32-MFMA path (split=False) folds a
BatchNorm-backward reduce into an input gradient only in the F(4x4) kernel, which the dispatch takes where its blocks fill the chip:
also 128 x 256 under the twin batch.  Without the twin batch (twin=False, bshare=False) only the pooling link runs below 256 x 256,
so those configurations run at 64 x 64."""
import types

import pytest
import torch

from oracle import onet_oracle as orc
from tests.test_gpu_gradients import GRAD_TOL, _check, _record_units, _to64

pytestmark = pytest.mark.gpu

GAIN = 0.3
SLOT_SHAPE = (2, 1, 128, 256)
SMALL_SHAPE = (2, 1, 64, 64)
# tag: (Settings keyword arguments, bshare, shape)
CONFIGS = {
    "default": ({}, True, SLOT_SHAPE),
    "twin_off": ({"twin": False}, True, SMALL_SHAPE),
    "split_off": ({"split": False}, True, SLOT_SHAPE),
    "unshared": ({}, False, SMALL_SHAPE),
}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _model(dev, cfg, seed=1981):
    import Onet_vanilla_20240606 as ov
    from onet_amd import ops
    kw, bshare, _ = CONFIGS[cfg]
    m = ov.Onet(in_chns=1, binit=True, bshare=bshare)
    m.load_state_dict(orc.onet_state_dict(1, seed, bshare, head_gain=GAIN))
    m = m.to(dev).train()
    m.settings = ops.Settings(**kw)
    return m


def _input(cfg, dev, seed=7):
    B, C, H, W = CONFIGS[cfg][2]
    return orc.det_input(B, C, H, W, seed=seed).to(dev)


def _loss(m, X):
    Lt, Vt, Ld, Vd, S = m(X)
    return m.compute_loss(Lt, S[:, 0].unsqueeze(1), Ld, S[:, 1].unsqueeze(1)), (Lt, Vt, Ld, Vd, S)


def _grads(m):
    return {k: p.grad.detach().clone() for k, p in m.named_parameters()}


def _as_named(grads):
    """`_check` reads `named[k].grad`: a plain dict of gradient tensors in that form (keys without the "topu." prefix)"""
    return {(k[5:] if k.startswith("topu.") else k): types.SimpleNamespace(grad=g) for k, g in grads.items()}


def _stats(m):
    return [b.detach().clone() for n, b in m.named_buffers() if "running" in n or "num_batches" in n]


HANDOFFS = ("conv3x3_split_dgrad_pre_slots", "convT2x2_dgrad_slots", "convT2x2_wgrad_slots", "conv3x3_split_dgrad_pre_bnreduce",
            "conv3x3_dgrad_bnreduce", "maxpool2_bwd", "head_softmax_fwd")


def _count_handoffs(monkeypatch):
    """Spies on the launches that consume a hand-off; -> the dict of counts (a fused launch counts only where it was taken)."""
    from onet_amd import ops
    used = {}
    for name in HANDOFFS:
        real = getattr(ops, name)

        def spy(*a, _real=real, _name=name, **k):
            out = _real(*a, **k)
            took = out is not None
            if _name == "maxpool2_bwd":
                took = k.get("bn") is not None and isinstance(out, tuple) and out[1] is not None
            elif _name == "head_softmax_fwd":
                took = k.get("h_norm") is not None
            if took:
                used[_name] = used.get(_name, 0) + 1
            return out

        monkeypatch.setattr(ops, name, spy)
    return used


def _assert_handoffs(cfg, used):
    """The hand-offs a configuration takes at its shape, from one forward + backward (see the module's note on shapes)."""
    assert used.get("maxpool2_bwd", 0) >= 1, used                     # pooling backward with the BatchNorm reduce
    if cfg == "split_off":                                            # fp32 path: the F(4x4) input gradient with the reduce
        assert used.get("conv3x3_dgrad_bnreduce", 0) >= 1, used
    if cfg == "default":
        assert used.get("conv3x3_split_dgrad_pre_bnreduce", 0) >= 1, used                 # fused dgrad reduce, pre-split operands
        assert used.get("conv3x3_split_dgrad_pre_slots", 0) >= 1, used
        assert used.get("convT2x2_dgrad_slots", 0) >= 1 and used.get("convT2x2_wgrad_slots", 0) >= 1, used
        assert used.get("head_softmax_fwd", 0) == 1, used             # the head normalising the last unit on load


_ORACLE = {}


def _oracle(cfg, dev):
    """Per configuration, cached for the module: the routed fp64 oracle's graph (X and the parameters fp64 leaves, the HIP run's
    decisions), the routing, and the oracle's gradients of the training loss."""
    if cfg in _ORACLE:
        return _ORACLE[cfg]
    _, bshare, (B, C, H, W) = CONFIGS[cfg]
    X = _input(cfg, dev)
    m = _model(dev, cfg)
    with pytest.MonkeyPatch.context() as mp:
        rec, finish = _record_units(mp, B, range(B), dev)
        m.zero_grad()
        loss, _ = _loss(m, X)
        loss.backward()
        acts = finish()
    assert len(acts) == 36
    r = orc.Routing.from_activations(acts)
    top = orc.clone_state(_to64(orc.det_state_dict(C, 1981, head_gain=GAIN)))
    dwn = None if bshare else orc.clone_state(_to64(orc.det_state_dict(C, 1982, head_gain=GAIN)))
    X64 = X.cpu().double().requires_grad_(True)
    outs = orc.onet_forward(X64, top, dwn, training=True, routing=r)
    Lt, Vt, Ld, Vd, S = outs
    oloss = orc.compute_loss(Lt, S[:, 0:1], Ld, S[:, 1:2])
    leaves = {k: v for k, v in top.items() if v.requires_grad}
    if dwn is not None:
        leaves.update({"dwnu." + k: v for k, v in dwn.items() if v.requires_grad})
    o = types.SimpleNamespace(X=X64, outs=outs, loss=oloss, leaves=leaves, routing=r, bshare=bshare)
    g = torch.autograd.grad(oloss, list(leaves.values()) + [X64], retain_graph=True)      # (one fp64 backward for both)
    o.grads, o.gX = dict(zip(leaves, g[:-1])), g[-1]
    _ORACLE[cfg] = o
    return o


def _ograds(o, loss, wrt=None):
    keys = list(o.leaves) if wrt is None else wrt
    g = torch.autograd.grad(loss, [o.leaves[k] for k in keys], retain_graph=True)
    return dict(zip(keys, g))


def _hip_named(m):
    return {(k[5:] if k.startswith("topu.") else k): v for k, v in m.named_parameters()}


# ----------------------------------------------------------------------------------------------------------------- case 1
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_second_backward_through_a_retained_graph(dev, cfg, monkeypatch):
    """loss.backward(retain_graph=True) then loss.backward(): the first backward is the single backward's, bit for bit; the second
    one's contribution is the oracle's gradient; the BatchNorm running statistics do not move in either backward."""
    o = _oracle(cfg, dev)
    X = _input(cfg, dev)
    m = _model(dev, cfg)
    m.zero_grad()
    loss, _ = _loss(m, X)
    loss.backward()
    g_single = _grads(m)

    m = _model(dev, cfg)
    used = _count_handoffs(monkeypatch)
    m.zero_grad()
    loss, _ = _loss(m, X)
    st0 = _stats(m)
    loss.backward(retain_graph=True)
    _assert_handoffs(cfg, used)
    g1 = _grads(m)
    loss.backward()
    g2 = _grads(m)
    for a, b in zip(st0, _stats(m)):
        assert torch.equal(a, b), "a backward moved the BatchNorm running statistics"
    for k in g1:
        assert torch.equal(g1[k], g_single[k]), (cfg, k, "first backward of a retained graph differs from a single backward")
        # the second backward runs the same kernels on the same hand-offs: the same bits again
        assert torch.equal(g2[k], 2 * g1[k]), (cfg, k, float((g2[k] - 2 * g1[k]).abs().max()))
    _check(m, o.grads, o.routing, f"retain_graph second backward ({cfg})",
           named=_as_named({k: g2[k] - g1[k] for k in g1}))


def test_second_backward_through_a_retained_graph_bf16(dev, monkeypatch):
    """The bf16 conv path (BASELINE configs[2]) at the slot-operand shape: both backwards finish, every gradient is finite, and the
    second backward reproduces the first one's kernels exactly."""
    X = _input("default", dev)
    m = _model(dev, "default")
    m.settings = m.settings.replace(conv="bf16")
    used = _count_handoffs(monkeypatch)
    m.zero_grad()
    loss, _ = _loss(m, X)
    loss.backward(retain_graph=True)
    assert used.get("convT2x2_dgrad_slots", 0) >= 1 and used.get("conv3x3_split_dgrad_pre_slots", 0) >= 1, used
    g1 = _grads(m)
    loss.backward()
    g2 = _grads(m)
    for k in g1:
        assert bool(torch.isfinite(g1[k]).all()) and bool(torch.isfinite(g2[k]).all()), k
        assert torch.equal(g2[k], 2 * g1[k]), (k, float((g2[k] - 2 * g1[k]).abs().max()))


# ----------------------------------------------------------------------------------------------------------------- case 2
@pytest.mark.parametrize("cfg", ["default", "twin_off"])
def test_autograd_grad_then_backward(dev, cfg, monkeypatch):
    """torch.autograd.grad(loss, params, retain_graph=True) returns the oracle's gradients and leaves every .grad None; a following
    loss.backward() fills .grad with them again."""
    o = _oracle(cfg, dev)
    X = _input(cfg, dev)
    m = _model(dev, cfg)
    used = _count_handoffs(monkeypatch)
    m.zero_grad()
    loss, _ = _loss(m, X)
    names = [k for k, _ in m.named_parameters()]
    gs = torch.autograd.grad(loss, [p for _, p in m.named_parameters()], retain_graph=True)
    _assert_handoffs(cfg, used)
    assert all(p.grad is None for p in m.parameters())
    _check(m, o.grads, o.routing, f"autograd.grad ({cfg})", named=_as_named(dict(zip(names, gs))))
    loss.backward()
    _check(m, o.grads, o.routing, f"backward after autograd.grad ({cfg})")


def test_autograd_grad_with_flat_adam_returns_gradients_of_its_own(dev, monkeypatch):
    """With FlatAdam attached, what torch.autograd.grad returns must not be a view of the flat gradient buffer: a later zero_grad and
    a further step leave it unchanged."""
    from onet_amd.trainer import FlatAdam
    X = _input("default", dev)
    m = _model(dev, "default")
    opt = FlatAdam(m, lr=5e-6)
    opt.zero_grad()
    used = _count_handoffs(monkeypatch)
    loss, _ = _loss(m, X)
    gs = torch.autograd.grad(loss, list(m.parameters()))
    _assert_handoffs("default", used)
    kept = [g.clone() for g in gs]
    lo, hi = opt.gflat.data_ptr(), opt.gflat.data_ptr() + 4 * opt.gflat.numel()
    assert not any(lo <= g.data_ptr() < hi for g in gs), "autograd.grad handed out a view of FlatAdam's gradient buffer"
    opt.zero_grad()
    loss, _ = _loss(m, X)
    loss.backward()
    opt.step()
    for g, k in zip(gs, kept):
        assert torch.equal(g, k)


# ----------------------------------------------------------------------------------------------------------------- case 3
@pytest.mark.parametrize("cfg", ["default", "twin_off"])
def test_partial_graphs(dev, cfg, monkeypatch):
    """autograd.grad with respect to one weight or to X alone (needs_input_grad combinations the training step never produces), and
    losses that leave some outputs without a gradient (None gradients into the head, the JSD sums, the twin split and the skip
    pooling): each against the oracle's gradient of the same loss."""
    o = _oracle(cfg, dev)
    X = _input(cfg, dev)
    m = _model(dev, cfg)
    named = _hip_named(m)
    Xg = X.clone().requires_grad_(True)
    used = _count_handoffs(monkeypatch)
    loss, (Lt, Vt, Ld, Vd, S) = _loss(m, Xg)
    (gx,) = torch.autograd.grad(loss, [Xg], retain_graph=True)
    _assert_handoffs(cfg, used)
    # d loss / dX: the same statement _check makes of a parameter gradient (relative L2, and no element off by more than 20 x that
    # of the largest magnitude)
    gx, t = gx.cpu().double(), o.gX
    e, emax = float((gx - t).norm() / t.norm()), float((gx - t).abs().max() / t.abs().max())
    print(f"autograd.grad wrt X ({cfg}): relative error {e:.2e}, worst element {emax:.2e} of the largest")
    assert e <= GRAD_TOL and emax <= 20 * GRAD_TOL, (e, emax)
    for k in ("inc.double_conv.0.weight", "up1.up.weight"):
        (g,) = torch.autograd.grad(loss, [named[k]], retain_graph=True)
        _check(m, {k: o.grads[k]}, o.routing, f"autograd.grad wrt {k} ({cfg})", named=_as_named({k: g}))
    oLt, oVt, oLd, oVd, oS = o.outs
    for what, hl, ol in (("Vt.mean()", Vt.mean(), oVt.mean()),
                         ("jsd(Lt, St, Sd)", m.jensen_shannon_divergence(Lt, S[:, 0].unsqueeze(1), S[:, 1].unsqueeze(1)),
                          orc.jsd(oLt, oS[:, 0:1], oS[:, 1:2]))):
        m.zero_grad()
        hl.backward(retain_graph=True)
        _check(m, _ograds(o, ol), o.routing, f"{what} alone ({cfg})")


# ----------------------------------------------------------------------------------------------------------------- case 4
EDITS = ("inc.double_conv.0.weight", "inc.double_conv.1.weight", "inc.double_conv.1.bias", "up1.up.weight", "up4.up.bias")


def _torch_raises_on_edit(key, bshare):
    """The same edit on the oracle's CPU graph: does torch's own backward raise?"""
    top = orc.clone_state(orc.det_state_dict(1, 1981, head_gain=GAIN))
    dwn = None if bshare else orc.clone_state(orc.det_state_dict(1, 1982, head_gain=GAIN))
    X = orc.det_input(2, 1, 32, 32)
    Lt, Vt, Ld, Vd, S = orc.onet_forward(X, top, dwn, training=True)
    loss = orc.compute_loss(Lt, S[:, 0:1], Ld, S[:, 1:2])
    with torch.no_grad():
        top[key].mul_(1.01)
    try:
        loss.backward()
    except RuntimeError as e:
        assert "modified by an inplace operation" in str(e)
        return True
    return False


@pytest.mark.parametrize("cfg", ["default", "twin_off"])
def test_in_place_parameter_edit_between_forward_and_backward(dev, cfg, monkeypatch):
    """p.mul_(1.01) under no_grad between forward and backward: where torch raises, so does the HIP model; where torch does not,
    the gradients are those of the unedited forward."""
    o = _oracle(cfg, dev)
    X = _input(cfg, dev)
    used = _count_handoffs(monkeypatch)
    for key in EDITS:
        used.clear()
        raises = _torch_raises_on_edit(key, o.bshare)
        m = _model(dev, cfg)
        m.zero_grad()
        loss, _ = _loss(m, X)
        with torch.no_grad():
            _hip_named(m)[key].mul_(1.01)
        if raises:
            with pytest.raises(RuntimeError, match="modified by an inplace operation"):
                loss.backward()
        else:
            loss.backward()
            _check(m, o.grads, o.routing, f"{key} edited after forward ({cfg})")
            _assert_handoffs(cfg, used)
        print(f"{cfg}: {key} edited between forward and backward: torch raises {raises}")


def test_optimizer_step_between_forward_and_backward_raises(dev, monkeypatch):
    """torch.optim.Adam on the oracle's leaves between a forward and its backward makes the backward raise; FlatAdam.step() (a
    kernel writing the parameters through a pointer) must too."""
    from onet_amd.trainer import FlatAdam
    top = orc.clone_state(orc.det_state_dict(1, 1981, head_gain=GAIN))
    X = orc.det_input(2, 1, 32, 32)
    opt = torch.optim.Adam([v for v in top.values() if v.requires_grad], lr=5e-6)
    for i in range(2):
        Lt, Vt, Ld, Vd, S = orc.onet_forward(X, top, None, training=True)
        loss = orc.compute_loss(Lt, S[:, 0:1], Ld, S[:, 1:2])
        if i == 1:
            opt.step()
            with pytest.raises(RuntimeError, match="modified by an inplace operation"):
                loss.backward()
        else:
            loss.backward()
    Xh = _input("default", dev)
    m = _model(dev, "default")
    fopt = FlatAdam(m, lr=5e-6)
    fopt.zero_grad()
    used = _count_handoffs(monkeypatch)
    loss, _ = _loss(m, Xh)
    loss.backward()
    _assert_handoffs("default", used)
    loss, _ = _loss(m, Xh)
    fopt.step()
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        loss.backward()


# ----------------------------------------------------------------------------------------------------------------- case 6
@pytest.mark.parametrize("cfg", ["default", "twin_off"])
def test_eval_forward_between_forward_and_backward(dev, cfg, monkeypatch):
    """train forward, m.eval() + a no_grad forward of another input, m.train(), then the first loss's backward: the gradients are
    those of a run without the eval forward, bit for bit."""
    X, X2 = _input(cfg, dev), _input(cfg, dev, seed=11)
    m = _model(dev, cfg)
    m.zero_grad()
    loss, _ = _loss(m, X)
    loss.backward()
    ref = _grads(m)
    m = _model(dev, cfg)
    m.zero_grad()
    used = _count_handoffs(monkeypatch)
    loss, _ = _loss(m, X)
    m.eval()
    with torch.no_grad():
        m(X2)
    m.train()
    loss.backward()
    _assert_handoffs(cfg, used)             # (the eval forward takes none of them: no link, no head normalisation)
    for k, g in _grads(m).items():
        assert torch.equal(g, ref[k]), (cfg, k)


# ----------------------------------------------------------------------------------------------------------------- case 7
@pytest.mark.parametrize("cfg", ["default", "twin_off"])
def test_gradient_accumulation_through_flat_adam(dev, cfg, monkeypatch):
    """Two micro-batch backwards after one zero_grad: the first writes its gradients into FlatAdam's buffer, autograd adds the
    second.  The buffer holds the fp32 sum of the two separate gradients, bit for bit, and the step is torch.optim.Adam's on it."""
    from onet_amd.trainer import FlatAdam
    Xa, Xb = _input(cfg, dev), _input(cfg, dev, seed=11)
    sep = []
    for X in (Xa, Xb):
        m = _model(dev, cfg)
        m.zero_grad()
        _loss(m, X)[0].backward()
        sep.append(_grads(m))
    m = _model(dev, cfg)
    p0 = {k: p.detach().clone() for k, p in m.named_parameters()}
    opt = FlatAdam(m, lr=5e-6)
    opt.zero_grad()
    for X in (Xa, Xb):
        used = _count_handoffs(monkeypatch)
        _loss(m, X)[0].backward()
        _assert_handoffs(cfg, used)
    for (k, p), off in zip(m.named_parameters(), opt.offsets):
        assert torch.equal(p.grad, sep[0][k] + sep[1][k]), (cfg, k)
        if cfg == "default":        # (the twin batch: one contribution per backward, the first one written in the buffer's slot)
            g = opt.gflat[off:off + p.numel()].view_as(p)
            assert p.grad.data_ptr() == g.data_ptr() and torch.equal(g, sep[0][k] + sep[1][k]), (cfg, k)
    opt.step()
    ref = {k: v.clone().requires_grad_(True) for k, v in p0.items()}
    topt = torch.optim.Adam(list(ref.values()), lr=5e-6, betas=(0.9, 0.999), eps=1e-8)
    for k, v in ref.items():
        v.grad = sep[0][k] + sep[1][k]
    topt.step()
    for k, p in m.named_parameters():
        d = float((p.detach() - ref[k].detach()).abs().max())
        assert d <= 1e-6 * float(ref[k].detach().abs().max()) + 1e-3 * 5e-6, (cfg, k, d)


# ----------------------------------------------------------------------------------------------------------------- create_graph
def test_double_differentiation_is_refused_with_a_clear_message(dev):
    X = _input("twin_off", dev)
    m = _model(dev, "twin_off")
    loss, _ = _loss(m, X)
    with pytest.raises(RuntimeError, match="double differentiation"):
        torch.autograd.grad(loss, list(m.parameters()), create_graph=True)


# ----------------------------------------------------------------------------------------------------------------- case 5
def _blocks(m):
    from onet_amd.modules import DoubleConv, Down, Up
    return [(n, mod) for n, mod in m.topu.named_modules() if isinstance(mod, (DoubleConv, Down, Up))]


def _hooked_run(m, X, scale_down4=False):
    """Forward + loss + backward with a forward hook on every DoubleConv, Down and Up of topu: -> (outputs seen by the hooks, the
    names of the blocks whose hook got a placeholder, loss, S, gradients).  scale_down4: down4's hook returns out * 0.5."""
    from onet_amd import ops
    seen, bad, handles = {}, [], []
    for n, mod in _blocks(m):
        def hook(mod, inp, out, n=n):
            if ops.is_placeholder(out):
                bad.append(n)
            seen.setdefault(n, []).append(out.detach().clone())
            return out * 0.5 if (scale_down4 and n == "down4") else None
        handles.append(mod.register_forward_hook(hook))
    try:
        m.zero_grad()
        loss, outs = _loss(m, X)
        loss.backward()
    finally:
        for h in handles:
            h.remove()
    return seen, bad, loss.detach(), outs[4].detach(), _grads(m)


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


def _rel_l2(a, b):
    """relative L2 error of a tensor (the measure _check applies per parameter)"""
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


@pytest.mark.parametrize("cfg", ["default", "split_off"])
def test_forward_hooks_on_inner_blocks(dev, cfg, monkeypatch):
    """Forward hooks on every DoubleConv / Down / Up in training mode.  Read-only hooks see real activations (no placeholder), equal to
    the same blocks' outputs of a Settings(presplit=False, bn_on_load=False) run; loss, S and gradients stay those of the unhooked
    model.  A hook on down4 that returns out * 0.5 changes the result, as it does on the presplit=False model.

    A hooked network takes the plain fp32 hand-offs (modules._hooked), which may run other kernels than the unhooked one (fp32 concat
    buffers instead of pre-split ones, the pooling pass separate): hence 1e-5 against the unhooked run, not bit identity.  Under
    Settings() that also moves a few ReLU decisions, and the gradients of two runs with different decisions differ by ~3e-3 (the
    decision noise of tests/test_gpu_gradients.py's header), so there the gradients of the hooked runs are held to the routed fp64
    oracle under their own decisions instead of to another run."""
    X = _input(cfg, dev)
    m = _model(dev, cfg)
    used = _count_handoffs(monkeypatch)
    m.zero_grad()
    loss0, outs0 = _loss(m, X)
    loss0.backward()
    _assert_handoffs(cfg, used)         # (the unhooked model takes the hand-offs a hook must not be bypassed by)
    g0, S0 = _grads(m), outs0[4].detach()
    m = _model(dev, cfg)
    seen, bad, loss, S, g = _hooked_run(m, X)
    assert not bad, ("a hook was handed a placeholder", bad)
    assert len(seen) == len(_blocks(m)) == 17, sorted(seen)            # 9 DoubleConv, 4 Down, 4 Up
    assert _rel(loss, loss0.detach()) <= 1e-5 and _rel(S, S0) <= 1e-5, (_rel(loss, loss0.detach()), _rel(S, S0))
    worst = max(float((g[k] - g0[k]).norm() / g0[k].norm()) for k in g0)
    assert cfg == "default" or worst <= GRAD_TOL, worst
    ref = _model(dev, cfg)
    ref.settings = ref.settings.replace(presplit=False, bn_on_load=False)
    rseen, rbad, rloss, rS, rg = _hooked_run(ref, X)
    assert not rbad
    # (the pre-split and the fp32-operand split kernels round differently: measured 1.1e-5 of the largest element at the last block under
    # Settings(), relative L2 well below)
    worst_out = max(_rel_l2(a, b) for n, outs in seen.items() for a, b in zip(outs, rseen[n]))
    assert worst_out <= 1e-5, worst_out
    # a hook that replaces down4's output: every reader of that output must read the replacement
    m = _model(dev, cfg)
    if cfg == "default":
        B = X.shape[0]
        with pytest.MonkeyPatch.context() as mp:
            _, finish = _record_units(mp, B, range(B), dev)
            _, bad, hloss, hS, hg = _hooked_run(m, X, scale_down4=True)
            acts = finish()
        real_dc = orc._double_conv
        monkeypatch.setattr(orc, "_double_conv", lambda x, st, block, *a, **k: real_dc(x, st, block, *a, **k) * (0.5 if block == "down4" else 1.0))
        r = orc.Routing.from_activations(acts)
        top = orc.clone_state(_to64(orc.det_state_dict(1, 1981, head_gain=GAIN)))
        oLt, oVt, oLd, oVd, oS = orc.onet_forward(X.cpu().double(), top, None, training=True, routing=r)
        oloss = orc.compute_loss(oLt, oS[:, 0:1], oLd, oS[:, 1:2])
        g64 = dict(zip([k for k, v in top.items() if v.requires_grad],
                       torch.autograd.grad(oloss, [v for v in top.values() if v.requires_grad])))
        assert _rel(hloss, oloss.detach()) <= 1e-5, _rel(hloss, oloss.detach())
        _check(m, g64, r, "down4 hook returning out * 0.5 (default)")
    else:
        _, bad, hloss, hS, hg = _hooked_run(m, X, scale_down4=True)
    ref = _model(dev, cfg)
    ref.settings = ref.settings.replace(presplit=False, bn_on_load=False)
    _, _, rloss, rS, rg = _hooked_run(ref, X, scale_down4=True)
    assert not bad
    assert _rel(hloss, loss0.detach()) > 1e-4 or _rel(hS, S0) > 1e-4, "the replacement returned by the hook was not read"
    assert _rel(hloss, rloss) <= 1e-5 and _rel(hS, rS) <= 1e-5, (_rel(hloss, rloss), _rel(hS, rS))
    worst_r = max(float((hg[k] - rg[k]).norm() / rg[k].norm()) for k in rg)
    assert cfg == "default" or worst_r <= GRAD_TOL, worst_r
    print(f"forward hooks ({cfg}): block outputs vs presplit=False {worst_out:.1e}; read-only vs unhooked: loss {_rel(loss, loss0.detach()):.1e}, S {_rel(S, S0):.1e}, gradients "
          f"{worst:.2e}; down4 * 0.5 vs presplit=False: loss {_rel(hloss, rloss):.1e}, gradients {worst_r:.2e}")
