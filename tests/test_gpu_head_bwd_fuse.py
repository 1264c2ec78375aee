"""The twin head's backward fused with the last unit's BatchNorm-backward reduce (ops.head_grad_map + ops.head_bwd_reduce, and the
apply pass that forms da = g L on load: ops.bn_relu_bwd_split(da_gl=...)) against the unfused kernels it replaces in the step
(ops.head_softmax_bwd writing dH, bn_relu_bwd_reduce_kernel and the apply pass reading it), and against fp64 on the host."""
import numpy as np
import pytest
import torch

from oracle import onet_oracle as orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _inputs(B2, C, H, W, dev, seed):
    """A twin batch of B2 images (two statistics groups of B2 / 2): L, the last unit's pre-activation z with coefficients made from
    its own group statistics, the head's saved S and upstream gradients of the sizes a training step produces."""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    B = B2 // 2
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float32)
    L = rn(B2, C, H, W)
    z = rn(B2, C, H, W) * (0.5 + torch.rand(C, generator=gen).view(1, C, 1, 1)) + 0.3 * rn(1, C, 1, 1)
    save = torch.empty(2, 4, C)
    for g in range(2):
        zg = z[g * B:(g + 1) * B].double()
        mean, var = zg.mean(dim=(0, 2, 3)), zg.var(dim=(0, 2, 3), unbiased=False)
        invstd = 1.0 / torch.sqrt(var + 1e-5)
        gamma, beta = 1.0 + 0.2 * rn(C).double(), 0.2 * rn(C).double()
        save[g, 0], save[g, 1], save[g, 2] = mean.float(), invstd.float(), (gamma * invstd).float()
        save[g, 3] = beta.float()
    S = torch.softmax(3.0 * rn(B, 2, H, W), dim=1)
    n = B * H * W
    dVt, dVd, dS = rn(B, 1, H, W) / n, rn(B, 1, H, W) / n, rn(B, 2, H, W) / n
    gst, gsd = rn(B, 1, H, W) / n, rn(B, 1, H, W) / n
    return [t.to(dev).contiguous() for t in (L, z, save, S, dVt, dVd, dS, gst, gsd)]


def _amax_value(slots):
    return float(slots.view(torch.float32).max())


def _record_sums(rec4):
    """[2 * np][C][4] (hi, lo, hi, lo) records -> fp64 [2][C][2] = per group and channel (sum dy, sum dy * xhat)"""
    r = rec4.double().cpu()
    r = r.view(2, r.shape[0] // 2, r.shape[1], 4)
    return torch.stack([(r[..., 0] + r[..., 1]).sum(1), (r[..., 2] + r[..., 3]).sum(1)], dim=-1)


def _host_fp64(g, L, z, save):
    """fp64 on the host from the fp32 inputs: per group and channel (sum dy, sum dy xhat), their sums of magnitudes (the scale a
    summation error is measured against) and max |g L|; dy = g L where relu(bn(z)) > 0 (the kernels' fp32 decision)."""
    B2, C, H, W = L.shape
    B = B2 // 2
    g, L, z, save = g.cpu(), L.cpu(), z.cpu(), save.cpu()
    sums, mags = torch.zeros(2, C, 2, dtype=torch.float64), torch.zeros(2, C, 2, dtype=torch.float64)
    amax = 0.0
    for grp in range(2):
        gd = g[grp * B:(grp + 1) * B, 0].double()
        for c in range(C):
            zc, lc = z[grp * B:(grp + 1) * B, c], L[grp * B:(grp + 1) * B, c]
            mean, invstd, sc, sh = (save[grp, k, c] for k in range(4))
            # the kernels' fp32 decision fma(z - mean, scale, shift) > 0: the product is exact in fp64, the sum keeps its sign
            on = ((zc - mean).double() * sc.double() + sh.double()).float() > 0
            da = gd * lc.double()
            amax = max(amax, float(da.abs().max()))
            dy = torch.where(on, da, torch.zeros_like(da))
            xh = (zc.double() - mean.double()) * invstd.double()
            sums[grp, c, 0], sums[grp, c, 1] = dy.sum(), (dy * xh).sum()
            mags[grp, c, 0], mags[grp, c, 1] = dy.abs().sum(), (dy * xh).abs().sum()
    return sums, mags, amax


CASES = [(64, 64, 256, 256, "all"),       # the benchmark's last unit: 64 images, 64 channels, 256 x 256
         (6, 16, 20, 36, "all"),          # odd groups of 3; H W = 720: less than one block's pixel chunk (tail loops only)
         (2, 8, 132, 128, "all"),         # H W = 16896: two reduce chunks of 8448 = 2 x 4096 + 256 (main loop + tail), 16.5 apply blocks
         (6, 16, 20, 36, "partial")]      # partial graph: no gradient through Vt, nor through the down half's channel sums


@pytest.mark.parametrize("B2,C,H,W,graph", CASES)
def test_fused_head_backward_kernels(dev, B2, C, H, W, graph):
    """dL bit for bit; records and max |da| against fp64 on the host, the fused kernel held to twice the error of
    bn_relu_bwd_reduce_kernel fed the materialised dH (both sum in fp64: the factor covers another summation order and nothing
    more); dz slots of the on-load apply pass bit for bit against the pass fed dH = fl(g L).
    Measured (MI355X): see profiles/r06_head_bwd_fuse.md -- the records come out bit-identical (same partition, same order)."""
    from onet_amd import ops
    if B2 * C * H * W * 4 * 8 > torch.cuda.mem_get_info(dev)[0]:
        pytest.skip("not enough free HBM for this shape")
    L, z, save, S, dVt, dVd, dS, gst, gsd = _inputs(B2, C, H, W, dev, seed=B2 * 1000 + H)
    if graph == "partial":
        dVt, gsd = None, None
    B = B2 // 2
    # ---- unfused: head backward writes dH, the reduce pass sums it
    dL0, dH0 = ops.head_softmax_bwd(dVt, dVd, dS, S, L[:B], z[:B], L[B:], z[B:], twin=True, gsums=(gst, gsd), h_norm=(save[0], save[1]))
    amax0 = ops.new_amax(dev)
    np_g = ops._bn_nparts(B, H * W)
    rec0 = torch.empty((2 * np_g, C, 4), dtype=torch.float32, device=dev)
    from onet_amd import _lib
    _lib.call("onet_bn_relu_bwd_reduce", dH0.data_ptr(), C * H * W, z.data_ptr(), 0, C * H * W, save.data_ptr(), rec0.data_ptr(), 2 * np_g,
              amax0.data_ptr(), B, B2, C, H * W, torch.cuda.current_stream().cuda_stream)
    # ---- fused
    g = ops.head_grad_map(dVt, dVd, dS, S)
    assert ops.head_bwd_fuse_ok(L, z)
    dL1, rec1, amax1 = ops.head_bwd_reduce(g, (gst, gsd), L, z, save)
    torch.cuda.synchronize()
    assert rec1.shape == rec0.shape
    # dL: the same bits; the materialised dH is fl(g L)
    assert torch.equal(dL0.view(torch.int32), dL1.view(torch.int32))
    assert torch.equal(dH0.view(torch.int32), (g * L).view(torch.int32))
    # records against fp64
    ref, mag, amax_ref = _host_fp64(g, L, z, save)
    s0, s1 = _record_sums(rec0), _record_sums(rec1)
    err0 = float(((s0 - ref).abs() / mag).max())
    err1 = float(((s1 - ref).abs() / mag).max())
    same = torch.equal(rec0.view(torch.int32), rec1.view(torch.int32))
    print(f"[{B2}x{C}x{H}x{W} {graph}] records vs fp64 (|error| / sum of magnitudes, worst channel): unfused reduce {err0:.3e}, "
          f"fused {err1:.3e}; records bit-identical: {same}; max|da| unfused {_amax_value(amax0):.9e} fused {_amax_value(amax1):.9e} "
          f"fp64 {amax_ref:.9e}")
    assert err1 <= 2.0 * err0, (err1, err0)
    # max |da|: the fp32 maximum of the rounded products = the rounded fp64 maximum (rounding is monotone)
    assert _amax_value(amax1) == _amax_value(amax0) == float(np.float32(amax_ref))
    # ---- apply pass: da formed on load against the pass fed the stored dH (same records, same magnitude slots)
    dz0, sl0, dg0, db0 = ops.bn_relu_bwd_split(dH0, z, save, True, rec4=rec0, da_amax=amax0)
    ph = ops.fp32_placeholder(z.shape, dev)
    dz1, sl1, dg1, db1 = ops.bn_relu_bwd_split(ph, z, save, True, rec4=rec0, da_amax=amax0, da_gl=(g, L))
    torch.cuda.synchronize()
    assert torch.equal(sl0, sl1) and torch.equal(dg0, dg1) and torch.equal(db0, db1)
    assert torch.equal(dz0.view(torch.int16), dz1.view(torch.int16))
    # (decoded: hi + mid parts of 2^k dz, the same k for both)
    assert torch.equal(dz0.float().sum(dim=3), dz1.float().sum(dim=3))
    # the placeholder is never read: without the (g, L) hand-off it is refused
    with pytest.raises(RuntimeError, match="placeholder"):
        ops.bn_relu_bwd_split(ph, z, save, True, rec4=rec0, da_amax=amax0)


def _fresh_model(dev):
    import Onet_vanilla_20240606 as ov
    m = ov.Onet(in_chns=1, binit=True, bshare=True)
    m.load_state_dict(orc.onet_state_dict(1, 1981, True, head_gain=0.3))
    return m.to(dev).train()


def _step(m, X, retain=False):
    m.zero_grad()
    Lt, Vt, Ld, Vd, S = m(X)
    loss = m.compute_loss(Lt, S[:, 0].unsqueeze(1), Ld, S[:, 1].unsqueeze(1))
    loss.backward(retain_graph=retain)
    return loss


def _count(monkeypatch, ops, name, box):
    real = getattr(ops, name)

    def spy(*a, **k):
        box[name] = box.get(name, 0) + 1
        return real(*a, **k)

    monkeypatch.setattr(ops, name, spy)


def test_whole_step_fused_vs_unfused(dev, monkeypatch):
    """One training step from the same state with the switch on, on again, and off: the two fused runs agree bit for bit; fused
    against unfused within test_presplit_storage_step_vs_fp32_storage's bounds for a changed summation order (loss 1e-6, worst
    parameter gradient 2e-2 relative) -- measured: bit-identical too, the fused kernels keep the unfused passes' order."""
    from onet_amd import ops
    X = orc.det_input(4, 1, 128, 128, seed=23).to(dev)
    used = {}
    for name in ("head_bwd_reduce", "head_softmax_bwd"):
        _count(monkeypatch, ops, name, used)
    res = []
    for fuse in (True, True, False):
        monkeypatch.setattr(ops, "HEAD_BWD_FUSE", fuse)
        used.clear()
        m = _fresh_model(dev)
        loss = _step(m, X)
        assert used == ({"head_bwd_reduce": 1} if fuse else {"head_softmax_bwd": 1}), used
        res.append((loss.detach().clone(), {k: p.grad.detach().clone() for k, p in m.named_parameters()}))
    (l0, g0), (l1, g1), (l2, g2) = res
    assert torch.equal(l0, l1) and all(torch.equal(g0[k].view(torch.int32), g1[k].view(torch.int32)) for k in g0)
    assert abs(float(l0) - float(l2)) <= 1e-6 * abs(float(l2))
    worst = max((float((g0[k] - g2[k]).norm() / g2[k].norm()), k) for k in g0)
    nbit = sum(torch.equal(g0[k], g2[k]) for k in g0)
    print(f"fused vs unfused step: loss {float(l0):.9g} / {float(l2):.9g}; worst relative gradient difference {worst[0]:.2e} ({worst[1]}); "
          f"{nbit} of {len(g0)} parameter gradients bit-identical")
    assert worst[0] <= 2e-2, worst


def test_second_backward_through_a_retained_graph_makes_the_hand_off_again(dev, monkeypatch):
    from onet_amd import ops
    used = {}
    _count(monkeypatch, ops, "head_bwd_reduce", used)
    X = orc.det_input(4, 1, 128, 128, seed=29).to(dev)
    m = _fresh_model(dev)
    m.zero_grad()
    Lt, Vt, Ld, Vd, S = m(X)
    loss = m.compute_loss(Lt, S[:, 0].unsqueeze(1), Ld, S[:, 1].unsqueeze(1))
    loss.backward(retain_graph=True)
    first = {k: p.grad.detach().clone() for k, p in m.named_parameters()}
    m.zero_grad()
    loss.backward()
    assert used == {"head_bwd_reduce": 2}, used
    for k, p in m.named_parameters():
        assert torch.equal(first[k].view(torch.int32), p.grad.view(torch.int32)), k


def test_unit_refuses_a_gradient_that_is_not_the_heads_placeholder(dev):
    """The last unit's da exists only as (g, L) after a fused head backward: handed anything but the head's placeholder, the unit
    raises -- it never reads a placeholder and never silently drops the hand-off; the hand-off is taken once."""
    from onet_amd import ops
    from onet_amd import functional as Fn
    from onet_amd.handoff import HeadLink
    shape = (2, 8, 4, 4)
    ph = ops.fp32_placeholder(shape, dev)
    take = Fn.ConvBNReLUFn._take_head_handoff

    def link():
        lk = HeadLink()
        lk.grad.publish(ph, rec4="records", da_amax=None, gl=("g", "L"))
        return lk

    got = take(link(), ops.fp32_placeholder(shape, dev))
    assert (got.rec4, got.da_amax, got.gl) == ("records", None, ("g", "L"))
    with pytest.raises(RuntimeError, match="another tensor"):
        take(link(), torch.ones(shape, device=dev))
    with pytest.raises(RuntimeError, match="another tensor"):
        take(link(), ops.fp32_placeholder((2, 8, 4, 8), dev))
    taken = link()
    take(taken, ph)
    assert taken.grad.gl is None and take(taken, ph) is None
    assert take(None, ph) is None
