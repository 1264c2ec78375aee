"""The ragged entry points of include/onet_hip_ragged.h: the one-part (plain bf16) eval launches on maps that are not made of full
16 x 32 tiles, and the slot-operand ConvTranspose2d forward on maps with h w % 128 != 0.

Reference of every convolution case: the EXISTING full-tile entry point on a zero-padded canvas -- the map in the top-left corner of the
smallest map made of full tiles that holds it, zero slots everywhere else.  A border tap of the ragged launch is a bounds-checked load
that returns zero, the canvas launch reads a zero slot there, and the chunk order is the same: the valid region must be EQUAL, value
for value (`==`: -0 = +0), no tolerance.  ConvTranspose2d: the existing kernel on the map with zero rows appended until
h' w % 128 == 0 (pixels are independent columns of the GEMM).

Every output is a slice of a larger buffer pre-filled with a sentinel bit pattern, with a batch stride above dense (an extra channel
group / two extra channels per image); the sentinel must be intact outside the slice, which a stray store past a row, a map or an image
would break -- nothing is provoked.  V, whose entry takes no batch stride, is a dense slice out of the middle of a sentinel buffer."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B = 2
S16 = 0x7FC5            # bf16 NaN with a payload: no launch of these tests writes it
S32 = 0x7FC12345        # fp32 likewise


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


def canvas_of(H, W):
    return -(-H // 16) * 16, max(32, -(-W // 32) * 32)


def slots_out(C, H, W, dev, batch=B):
    """-> (the [batch, C/8, H, 1, W, 8] slice to write, the whole sentinel buffer: one channel group more per image)"""
    big = torch.full((batch, C // 8 + 1, H, 1, W, 8), S16, dtype=torch.int16, device=dev).view(torch.bfloat16)
    return big[:, :C // 8], big


def f32_out(C, H, W, dev, batch=B):
    """-> (the [batch, C, H, W] slice to write, the whole sentinel buffer: two channels more per image)"""
    big = torch.full((batch, C + 2, H, W), S32, dtype=torch.int32, device=dev).view(torch.float32)
    return big[:, :C], big


def gap_intact(big, C_valid):
    """the channels (channel groups) of `big` behind the written slice still hold the sentinel"""
    rest = big[:, C_valid:]
    if big.dtype == torch.bfloat16:
        return bool((rest.contiguous().view(torch.int16) == S16).all())
    return bool((rest.contiguous().view(torch.int32) == S32).all())


def all_sentinel(big):
    return gap_intact(big, 0)


def same(got, ref):
    """value for value: == on every element (finite values: -0 = +0), nothing left of the sentinel"""
    got, ref = got.float(), ref.float()
    return bool(torch.isfinite(got).all()) and bool(torch.isfinite(ref).all()) and bool((got == ref).all())


_CASES = {}


def conv_case(dev, Cin, Cout, H, W):
    """operands of one convolution case on the map and on its canvas, computed once"""
    from onet_amd import ops
    key = (Cin, Cout, H, W)
    if key not in _CASES:
        Hc, Wc = canvas_of(H, W)
        x = rnd(B, Cin, H, W, seed=700).to(torch.bfloat16).float()
        xc = torch.zeros(B, Cin, Hc, Wc)
        xc[:, :, :H, :W] = x
        w = rnd(Cout, Cin, 3, 3, seed=701, scale=(2.0 / (Cin * 9)) ** 0.5)
        gamma = (rnd(Cout, seed=702).abs() + 0.5) * torch.where(rnd(Cout, seed=703) > 0.5, -1.0, 1.0)
        save = ops.bn_eval_coeffs(gamma.to(dev), rnd(Cout, seed=704, scale=0.3).to(dev), rnd(Cout, seed=705, scale=0.1).to(dev),
                                  (rnd(Cout, seed=706) ** 2 + 0.5).to(dev), 1e-5)
        _CASES[key] = dict(P=ops.split_pack_act(x.to(dev), parts=1), Pc=ops.split_pack_act(xc.to(dev), parts=1),
                           wq=ops.pack3x3_plain16(w.to(dev))[0], save=save, Hc=Hc, Wc=Wc)
    return _CASES[key]


# ----------------------------------------------------------------------------------------------------------------- act
@pytest.mark.parametrize("Cin,Cout,H,W", [(32, 64, 24, 40), (32, 64, 28, 28), (32, 64, 18, 36), (32, 64, 2, 4), (96, 128, 24, 40)],
                         ids=["24x40", "28x28", "18x36", "2x4", "96to128-24x40"])
def test_act_ragged_equals_the_canvas(dev, Cin, Cout, H, W):
    """slots and the optional fp32 activation == the full-tile entry on the zero-padded canvas; 96 -> 128: three chunks, two channel tiles"""
    from onet_amd import ops
    c = conv_case(dev, Cin, Cout, H, W)
    aPc = ops.conv3x3_plain16_pre_act(c["Pc"], c["wq"], Cout, c["save"])
    ac = torch.empty((B, Cout, c["Hc"], c["Wc"]), device=dev)
    assert ops.conv3x3_plain16_pre_act(c["Pc"], c["wq"], Cout, c["save"], a=ac) is not None and aPc is not None
    aP, bigP = slots_out(Cout, H, W, dev)
    a, bigA = f32_out(Cout, H, W, dev)
    assert ops.conv3x3_plain16_pre_act_ragged(c["P"], c["wq"], Cout, c["save"], out=aP, a=a) is aP
    torch.cuda.synchronize()
    assert bool((ac[:, :, :H, :W] > 0).any()) and bool((ac[:, :, :H, :W] == 0).any())
    assert same(aP, aPc[:, :, :H, :, :W]), "slots differ from the canvas"
    assert same(a, ac[:, :, :H, :W]), "fp32 activation differs from the canvas"
    assert gap_intact(bigP, Cout // 8) and gap_intact(bigA, Cout), "a store left the map"
    # without the optional fp32 tensor: the same slots
    aP2, bigP2 = slots_out(Cout, H, W, dev)
    assert ops.conv3x3_plain16_pre_act_ragged(c["P"], c["wq"], Cout, c["save"], out=aP2) is aP2
    torch.cuda.synchronize()
    assert torch.equal(aP2.contiguous().view(torch.int16), aP.contiguous().view(torch.int16)) and gap_intact(bigP2, Cout // 8)


def test_act_ragged_on_full_tiles_is_the_full_tile_entry(dev):
    """(16, 32): the ragged entry launches what its sibling launches -- the same bits"""
    from onet_amd import ops
    c = conv_case(dev, 32, 64, 16, 32)
    ref = ops.conv3x3_plain16_pre_act(c["P"], c["wq"], 64, c["save"])
    a_ref = torch.empty((B, 64, 16, 32), device=dev)
    ops.conv3x3_plain16_pre_act(c["P"], c["wq"], 64, c["save"], a=a_ref)
    aP, bigP = slots_out(64, 16, 32, dev)
    a, bigA = f32_out(64, 16, 32, dev)
    assert ops.conv3x3_plain16_pre_act_ragged(c["P"], c["wq"], 64, c["save"], out=aP, a=a) is aP
    torch.cuda.synchronize()
    assert torch.equal(aP.contiguous().view(torch.int16), ref.view(torch.int16))
    assert torch.equal(a.contiguous().view(torch.int32), a_ref.view(torch.int32))
    assert gap_intact(bigP, 8) and gap_intact(bigA, 64)


# ----------------------------------------------------------------------------------------------------------------- act_pool
@pytest.mark.parametrize("H,W", [(24, 40), (28, 28), (12, 20)], ids=["24x40", "28x28", "12x20"])
def test_act_pool_ragged_equals_the_canvas(dev, H, W):
    """skip slots, fp32 L, pooled slots and pooled fp32 (rows of 20, 14, 10 floats) == the full-tile entry on the canvas"""
    from onet_amd import ops
    Cin, Cout = 32, 64
    c = conv_case(dev, Cin, Cout, H, W)
    Hc, Wc = c["Hc"], c["Wc"]
    Lc = torch.empty((B, Cout, Hc, Wc), device=dev)
    yPc = torch.empty((B, Cout // 8, Hc // 2, 1, Wc // 2, 8), dtype=torch.bfloat16, device=dev)
    yc = torch.empty((B, Cout, Hc // 2, Wc // 2), device=dev)
    aPc = ops.conv3x3_plain16_pre_act_pool(c["Pc"], c["wq"], Cout, c["save"], a=Lc, yP=yPc, y=yc)
    assert aPc is not None
    aP, bigP = slots_out(Cout, H, W, dev)
    L, bigL = f32_out(Cout, H, W, dev)
    yP, bigyP = slots_out(Cout, H // 2, W // 2, dev)
    y, bigy = f32_out(Cout, H // 2, W // 2, dev)
    assert ops.conv3x3_plain16_pre_act_pool_ragged(c["P"], c["wq"], Cout, c["save"], out=aP, a=L, yP=yP, y=y) is aP
    torch.cuda.synchronize()
    assert same(aP, aPc[:, :, :H, :, :W]), "skip slots"
    assert same(L, Lc[:, :, :H, :W]), "fp32 L"
    assert same(yP, yPc[:, :, :H // 2, :, :W // 2]), "pooled slots"
    assert same(y, yc[:, :, :H // 2, :W // 2]), "pooled fp32"
    assert bool((y > 0).any())
    assert gap_intact(bigP, Cout // 8) and gap_intact(bigL, Cout) and gap_intact(bigyP, Cout // 8) and gap_intact(bigy, Cout)
    # one pooled destination at a time: the same values
    for kw in (dict(yP=True), dict(y=True)):
        yP2, bigyP2 = slots_out(Cout, H // 2, W // 2, dev)
        y2, bigy2 = f32_out(Cout, H // 2, W // 2, dev)
        aP2, bigP2 = slots_out(Cout, H, W, dev)
        assert ops.conv3x3_plain16_pre_act_pool_ragged(c["P"], c["wq"], Cout, c["save"], out=aP2, yP=yP2 if "yP" in kw else None,
                                                       y=y2 if "y" in kw else None) is aP2
        torch.cuda.synchronize()
        assert same(aP2, aP) and gap_intact(bigP2, Cout // 8)
        if "yP" in kw:
            assert same(yP2, yP) and gap_intact(bigyP2, Cout // 8) and all_sentinel(bigy2)
        else:
            assert same(y2, y) and gap_intact(bigy2, Cout) and all_sentinel(bigyP2)


# ----------------------------------------------------------------------------------------------------------------- head, plain
@pytest.mark.parametrize("H,W", [(24, 40), (28, 28)], ids=["24x40", "28x28"])
def test_head_ragged_equals_the_canvas(dev, H, W):
    """V == the canvas V on the map; L is read from a batch-strided slice; V (no batch stride in the ABI) is a dense slice out of the
    middle of a sentinel buffer"""
    from onet_amd import ops
    Cin = Cout = 64
    c = conv_case(dev, Cin, Cout, H, W)
    Hc, Wc = c["Hc"], c["Wc"]
    Lh = rnd(B, Cout, H, W, seed=720).abs()
    Lc = torch.zeros(B, Cout, Hc, Wc)
    Lc[:, :, :H, :W] = Lh
    Vc = ops.conv3x3_plain16_pre_head(c["Pc"], c["wq"], Cout, c["save"], Lc.to(dev))
    assert Vc is not None
    L, _ = f32_out(Cout, H, W, dev)
    L.copy_(Lh.to(dev))
    n = B * H * W
    flat = torch.full((3 * n,), S32, dtype=torch.int32, device=dev).view(torch.float32)
    V = flat[n:2 * n].view(B, 1, H, W)
    assert ops.conv3x3_plain16_pre_head_ragged(c["P"], c["wq"], Cout, c["save"], L, out=V) is V
    torch.cuda.synchronize()
    assert same(V, Vc[:, :, :H, :W]) and bool((V != 0).any())
    assert bool((flat[:n].view(torch.int32) == S32).all()) and bool((flat[2 * n:].view(torch.int32) == S32).all())


def test_plain_ragged_equals_the_canvas(dev):
    from onet_amd import ops
    Cin, Cout, H, W = 32, 64, 24, 40
    c = conv_case(dev, Cin, Cout, H, W)
    zc = ops.conv3x3_split_pre(c["Pc"], c["wq"], Cout)
    z, bigz = f32_out(Cout, H, W, dev)
    assert ops.conv3x3_plain16_pre_plain_ragged(c["P"], c["wq"], Cout, out=z) is z
    torch.cuda.synchronize()
    assert same(z, zc[:, :, :H, :W]) and bool((z != 0).any()) and gap_intact(bigz, Cout)


# ----------------------------------------------------------------------------------------------------------------- ConvTranspose2d
def _convt_case(dev, Cin, Ct, h, w, batch):
    from onet_amd import ops
    x = rnd(batch, Cin, h, w, seed=740).to(torch.bfloat16).float()
    wt = rnd(Cin, Ct, 2, 2, seed=741, scale=(1.0 / Cin) ** 0.5)
    bias = rnd(Ct, seed=742, scale=0.2).to(dev)
    wP = ops.packT2x2_slots(wt.to(dev), parts=1)
    wP = wP[0] if isinstance(wP, tuple) else wP
    return x, wP, bias


@pytest.mark.parametrize("Cin,Ct,h,w,batch", [(128, 64, 12, 20, B), (128, 64, 14, 14, B), (128, 64, 5, 6, B), (256, 128, 14, 14, 3)],
                         ids=["12x20", "14x14", "5x6", "256to128-14x14-b3"])
def test_convt_ragged_equals_the_zero_extended_map(dev, Cin, Ct, h, w, batch):
    """the up-sampled slots == the existing kernel on (h', w), zero rows appended until h' w % 128 == 0.  Batch 3 at 14 x 14: 196
    pixels per image, so an image boundary falls inside a 128-pixel tile of the existing kernel's global pixel index -- the ragged
    kernel counts its tiles per image"""
    from onet_amd import ops
    x, wP, bias = _convt_case(dev, Cin, Ct, h, w, batch)
    hc = next(v for v in range(h, h + 129) if (v * w) % 128 == 0)
    assert (h * w) % 128 and hc > h
    xc = torch.zeros(batch, Cin, hc, w)
    xc[:, :, :h] = x
    P, Pc = ops.split_pack_act(x.to(dev), parts=1), ops.split_pack_act(xc.to(dev), parts=1)
    outc = torch.empty((batch, Ct // 8, 2 * hc, 1, 2 * w, 8), dtype=torch.bfloat16, device=dev)
    assert ops.convT2x2_fwd_slots(Pc, wP, bias, outc, Ct, kind="convt_slot_fwd_kernel")
    out, big = slots_out(Ct, 2 * h, 2 * w, dev, batch)
    assert ops.convT2x2_fwd_slots_ragged(P, wP, bias, out, Ct)
    torch.cuda.synchronize()
    assert same(out, outc[:, :, :2 * h]) and bool((out.float() != 0).any())
    assert gap_intact(big, Ct // 8), "a store left the map"


def test_convt_ragged_on_whole_tiles_is_the_existing_entry(dev):
    """(8, 16) = 128 pixels: bit for bit the existing entry point"""
    from onet_amd import ops
    Cin, Ct, h, w = 128, 64, 8, 16
    x, wP, bias = _convt_case(dev, Cin, Ct, h, w, B)
    P = ops.split_pack_act(x.to(dev), parts=1)
    ref = torch.empty((B, Ct // 8, 2 * h, 1, 2 * w, 8), dtype=torch.bfloat16, device=dev)
    assert ops.convT2x2_fwd_slots(P, wP, bias, ref, Ct, kind="convt_slot_fwd_kernel")
    out, big = slots_out(Ct, 2 * h, 2 * w, dev)
    assert ops.convT2x2_fwd_slots_ragged(P, wP, bias, out, Ct)
    torch.cuda.synchronize()
    assert torch.equal(out.contiguous().view(torch.int16), ref.view(torch.int16)) and gap_intact(big, Ct // 8)


# ----------------------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("Cin,H,W", [(32, 23, 40), (32, 24, 38), (48, 24, 40)], ids=["odd-H", "W%4", "Cin%32"])
def test_ragged_convolution_entries_refuse(dev, Cin, H, W):
    """odd H, W % 4 != 0, Cin % 32 != 0: every ragged convolution entry answers "not taken" (1 from the library, None from the wrapper)
    and writes nothing"""
    from onet_amd import ops, _lib
    Cout = 64
    P = ops.split_pack_act(rnd(B, Cin, H, W, seed=760).to(dev), parts=1)
    wq = torch.zeros(Cin * 9 * Cout + 8, dtype=torch.bfloat16, device=dev) if Cin % 32 else \
        ops.pack3x3_plain16(rnd(Cout, Cin, 3, 3, seed=761, scale=0.1).to(dev))[0]
    save = ops.bn_eval_coeffs(torch.ones(Cout, device=dev), torch.zeros(Cout, device=dev), torch.zeros(Cout, device=dev),
                              torch.ones(Cout, device=dev), 1e-5)
    Hp, Wp = max(H // 2, 1), max(W // 2, 1)
    aP, bigP = slots_out(Cout, H, W, dev)
    a, bigA = f32_out(Cout, H, W, dev)
    yP, bigyP = slots_out(Cout, Hp, Wp, dev)
    y, bigy = f32_out(Cout, Hp, Wp, dev)
    V = torch.full((B, 1, H, W), S32, dtype=torch.int32, device=dev).view(torch.float32)
    L = torch.ones((B, Cout, H, W), device=dev)
    st = torch.cuda.current_stream().cuda_stream
    rc = _lib.load().onet_conv3x3_plain16_fwd_pre_act_ragged(P.data_ptr(), Cin * H * W // 2, wq.data_ptr(), save.data_ptr(), aP.data_ptr(),
                                                             aP.stride(0) // 2, None, a.data_ptr(), a.stride(0), B, Cin, Cout, H, W, st)
    assert rc == 1
    assert ops.conv3x3_plain16_pre_act_ragged(P, wq, Cout, save, out=aP, a=a) is None
    assert ops.conv3x3_plain16_pre_act_pool_ragged(P, wq, Cout, save, out=aP, a=a, yP=yP, y=y) is None
    assert ops.conv3x3_plain16_pre_plain_ragged(P, wq, Cout, out=a) is None
    assert ops.conv3x3_plain16_pre_head_ragged(P, wq, Cout, save, L, out=V) is None
    torch.cuda.synchronize()
    assert all_sentinel(bigP) and all_sentinel(bigA) and all_sentinel(bigyP) and all_sentinel(bigy)
    assert bool((V.view(torch.int32) == S32).all())


@pytest.mark.parametrize("Cin,h,w", [(128, 6, 5), (144, 6, 6), (96, 6, 6)], ids=["odd-w", "Cin%32", "Cin<128"])
def test_convt_ragged_refuses(dev, Cin, h, w):
    """the ConvTranspose2d entry's own domain (onet_convT2x2_fwd_slots' without h w % 128): odd w, Cin % 32 != 0, Cin < 128 -> not
    taken, nothing written"""
    from onet_amd import ops
    Ct = 64
    P = ops.split_pack_act(rnd(B, Cin, h, w, seed=770).to(dev), parts=1)
    wP = torch.zeros(Cin * 4 * Ct + 64, dtype=torch.bfloat16, device=dev)
    out, big = slots_out(Ct, 2 * h, 2 * w, dev)
    assert not ops.convT2x2_fwd_slots_ragged(P, wP, torch.zeros(Ct, device=dev), out, Ct)
    torch.cuda.synchronize()
    assert all_sentinel(big)
