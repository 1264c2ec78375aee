"""The ragged entry points of include/onet_hip_ragged_split.h: the fp16 (hi | mid) eval launches on maps that are not made of full
16 x 32 tiles, and the two-part slot-operand ConvTranspose2d forward on maps with h w % 128 != 0.

The method of tests/test_gpu_ragged_kernels.py.  Reference of every convolution case: the EXISTING full-tile entry point on a zero-padded
canvas -- the map in the top-left corner of the smallest map made of full tiles that holds it, zero slots everywhere else -- given the
SAME magnitude slots (operand and output bound).  A border tap of the ragged launch is a bounds-checked load that returns zero, the
canvas launch reads a zero slot there, and the chunk order is the same: the valid region must be EQUAL, value for value (`==`), no
tolerance.  ConvTranspose2d: the existing kernel on the map with zero rows appended until h' w % 128 == 0.

Every output is a slice of a larger buffer pre-filled with a sentinel bit pattern, with a batch stride above dense; the sentinel must be
intact outside the slice -- nothing is provoked.

The exact-maximum record is what these entries add to the one-part ones: it must be the maximum over the MAP's pixels, bit-equal to the
maximum of the fp32 activation of the same launch, also where an out-of-map accumulator of the same tile is larger."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B = 2
S16 = 0x7E05            # fp16 NaN with a payload: no launch of these tests writes it
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
    """-> (the [batch, C/8, H, 2, W, 8] slice to write, the whole sentinel buffer: one channel group more per image)"""
    big = torch.full((batch, C // 8 + 1, H, 2, W, 8), S16, dtype=torch.int16, device=dev).view(torch.float16)
    return big[:, :C // 8], big


def f32_out(C, H, W, dev, batch=B):
    """-> (the [batch, C, H, W] slice to write, the whole sentinel buffer: two channels more per image)"""
    big = torch.full((batch, C + 2, H, W), S32, dtype=torch.int32, device=dev).view(torch.float32)
    return big[:, :C], big


def gap_intact(big, C_valid):
    """the channels (channel groups) of `big` behind the written slice still hold the sentinel"""
    rest = big[:, C_valid:]
    if big.dtype == torch.float16:
        return bool((rest.contiguous().view(torch.int16) == S16).all())
    return bool((rest.contiguous().view(torch.int32) == S32).all())


def all_sentinel(big):
    return gap_intact(big, 0)


def same(got, ref):
    """value for value: == on every element (finite values: -0 = +0), nothing left of the sentinel"""
    got, ref = got.float(), ref.float()
    return bool(torch.isfinite(got).all()) and bool(torch.isfinite(ref).all()) and bool((got == ref).all())


def amax_slots(dev):
    from onet_amd import ops
    return torch.zeros(ops.AMAX_SLOTS, dtype=torch.int32, device=dev)


def slot_max(slots):
    return float(slots.view(torch.float32).max())


def pack(w):
    from onet_amd import ops
    with ops.using(ops.Settings(conv="auto", split_f16=True)):
        qf, _ = ops.pack3x3_split(w)
    assert qf.dtype == torch.float16
    return qf


def save_of(Cout, seed, dev, gain=1.0):
    """[4][Cout] coefficients in bn_eval_coeffs' format (mean, invstd, sc, sh): about half of relu's inputs negative, a few negative
    BatchNorm weights (tests/test_gpu_fused_eval.py: _save)"""
    mean, sc, sh = rnd(Cout, seed=seed, scale=0.1), rnd(Cout, seed=seed + 1).abs() + 0.5, rnd(Cout, seed=seed + 2, scale=0.3)
    sc = sc * torch.where(rnd(Cout, seed=seed + 3) > 1.0, -1.0, 1.0)
    return torch.stack([mean, torch.ones(Cout), sc * gain, sh * gain]).contiguous().to(dev)


_CASES = {}


def conv_case(dev, Cin, Cout, H, W, mode="one"):
    """operands of one convolution case on the map and on its canvas, computed once.  mode "one": one producer; "two": a concat input
    of two producers (split_ch = 64: the first at 1e5 -- its guard exponent is non-zero -- the second at 1e-1); "guard": coefficients
    scaled so that the OUTPUT's bound reaches 2^15 (non-zero guard exponent of the slots written)"""
    from onet_amd import ops
    key = (Cin, Cout, H, W, mode)
    if key in _CASES:
        return _CASES[key]
    Hc, Wc = canvas_of(H, W)
    x = rnd(B, Cin, H, W, seed=800)
    sc = 64 if mode == "two" else 0
    if sc:
        x[:, :sc] *= 1e5
        x[:, sc:] *= 1e-1
    xc = torch.zeros(B, Cin, Hc, Wc)
    xc[:, :, :H, :W] = x
    x, xc = x.to(dev), xc.to(dev)
    P = torch.empty((B, Cin // 8, H, 2, W, 8), dtype=torch.float16, device=dev)
    Pc = torch.empty((B, Cin // 8, Hc, 2, Wc, 8), dtype=torch.float16, device=dev)
    if sc:
        s1, s2 = ops.absmax_slots(x[:, :sc]), ops.absmax_slots(x[:, sc:])
        for p, t in ((P, x), (Pc, xc)):
            ops.split_pack_act(t[:, :sc], f16=True, slots=s1, out=p[:, :sc // 8])
            ops.split_pack_act(t[:, sc:], f16=True, slots=s2, out=p[:, sc // 8:])
    else:
        s1, s2 = ops.absmax_slots(x), None
        ops.split_pack_act(x, f16=True, slots=s1, out=P)
        ops.split_pack_act(xc, f16=True, slots=s1, out=Pc)
    w = rnd(Cout, Cin, 3, 3, seed=801, scale=(2.0 / (Cin * 9)) ** 0.5).to(dev)
    save = save_of(Cout, 802, dev, gain={"one": 1.0, "two": 1e-4, "guard": 3.0e4}[mode])
    scale = ops.conv3x3_act_bound(w, save, s1, s2, sc)
    if mode == "guard":
        assert slot_max(scale) >= 2.0 ** 15
    if mode == "two":
        assert slot_max(s1) >= 2.0 ** 15
    _CASES[key] = dict(P=P, Pc=Pc, wq=pack(w), w=w, save=save, scale=scale, kw=dict(slots=s1, slots2=s2, split_ch=sc), Hc=Hc, Wc=Wc)
    return _CASES[key]


ACT_CASES = [(32, 64, 24, 40, "one"), (32, 64, 28, 28, "guard"), (32, 64, 18, 36, "one"), (32, 64, 2, 4, "one"), (96, 128, 24, 40, "two")]
ACT_IDS = ["24x40", "28x28-guard", "18x36", "2x4", "96to128-24x40-two-producers"]


# ----------------------------------------------------------------------------------------------------------------- act
@pytest.mark.parametrize("Cin,Cout,H,W,mode", ACT_CASES, ids=ACT_IDS)
def test_act_ragged_equals_the_canvas(dev, Cin, Cout, H, W, mode):
    """slots and the optional fp32 activation == the full-tile entry on the zero-padded canvas; the record == max of the map's own a.
    96 -> 128: six chunks, two channel tiles, two producers' slot sets; 28 x 28: a non-zero guard exponent of the output"""
    from onet_amd import ops
    c = conv_case(dev, Cin, Cout, H, W, mode)
    ac = torch.empty((B, Cout, c["Hc"], c["Wc"]), device=dev)
    aPc = ops.conv3x3_split_pre_act(c["Pc"], c["wq"], Cout, c["save"], c["scale"], a=ac, **c["kw"])
    assert aPc is not None
    aP, bigP = slots_out(Cout, H, W, dev)
    a, bigA = f32_out(Cout, H, W, dev)
    am = amax_slots(dev)
    assert ops.conv3x3_split_pre_act_ragged(c["P"], c["wq"], Cout, c["save"], c["scale"], out=aP, a_amax=am, a=a, **c["kw"]) is aP
    torch.cuda.synchronize()
    assert bool((ac[:, :, :H, :W] > 0).any()) and bool((ac[:, :, :H, :W] == 0).any())
    assert same(aP, aPc[:, :, :H, :, :W]), "slots differ from the canvas"
    assert same(a, ac[:, :, :H, :W]), "fp32 activation differs from the canvas"
    assert gap_intact(bigP, Cout // 8) and gap_intact(bigA, Cout), "a store left the map"
    assert slot_max(am) == float(a.max()), (slot_max(am), float(a.max()))
    # without the optional fp32 tensor and the record: the same slots
    aP2, bigP2 = slots_out(Cout, H, W, dev)
    assert ops.conv3x3_split_pre_act_ragged(c["P"], c["wq"], Cout, c["save"], c["scale"], out=aP2, **c["kw"]) is aP2
    torch.cuda.synchronize()
    assert torch.equal(aP2.contiguous().view(torch.int16), aP.contiguous().view(torch.int16)) and gap_intact(bigP2, Cout // 8)


# ----------------------------------------------------------------------------------------------------------------- act_pool
@pytest.mark.parametrize("Cin,Cout,H,W,mode", ACT_CASES, ids=ACT_IDS)
def test_act_pool_ragged_equals_the_canvas(dev, Cin, Cout, H, W, mode):
    """skip slots, fp32 a, pooled slots and pooled fp32 (rows of 20, 14, 18, 2 floats) == the full-tile entry on the canvas; the record
    == max of the map's own a"""
    from onet_amd import ops
    c = conv_case(dev, Cin, Cout, H, W, mode)
    Hc, Wc = c["Hc"], c["Wc"]
    Lc = torch.empty((B, Cout, Hc, Wc), device=dev)
    yPc = torch.empty((B, Cout // 8, Hc // 2, 2, Wc // 2, 8), dtype=torch.float16, device=dev)
    yc = torch.empty((B, Cout, Hc // 2, Wc // 2), device=dev)
    aPc = ops.conv3x3_split_pre_act_pool(c["Pc"], c["wq"], Cout, c["save"], c["scale"], a=Lc, yP=yPc, y=yc, **c["kw"])
    assert aPc is not None
    aP, bigP = slots_out(Cout, H, W, dev)
    L, bigL = f32_out(Cout, H, W, dev)
    yP, bigyP = slots_out(Cout, H // 2, W // 2, dev)
    y, bigy = f32_out(Cout, H // 2, W // 2, dev)
    am = amax_slots(dev)
    assert ops.conv3x3_split_pre_act_pool_ragged(c["P"], c["wq"], Cout, c["save"], c["scale"], out=aP, a_amax=am, a=L, yP=yP, y=y,
                                                 **c["kw"]) is aP
    torch.cuda.synchronize()
    assert same(aP, aPc[:, :, :H, :, :W]), "skip slots"
    assert same(L, Lc[:, :, :H, :W]), "fp32 a"
    assert same(yP, yPc[:, :, :H // 2, :, :W // 2]), "pooled slots"
    assert same(y, yc[:, :, :H // 2, :W // 2]), "pooled fp32"
    assert bool((y > 0).any())
    assert gap_intact(bigP, Cout // 8) and gap_intact(bigL, Cout) and gap_intact(bigyP, Cout // 8) and gap_intact(bigy, Cout)
    assert slot_max(am) == float(L.max()) == float(y.max()), (slot_max(am), float(L.max()), float(y.max()))
    # one pooled destination at a time: the same values
    for kw in (dict(yP=True), dict(y=True)):
        yP2, bigyP2 = slots_out(Cout, H // 2, W // 2, dev)
        y2, bigy2 = f32_out(Cout, H // 2, W // 2, dev)
        aP2, bigP2 = slots_out(Cout, H, W, dev)
        assert ops.conv3x3_split_pre_act_pool_ragged(c["P"], c["wq"], Cout, c["save"], c["scale"], out=aP2, yP=yP2 if "yP" in kw else None,
                                                     y=y2 if "y" in kw else None, **c["kw"]) is aP2
        torch.cuda.synchronize()
        assert same(aP2, aP) and gap_intact(bigP2, Cout // 8)
        if "yP" in kw:
            assert same(yP2, yP) and gap_intact(bigyP2, Cout // 8) and all_sentinel(bigy2)
        else:
            assert same(y2, y) and gap_intact(bigy2, Cout) and all_sentinel(bigyP2)


# ----------------------------------------------------------------------------------------------------------------- the exact maximum
@pytest.mark.parametrize("pool", [False, True], ids=["act", "act_pool"])
def test_exact_maximum_is_taken_over_the_map_alone(dev, pool):
    """A case an UNMASKED record gets wrong: a strictly positive input, output channel 5 with all-negative weights, mean 0 and a large
    positive BatchNorm offset (sh = 50) on it.  On the map z[5] < 0, so a[5] = relu(sc z + 50) < 50; two or more pixels outside the map
    every tap reads zero, z = 0 and relu(bn(0)) = 50 exceeds every value on the map.  24 x 40 on a 32 x 64 canvas: each partly filled
    tile holds such pixels.  The ragged launch must record max over the map's a, bit for bit; the canvas launch, whose map IS the
    canvas, records 50 -- strictly more, so the assertion cannot pass vacuously."""
    from onet_amd import ops
    Cin, Cout, H, W, ch = 32, 64, 24, 40, 5
    Hc, Wc = canvas_of(H, W)
    x = rnd(B, Cin, H, W, seed=810).abs() + 0.05
    xc = torch.zeros(B, Cin, Hc, Wc)
    xc[:, :, :H, :W] = x
    x, xc = x.to(dev), xc.to(dev)
    s = ops.absmax_slots(x)
    P, Pc = ops.split_pack_act(x, f16=True, slots=s), ops.split_pack_act(xc, f16=True, slots=s)
    w = rnd(Cout, Cin, 3, 3, seed=811, scale=(2.0 / (Cin * 9)) ** 0.5)
    w[ch] = -w[ch].abs() - 1e-3
    w = w.to(dev)
    save = save_of(Cout, 812, dev)
    save[0, ch], save[2, ch], save[3, ch] = 0.0, 1.0, 50.0
    scale = ops.conv3x3_act_bound(w, save, s)
    qf = pack(w)
    if pool:
        def launch(fn, p, hh, ww, am, a):
            return fn(p, qf, Cout, save, scale, slots=s, a_amax=am, a=a, y=torch.empty((B, Cout, hh // 2, ww // 2), device=dev))
        full, ragged = ops.conv3x3_split_pre_act_pool, ops.conv3x3_split_pre_act_pool_ragged
    else:
        def launch(fn, p, hh, ww, am, a):
            return fn(p, qf, Cout, save, scale, slots=s, a_amax=am, a=a)
        full, ragged = ops.conv3x3_split_pre_act, ops.conv3x3_split_pre_act_ragged
    amc, am = amax_slots(dev), amax_slots(dev)
    ac, a = torch.empty((B, Cout, Hc, Wc), device=dev), torch.empty((B, Cout, H, W), device=dev)
    assert launch(full, Pc, Hc, Wc, amc, ac) is not None and launch(ragged, P, H, W, am, a) is not None
    torch.cuda.synchronize()
    assert same(a, ac[:, :, :H, :W])
    on_map, outside = float(a.max()), float(ac.max())
    print(f"exact maximum ({'act_pool' if pool else 'act'}): on the map {on_map!r}, on the canvas {outside!r}")
    assert outside == 50.0 and float(ac[:, ch, H + 2:, :].min()) == 50.0 and float(ac[:, ch, :, W + 2:].min()) == 50.0
    assert on_map < 50.0 and float(a[:, ch].max()) < 50.0
    assert slot_max(amc) == outside                         # the canvas launch: its map is the canvas
    assert slot_max(am) == on_map, (slot_max(am), on_map)   # the ragged launch: the map alone, bit for bit
    assert slot_max(amc) > slot_max(am)


# ----------------------------------------------------------------------------------------------------------------- head, plain
@pytest.mark.parametrize("H,W", [(24, 40), (28, 28)], ids=["24x40", "28x28"])
def test_head_ragged_equals_the_canvas(dev, H, W):
    """V == the canvas V on the map; L is read from a batch-strided slice; V (no batch stride in the ABI) is a dense slice out of the
    middle of a sentinel buffer"""
    from onet_amd import ops
    Cin = Cout = 64
    c = conv_case(dev, Cin, Cout, H, W)
    Hc, Wc = c["Hc"], c["Wc"]
    Lh = rnd(B, Cout, H, W, seed=820).abs()
    Lc = torch.zeros(B, Cout, Hc, Wc)
    Lc[:, :, :H, :W] = Lh
    Vc = ops.conv3x3_split_pre_head(c["Pc"], c["wq"], Cout, c["save"], Lc.to(dev), **c["kw"])
    assert Vc is not None
    L, _ = f32_out(Cout, H, W, dev)
    L.copy_(Lh.to(dev))
    n = B * H * W
    flat = torch.full((3 * n,), S32, dtype=torch.int32, device=dev).view(torch.float32)
    V = flat[n:2 * n].view(B, 1, H, W)
    assert ops.conv3x3_split_pre_head_ragged(c["P"], c["wq"], Cout, c["save"], L, out=V, **c["kw"]) is V
    torch.cuda.synchronize()
    assert same(V, Vc[:, :, :H, :W]) and bool((V != 0).any())
    assert bool((flat[:n].view(torch.int32) == S32).all()) and bool((flat[2 * n:].view(torch.int32) == S32).all())


@pytest.mark.parametrize("H,W", [(24, 40), (28, 28)], ids=["24x40", "28x28"])
def test_plain_ragged_equals_the_canvas(dev, H, W):
    from onet_amd import ops
    Cin = Cout = 64
    c = conv_case(dev, Cin, Cout, H, W)
    zc = ops.conv3x3_split_pre(c["Pc"], c["wq"], Cout, **c["kw"])
    z, bigz = f32_out(Cout, H, W, dev)
    assert ops.conv3x3_split_pre_plain_ragged(c["P"], c["wq"], Cout, out=z, **c["kw"]) is z
    torch.cuda.synchronize()
    assert same(z, zc[:, :, :H, :W]) and bool((z != 0).any()) and gap_intact(bigz, Cout)


# ----------------------------------------------------------------------------------------------------------------- full tiles
def test_ragged_entries_on_full_tiles_are_the_full_tile_entries(dev):
    """(16, 32): every ragged convolution entry launches what its sibling launches -- the same bits, record included"""
    from onet_amd import ops
    Cin = Cout = 64
    H, W = 16, 32
    c = conv_case(dev, Cin, Cout, H, W)
    args = (c["wq"], Cout, c["save"], c["scale"])
    am0, am1, am2, am3 = (amax_slots(dev) for _ in range(4))
    a0, a1 = torch.empty((B, Cout, H, W), device=dev), torch.empty((B, Cout, H, W), device=dev)
    ref = ops.conv3x3_split_pre_act(c["P"], *args, a_amax=am0, a=a0, **c["kw"])
    got = ops.conv3x3_split_pre_act_ragged(c["P"], *args, a_amax=am1, a=a1, **c["kw"])
    y0, y1 = torch.empty((B, Cout, H // 2, W // 2), device=dev), torch.empty((B, Cout, H // 2, W // 2), device=dev)
    yP0, yP1 = (torch.empty((B, Cout // 8, H // 2, 2, W // 2, 8), dtype=torch.float16, device=dev) for _ in range(2))
    refp = ops.conv3x3_split_pre_act_pool(c["P"], *args, a_amax=am2, yP=yP0, y=y0, **c["kw"])
    gotp = ops.conv3x3_split_pre_act_pool_ragged(c["P"], *args, a_amax=am3, yP=yP1, y=y1, **c["kw"])
    L = rnd(B, Cout, H, W, seed=830).abs().to(dev)
    V0 = ops.conv3x3_split_pre_head(c["P"], c["wq"], Cout, c["save"], L, **c["kw"])
    V1 = ops.conv3x3_split_pre_head_ragged(c["P"], c["wq"], Cout, c["save"], L, **c["kw"])
    z0 = ops.conv3x3_split_pre(c["P"], c["wq"], Cout, **c["kw"])
    z1 = ops.conv3x3_split_pre_plain_ragged(c["P"], c["wq"], Cout, **c["kw"])
    torch.cuda.synchronize()
    bits = lambda t: t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)
    for g, r, what in ((got, ref, "act slots"), (a1, a0, "act a"), (am1, am0, "act record"), (gotp, refp, "pool skip slots"),
                       (yP1, yP0, "pooled slots"), (y1, y0, "pooled fp32"), (am3, am2, "pool record"), (V1, V0, "V"), (z1, z0, "z")):
        assert g is not None and r is not None and torch.equal(bits(g), bits(r)), what
    assert slot_max(am1) == float(a1.max()) > 0


# ----------------------------------------------------------------------------------------------------------------- ConvTranspose2d
def _convt_case(dev, Cin, Ct, h, w, batch):
    from onet_amd import ops
    x = rnd(batch, Cin, h, w, seed=840)
    wt = rnd(Cin, Ct, 2, 2, seed=841, scale=(1.0 / Cin) ** 0.5).to(dev)
    bias = rnd(Ct, seed=842, scale=0.2).to(dev)
    wP = ops.packT2x2_slots(wt, parts=2)
    wP = wP[0] if isinstance(wP, tuple) else wP
    s = ops.absmax_slots(x.to(dev))
    return x, wP, bias, s, ops.convT2x2_out_bound(wt, bias, s)


@pytest.mark.parametrize("Cin,Ct,h,w,batch", [(128, 64, 14, 14, 3), (128, 64, 12, 20, B), (256, 128, 6, 10, B)],
                         ids=["14x14-b3", "12x20", "256to128-6x10"])
def test_convt_ragged_equals_the_zero_extended_map(dev, Cin, Ct, h, w, batch):
    """the up-sampled slots (both parts, scaled by the output's magnitude slots) == the existing kernel on (h', w), zero rows appended
    until h' w % 128 == 0, given the same slots.  Batch 3 at 14 x 14: 196 pixels per image, so an image boundary falls inside a
    128-pixel tile of the existing kernel's global pixel index -- the ragged kernel counts its tiles per image"""
    from onet_amd import ops
    x, wP, bias, s, s_up = _convt_case(dev, Cin, Ct, h, w, batch)
    hc = next(v for v in range(h, h + 129) if (v * w) % 128 == 0)
    assert (h * w) % 128 and hc > h
    xc = torch.zeros(batch, Cin, hc, w)
    xc[:, :, :h] = x
    P, Pc = ops.split_pack_act(x.to(dev), f16=True, slots=s), ops.split_pack_act(xc.to(dev), f16=True, slots=s)
    outc = torch.empty((batch, Ct // 8, 2 * hc, 2, 2 * w, 8), dtype=torch.float16, device=dev)
    assert ops.convT2x2_fwd_slots(Pc, wP, bias, outc, Ct, x_slots=s, slots=s_up, kind="convt_slot_fwd_kernel")
    out, big = slots_out(Ct, 2 * h, 2 * w, dev, batch)
    assert ops.convT2x2_fwd_slots_split_ragged(P, wP, bias, out, Ct, x_slots=s, slots=s_up)
    torch.cuda.synchronize()
    assert same(out, outc[:, :, :2 * h]) and bool((out.float() != 0).any())
    assert gap_intact(big, Ct // 8), "a store left the map"


def test_convt_ragged_on_whole_tiles_is_the_existing_entry(dev):
    """(8, 16) = 128 pixels: bit for bit the existing entry point"""
    from onet_amd import ops
    Cin, Ct, h, w = 128, 64, 8, 16
    x, wP, bias, s, s_up = _convt_case(dev, Cin, Ct, h, w, B)
    P = ops.split_pack_act(x.to(dev), f16=True, slots=s)
    ref = torch.empty((B, Ct // 8, 2 * h, 2, 2 * w, 8), dtype=torch.float16, device=dev)
    assert ops.convT2x2_fwd_slots(P, wP, bias, ref, Ct, x_slots=s, slots=s_up, kind="convt_slot_fwd_kernel")
    out, big = slots_out(Ct, 2 * h, 2 * w, dev)
    assert ops.convT2x2_fwd_slots_split_ragged(P, wP, bias, out, Ct, x_slots=s, slots=s_up)
    torch.cuda.synchronize()
    assert torch.equal(out.contiguous().view(torch.int16), ref.view(torch.int16)) and gap_intact(big, Ct // 8)


# ----------------------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("Cin,H,W", [(32, 23, 40), (32, 24, 38), (24, 24, 40)], ids=["odd-H", "W%4", "Cin%16"])
def test_ragged_convolution_entries_refuse(dev, Cin, H, W):
    """odd H, W % 4 != 0, Cin % 16 != 0: every ragged convolution entry answers "not taken" (1 from the library, None from the wrapper)
    and writes nothing -- slots, fp32 tensors and the record"""
    from onet_amd import ops, _lib
    Cout = 64
    x = rnd(B, Cin, H, W, seed=860).to(dev)
    s = ops.absmax_slots(x)
    P = ops.split_pack_act(x, f16=True, slots=s)
    wq = torch.zeros(Cin * 2 * 9 * Cout + 8, dtype=torch.float16, device=dev) if Cin % 16 else \
        pack(rnd(Cout, Cin, 3, 3, seed=861, scale=0.1).to(dev))
    save = save_of(Cout, 862, dev)
    Hp, Wp = max(H // 2, 1), max(W // 2, 1)
    aP, bigP = slots_out(Cout, H, W, dev)
    a, bigA = f32_out(Cout, H, W, dev)
    yP, bigyP = slots_out(Cout, Hp, Wp, dev)
    y, bigy = f32_out(Cout, Hp, Wp, dev)
    V = torch.full((B, 1, H, W), S32, dtype=torch.int32, device=dev).view(torch.float32)
    L = torch.ones((B, Cout, H, W), device=dev)
    am = amax_slots(dev)
    st = torch.cuda.current_stream().cuda_stream
    rc = _lib.load().onet_conv3x3_split_fwd_pre_act_ragged(P.data_ptr(), Cin * H * W, s.data_ptr(), 0, None, 0, wq.data_ptr(), save.data_ptr(),
                                                           aP.data_ptr(), aP.stride(0) // 2, s.data_ptr(), am.data_ptr(), a.data_ptr(),
                                                           a.stride(0), B, Cin, Cout, H, W, st)
    assert rc == 1
    assert ops.conv3x3_split_pre_act_ragged(P, wq, Cout, save, s, out=aP, slots=s, a_amax=am, a=a) is None
    assert ops.conv3x3_split_pre_act_pool_ragged(P, wq, Cout, save, s, out=aP, slots=s, a_amax=am, a=a, yP=yP, y=y) is None
    assert ops.conv3x3_split_pre_plain_ragged(P, wq, Cout, out=a, slots=s) is None
    assert ops.conv3x3_split_pre_head_ragged(P, wq, Cout, save, L, out=V, slots=s) is None
    torch.cuda.synchronize()
    assert all_sentinel(bigP) and all_sentinel(bigA) and all_sentinel(bigyP) and all_sentinel(bigy)
    assert bool((V.view(torch.int32) == S32).all()) and int(am.abs().max()) == 0


@pytest.mark.parametrize("Cin,h,w", [(128, 6, 5), (144, 6, 6), (96, 6, 6)], ids=["odd-w", "Cin%32", "Cin<128"])
def test_convt_ragged_refuses(dev, Cin, h, w):
    """the ConvTranspose2d entry's own domain (onet_convT2x2_fwd_slots' without h w % 128): odd w, Cin % 32 != 0, Cin < 128 -> not
    taken, nothing written"""
    from onet_amd import ops
    Ct = 64
    x = rnd(B, Cin, h, w, seed=870).to(dev)
    s = ops.absmax_slots(x)
    P = ops.split_pack_act(x, f16=True, slots=s)
    wP = torch.zeros(Cin * 4 * Ct * 2 + 64, dtype=torch.float16, device=dev)
    out, big = slots_out(Ct, 2 * h, 2 * w, dev)
    assert not ops.convT2x2_fwd_slots_split_ragged(P, wP, torch.zeros(Ct, device=dev), out, Ct, x_slots=s, slots=s)
    torch.cuda.synchronize()
    assert all_sentinel(big)
