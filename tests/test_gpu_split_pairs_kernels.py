"""The entry point of include/onet_hip_split_pairs.h: the fp16 (hi | mid) _act launch on IMAGE-PAIR tiles -- maps of any H and
0 < W <= 16, two images of the batch side by side in a tile's 32 columns, each with its own halo columns.

The method is tests/test_gpu_pairs_kernels.py's on the helpers of tests/test_gpu_ragged_split_kernels.py (imported): every output is a
slice of a sentinel-filled buffer with a batch stride above dense and ONE IMAGE MORE than the batch, whose sentinel must be intact
everywhere else.  The reference of every case is the EXISTING ragged entry (ops.conv3x3_split_pre_act_ragged: one image per tile) on
the same operands and the same magnitude slots -- directly where it takes the map (even H, W % 4 == 0), otherwise on the map zero-padded
to even H and 16 columns and sliced to the map.  Slots and `a` must be EQUAL value for value (`==`): both instances add the same chunks
and taps in the same order per pixel on the same MFMA shape, apply the same epilogue expressions and split by the same 2^k, so a
difference is a bug and there is no tolerance.

What a pair tile can get wrong, and how a case would show it:
  * the right halo of image 0 / the left halo of image 1: a horizontal tap reading the neighbour image changes column W - 1 of image 0
    and column 0 of image 1.  Valid only if image 1's first column is non-zero and finite, which every case asserts;
  * stores beyond the map: at W < 16 the accumulators at columns W .. 15 of a half are relu(bn(partial sums)), not zero.  Every case
    with W < 16 computes them (the ragged entry on the map padded to 16 columns) and asserts that they are finite and not all zero;
  * an odd batch: the last tile holds one image, its second half must stage zeros and store nothing -- the sentinel image behind the
    batch stays intact -- and must not enter the exact-maximum record (relu(bn(0)) is not zero);
  * the record: bit-equal to max of the launch's own `a`, also where an accumulator beyond the map's columns, beyond its rows or of
    the absent image is larger (test_exact_maximum_*: the unmasked value is shown to be reachable)."""
import pytest
import torch

import test_gpu_ragged_split_kernels as rsk
from test_gpu_ragged_split_kernels import dev  # noqa: F401  (the module-scoped fixture)

pytestmark = pytest.mark.gpu

rnd, slots_out, f32_out, gap_intact, all_sentinel, same = rsk.rnd, rsk.slots_out, rsk.f32_out, rsk.gap_intact, rsk.all_sentinel, rsk.same
amax_slots, slot_max, pack, save_of = rsk.amax_slots, rsk.slot_max, rsk.pack, rsk.save_of

KIND = "conv3x3_split_pre_act_pairs_kernel"
# (batch, Cin, Cout, H, W, mode) -- mode as rsk.conv_case: "two": two producers (split_ch = 64, the first one's guard exponent non-zero),
# "guard": the output's bound reaches 2^15
CASES = [(2, 32, 64, 16, 16, "one"), (2, 32, 64, 14, 14, "guard"), (3, 32, 64, 12, 13, "one"), (1, 32, 64, 16, 16, "one"),
         (2, 32, 64, 20, 12, "one"), (4, 96, 128, 3, 10, "two"), (2, 1024, 1024, 14, 14, "one")]
IDS = ["full-pair", "14x14-guard", "b3-12x13", "b1-16x16", "20x12", "b4-96to128-3x10-two-producers", "1024to1024-14x14"]

_REF = {}


def _padded(x, Hp, Wp):
    out = torch.zeros(x.shape[0], x.shape[1], Hp, Wp)
    out[:, :, :x.shape[2], :x.shape[3]] = x
    return out


def _packs(ops, x, sc, dev):
    """-> (P, s1, s2) of x: one producer, or two (channels from sc on their own slot set)"""
    x = x.to(dev)
    if not sc:
        s1 = ops.absmax_slots(x)
        return ops.split_pack_act(x, f16=True, slots=s1), s1, None
    P = torch.empty((x.shape[0], x.shape[1] // 8, x.shape[2], 2, x.shape[3], 8), dtype=torch.float16, device=dev)
    s1, s2 = ops.absmax_slots(x[:, :sc]), ops.absmax_slots(x[:, sc:])
    ops.split_pack_act(x[:, :sc], f16=True, slots=s1, out=P[:, :sc // 8])
    ops.split_pack_act(x[:, sc:], f16=True, slots=s2, out=P[:, sc // 8:])
    return P, s1, s2


def _case(dev, batch, Cin, Cout, H, W, mode):
    """operands of one case, the ragged entry's outputs on them (directly, or on the map padded to even H and 16 columns) and -- W < 16 --
    the activation of the padded map; computed once and left unchanged"""
    from onet_amd import ops
    key = (batch, Cin, Cout, H, W, mode)
    if key in _REF:
        return _REF[key]
    sc = 64 if mode == "two" else 0
    x = rnd(batch, Cin, H, W, seed=900)
    if sc:
        x[:, :sc] *= 1e5
        x[:, sc:] *= 1e-1
    P, s1, s2 = _packs(ops, x, sc, dev)
    w = rnd(Cout, Cin, 3, 3, seed=901, scale=(2.0 / (Cin * 9)) ** 0.5).to(dev)
    save = save_of(Cout, 902, dev, gain={"one": 1.0, "two": 1e-4, "guard": 3.0e4}[mode])
    scale = ops.conv3x3_act_bound(w, save, s1, s2, sc)
    if mode == "guard":
        assert slot_max(scale) >= 2.0 ** 15
    if mode == "two":
        assert slot_max(s1) >= 2.0 ** 15
    wq, kw = pack(w), dict(slots=s1, slots2=s2, split_ch=sc)
    direct = H % 2 == 0 and W % 4 == 0
    aP_ref = a_ref = a16 = None
    if direct:
        a_ref = torch.empty((batch, Cout, H, W), device=dev)
        aP_ref = ops.conv3x3_split_pre_act_ragged(P, wq, Cout, save, scale, a=a_ref, **kw)
        assert aP_ref is not None
    if not direct or W < 16:
        # the SAME magnitude slots: the padded map's packs are scaled by the map's own s1, s2 (zeros stay zeros)
        Hp = H + H % 2
        xp = _padded(x, Hp, 16).to(dev)
        Pp = torch.empty((batch, Cin // 8, Hp, 2, 16, 8), dtype=torch.float16, device=dev)
        if sc:
            ops.split_pack_act(xp[:, :sc], f16=True, slots=s1, out=Pp[:, :sc // 8])
            ops.split_pack_act(xp[:, sc:], f16=True, slots=s2, out=Pp[:, sc // 8:])
        else:
            ops.split_pack_act(xp, f16=True, slots=s1, out=Pp)
        a16 = torch.empty((batch, Cout, Hp, 16), device=dev)
        aP16 = ops.conv3x3_split_pre_act_ragged(Pp, wq, Cout, save, scale, a=a16, **kw)
        assert aP16 is not None
        if not direct:
            aP_ref, a_ref = aP16[:, :, :H, :, :W].contiguous(), a16[:, :, :H, :W].contiguous()
    torch.cuda.synchronize()
    _REF[key] = dict(P=P, wq=wq, save=save, scale=scale, kw=kw, aP=aP_ref, a=a_ref, a16=a16)
    return _REF[key]


@pytest.mark.parametrize("with_a", [True, False], ids=["a", "no-a"])
@pytest.mark.parametrize("batch,Cin,Cout,H,W,mode", CASES, ids=IDS)
def test_act_pairs_equals_the_ragged_entry(dev, batch, Cin, Cout, H, W, mode, with_a):
    """slots and the optional fp32 activation == the ragged entry's on the same operands and magnitude slots, one launch of the pair
    kind, nothing written outside the map or behind the batch; the record == max of the launch's own a.
    Measured on an MI355X: all 14 cases equal (no tolerance to report); the file's 20 cases take 3 s."""
    from onet_amd import ops
    c = _case(dev, batch, Cin, Cout, H, W, mode)
    assert bool((c["a"] > 0).any()) and bool((c["a"] == 0).any())
    if batch > 1:
        col0 = c["a"][1, :, :, 0]
        assert bool(torch.isfinite(col0).all()) and bool((col0 != 0).any()), "image 1's first column must be able to show a halo fault"
    if W < 16:
        beyond = c["a16"][:, :, :H, W:]
        assert bool(torch.isfinite(beyond).all()) and bool((beyond != 0).any()), "the accumulators beyond the map must be able to show a stray store"
        assert same(c["a16"][:, :, :H, :W], c["a"])            # (the padded map's own columns: the same convolution)
    # one image more than the batch in every buffer: the second half of an odd batch's last tile must not reach it
    aP_big, bigP = slots_out(Cout, H, W, dev, batch=batch + 1)
    a_big, bigA = f32_out(Cout, H, W, dev, batch=batch + 1)
    aP, a = aP_big[:batch], (a_big[:batch] if with_a else None)
    am = amax_slots(dev) if with_a else None
    ops.profile_start(everything=False)
    try:
        assert ops.conv3x3_split_pre_act_pairs(c["P"], c["wq"], Cout, c["save"], c["scale"], out=aP, a_amax=am, a=a, **c["kw"]) is aP
        torch.cuda.synchronize()
    finally:
        kinds = {k: len(v) for k, v in ops.profile_stop()[0].items()}
    assert kinds == {KIND: 1}, kinds
    assert same(aP, c["aP"]), "slots differ from the ragged entry's"
    assert torch.equal(aP.contiguous().view(torch.int16), c["aP"].contiguous().view(torch.int16))
    assert gap_intact(bigP[:batch], Cout // 8) and all_sentinel(bigP[batch:]), "a slot store left the map"
    if with_a:
        assert same(a, c["a"]), "fp32 activation differs from the ragged entry's"
        assert gap_intact(bigA[:batch], Cout) and all_sentinel(bigA[batch:]), "an fp32 store left the map"
        assert slot_max(am) == float(a.max()), (slot_max(am), float(a.max()))
    else:
        assert all_sentinel(bigA)


@pytest.mark.parametrize("batch,H,W", [(2, 16, 12), (2, 20, 16), (3, 16, 16)], ids=["W=12", "H=20", "batch=3"])
def test_exact_maximum_is_taken_over_real_pixels_of_real_images(dev, batch, H, W):
    """tests/test_gpu_ragged_split_kernels.py's recipe on pair tiles: a strictly positive input, output channel 5 with all-negative
    weights, mean 0 and sh = 50.  On the map z[5] < 0, so a[5] < 50; wherever every tap reads zero -- columns from W + 2 of a half
    (W = 12), rows from H + 2 of the last row tile (H = 20: rows 22 .. 31), the absent second image of an odd batch's last tile
    (batch 3) -- relu(bn(0)) = 50 exceeds every value on the map.  That the 50 is reachable is shown by the ragged entry on the map
    extended by zeros over exactly that region (16 columns / 32 rows / a fourth all-zero image), whose record and activation are 50.0;
    the pair launch on the map itself must record max of its own `a`, bit for bit, strictly less.
    Measured on an MI355X: on the map 43.736 (W = 12), 43.543 (H = 20), 43.400 (batch 3); on the extended map 50.0 each."""
    from onet_amd import ops
    Cin, Cout, ch = 32, 64, 5
    x = rnd(batch, Cin, H, W, seed=910).abs() + 0.05
    He, We, Be = (32 if H > 16 else H), 16, batch + batch % 2
    xe = torch.zeros(Be, Cin, He, We)
    xe[:batch, :, :H, :W] = x
    x, xe = x.to(dev), xe.to(dev)
    s = ops.absmax_slots(x)
    P, Pe = ops.split_pack_act(x, f16=True, slots=s), ops.split_pack_act(xe, f16=True, slots=s)
    w = rnd(Cout, Cin, 3, 3, seed=911, scale=(2.0 / (Cin * 9)) ** 0.5)
    w[ch] = -w[ch].abs() - 1e-3
    w = w.to(dev)
    save = save_of(Cout, 912, dev)
    save[0, ch], save[2, ch], save[3, ch] = 0.0, 1.0, 50.0
    scale = ops.conv3x3_act_bound(w, save, s)
    qf = pack(w)
    ame, am = amax_slots(dev), amax_slots(dev)
    ae, a = torch.empty((Be, Cout, He, We), device=dev), torch.empty((batch, Cout, H, W), device=dev)
    assert ops.conv3x3_split_pre_act_ragged(Pe, qf, Cout, save, scale, slots=s, a_amax=ame, a=ae) is not None
    assert ops.conv3x3_split_pre_act_pairs(P, qf, Cout, save, scale, slots=s, a_amax=am, a=a) is not None
    torch.cuda.synchronize()
    assert same(a, ae[:batch, :, :H, :W])
    on_map, outside = float(a.max()), float(ae.max())
    print(f"exact maximum (pairs, batch {batch}, {H} x {W}): on the map {on_map!r}, on the extended map {outside!r}")
    region = ae[:, ch, :, W + 2:] if W < 16 else ae[:, ch, H + 2:, :] if H > 16 else ae[batch:, ch]
    assert region.numel() > 0 and float(region.min()) == 50.0 and outside == 50.0 and slot_max(ame) == 50.0
    assert on_map < 50.0 and float(a[:, ch].max()) < 50.0
    assert slot_max(am) == on_map, (slot_max(am), on_map)   # the pair launch: real pixels of real images alone, bit for bit
    assert slot_max(ame) > slot_max(am)


@pytest.mark.parametrize("Cin,Cout,W", [(32, 64, 17), (24, 64, 14), (32, 96, 14)], ids=["W=17", "Cin=24", "Cout=96"])
def test_pairs_entry_refuses(dev, Cin, Cout, W):
    """W > 16, Cin % 16 != 0, Cout % 64 != 0: the entry answers 1 (None from the wrapper) and writes nothing"""
    from onet_amd import ops, _lib
    batch, H = 2, 14
    x = rnd(batch, Cin, H, W, seed=960).to(dev)
    s = ops.absmax_slots(x)
    P = ops.split_pack_act(x, f16=True, slots=s)
    wq = torch.zeros(Cin * 2 * 9 * Cout + 8, dtype=torch.float16, device=dev)
    save = torch.zeros((4, Cout), device=dev)
    Cb = -(-Cout // 8) * 8
    aP, bigP = slots_out(Cb, H, W, dev)
    a, bigA = f32_out(Cout, H, W, dev)
    scale, am = ops.new_amax(dev), amax_slots(dev)
    before = am.clone()
    st = torch.cuda.current_stream().cuda_stream
    rc = _lib.load().onet_conv3x3_split_fwd_pre_act_pairs(P.data_ptr(), P.stride(0) // 2, s.data_ptr(), 0, None, 0, wq.data_ptr(), save.data_ptr(),
                                                          aP.data_ptr(), aP.stride(0) // 2, scale.data_ptr(), am.data_ptr(), a.data_ptr(),
                                                          a.stride(0), batch, Cin, Cout, H, W, st)
    assert rc == 1
    assert ops.conv3x3_split_pre_act_pairs(P, wq, Cout, save, scale, out=aP, slots=s, a_amax=am, a=a) is None
    torch.cuda.synchronize()
    assert all_sentinel(bigP) and all_sentinel(bigA)
    assert torch.equal(am, before)
