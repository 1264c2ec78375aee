"""The entry point of include/onet_hip_upmap.h: the slot-operand ConvTranspose2d forward on one-part (plain bf16) slots of a map of ANY w,
into an output map of Ho x Wo slots per channel group with Ho - 2h, Wo - 2w in {0, 1} -- the pad strip written by the same launch.

Reference of every case: ops.convT2x2_fwd_slots_ragged on the map itself (even w), or on the map with ONE zero column appended (odd w).
Pixels are independent columns of the GEMM and the chunk order is the same, so the map's own 2h x 2w block must be EQUAL, value for value
(`==`: -0 = +0), no tolerance.  The pad strip must be bit-zero.  Every output is a slice of a larger buffer pre-filled with a sentinel bit
pattern, with a batch stride above dense (one channel group more per image): the sentinel must be intact outside the Ct / 8 groups'
Ho x Wo maps, which a stray store past a row, a map or an image would break -- nothing is provoked.  Helpers: tests/test_gpu_ragged_kernels.py's."""
import pytest
import torch
import torch.nn.functional as F

from test_gpu_ragged_kernels import rnd, slots_out, gap_intact, same, all_sentinel, _convt_case
from test_gpu_ragged_kernels import dev  # noqa: F401  (the module-scoped fixture)
from test_gpu_fused_eval_bf16 import unslot

pytestmark = pytest.mark.gpu

# (Cin, Ct, h, w, Ho, Wo, batch)
CASES = [(128, 64, 6, 5, 12, 10, 2),          # odd w, no pad
         (128, 64, 3, 12, 6, 25, 2),          # pad column only: the bottom edge of 48 x 200
         (128, 64, 6, 25, 12, 50, 3),         # odd w, 150 pixels: two tiles per image, image boundaries inside the tile count
         (256, 128, 5, 7, 11, 15, 3),         # both pads and the corner
         (128, 64, 12, 12, 25, 25, 2)]        # 200 x 200's own bottom edge
IDS = ["6x5-to-12x10", "3x12-to-6x25", "6x25-to-12x50", "5x7-to-11x15", "12x12-to-25x25"]


def _reference(dev, x, wP, bias, Ct):
    """ops.convT2x2_fwd_slots_ragged on the map, one zero column appended where w is odd -> its [batch, Ct/8, 2h, 1, 2w, 8] block"""
    from onet_amd import ops
    batch, Cin, h, w = x.shape
    we = w + (w & 1)
    xe = torch.zeros(batch, Cin, h, we)
    xe[..., :w] = x
    ref = torch.empty((batch, Ct // 8, 2 * h, 1, 2 * we, 8), dtype=torch.bfloat16, device=dev)
    assert ops.convT2x2_fwd_slots_ragged(ops.split_pack_act(xe.to(dev), parts=1), wP, bias, ref, Ct)
    return ref[:, :, :, :, :2 * w]


def _launch(dev, x, wP, bias, Ct, Ho, Wo):
    from onet_amd import ops
    out, big = slots_out(Ct, Ho, Wo, dev, x.shape[0])
    assert ops.convT2x2_fwd_slots_anymap(ops.split_pack_act(x.to(dev), parts=1), wP, bias, out, Ct)
    torch.cuda.synchronize()
    return out, big


@pytest.mark.parametrize("Cin,Ct,h,w,Ho,Wo,batch", CASES, ids=IDS)
def test_block_equals_the_ragged_entry_and_the_pad_strip_is_zero(dev, Cin, Ct, h, w, Ho, Wo, batch):
    x, wP, bias = _convt_case(dev, Cin, Ct, h, w, batch)
    ref = _reference(dev, x, wP, bias, Ct)
    out, big = _launch(dev, x, wP, bias, Ct, Ho, Wo)
    block = out[:, :, :2 * h, :, :2 * w]
    assert same(block, ref), "the up-sampled block differs from the ragged entry's"
    assert bool((block.float() != 0).any())
    bits = out.contiguous().view(torch.int16)
    assert bool((bits[:, :, 2 * h:] == 0).all()) and bool((bits[:, :, :, :, 2 * w:] == 0).all()), "the pad strip is not bit-zero"
    assert (bits[:, :, 2 * h:].numel() > 0) == (Ho > 2 * h) and (bits[:, :, :, :, 2 * w:].numel() > 0) == (Wo > 2 * w)
    assert gap_intact(big, Ct // 8), "a store left the map"


def test_against_fp64_on_the_rounded_operands(dev):
    """5 x 7 -> 11 x 15 against torch.nn.functional.conv_transpose2d in fp64 on the CPU, on the same operands (x and the weights are
    bf16-representable: the pack's rounding is the identity).  Bound per element: 2^-8 |ref| (the output's bf16 rounding) +
    Cin 2^-23 sum |x| |w| (fp32 accumulation of exact products).  Measured on an MI355X: worst |got - ref| / bound 0.939 (the first
    term: bf16 rounds to nearest, at most 2^-8 of the value at the bottom of a binade)."""
    from onet_amd import ops
    Cin, Ct, h, w, Ho, Wo, batch = CASES[3]
    x, _, bias = _convt_case(dev, Cin, Ct, h, w, batch)
    wt = rnd(Cin, Ct, 2, 2, seed=741, scale=(1.0 / Cin) ** 0.5).to(torch.bfloat16).float()
    wP = ops.packT2x2_slots(wt.to(dev), parts=1)
    wP = wP[0] if isinstance(wP, tuple) else wP
    out, big = _launch(dev, x, wP, bias, Ct, Ho, Wo)
    got = unslot(out)
    ref = F.conv_transpose2d(x.double(), wt.double(), bias.cpu().double(), stride=2)
    terms = F.conv_transpose2d(x.double().abs(), wt.double().abs(), None, stride=2)
    assert tuple(ref.shape) == (batch, Ct, 2 * h, 2 * w)
    bound = 2.0 ** -8 * ref.abs() + Cin * 2.0 ** -23 * terms
    ratio = float(((got[:, :, :2 * h, :2 * w] - ref).abs() / bound).max())
    print(f"5x7 -> 11x15 against fp64: worst |got - ref| / bound = {ratio:.3f}")
    assert ratio <= 1.0, f"{ratio:.3f} x the bound"
    assert float(got[:, :, 2 * h:].abs().max()) == 0.0 and float(got[:, :, :, 2 * w:].abs().max()) == 0.0
    assert gap_intact(big, Ct // 8)


def test_even_w_without_pad_is_the_ragged_entry(dev):
    """14 x 14 -> 28 x 28: bit for bit ops.convT2x2_fwd_slots_ragged, the same launch kind recorded"""
    from onet_amd import ops
    Cin, Ct, h, w, batch = 128, 64, 14, 14, 2
    x, wP, bias = _convt_case(dev, Cin, Ct, h, w, batch)
    P = ops.split_pack_act(x.to(dev), parts=1)
    kinds = []
    outs = []
    for fn in (ops.convT2x2_fwd_slots_ragged, ops.convT2x2_fwd_slots_anymap):
        out, big = slots_out(Ct, 2 * h, 2 * w, dev, batch)
        ops.profile_start(everything=True)
        try:
            assert fn(P, wP, bias, out, Ct)
            torch.cuda.synchronize()
        finally:
            prof, rest = ops.profile_stop()
        kinds.append(({k: len(v) for k, v in prof.items()}, {k: len(v) for k, v in rest.items()}))
        outs.append(out.contiguous().view(torch.int16))
        assert gap_intact(big, Ct // 8)
    assert kinds[0] == kinds[1] and kinds[0][0] == {"convt_slot_fwd_kernel": 1}, kinds
    assert torch.equal(outs[0], outs[1]) and bool((outs[0] != 0).any())


@pytest.mark.parametrize("Cin,Ho,Wo", [(128, 14, 10), (128, 12, 9), (144, 12, 10), (96, 12, 10)], ids=["Ho-2h=2", "Wo-2w=-1", "Cin%32", "Cin<128"])
def test_refusals_write_nothing(dev, Cin, Ho, Wo):
    """outside the domain the entry answers "not taken" (False from the wrapper) and the sentinel canvas is untouched"""
    from onet_amd import ops
    Ct, h, w, batch = 64, 6, 5, 2
    P = ops.split_pack_act(rnd(batch, Cin, h, w, seed=770).to(dev), parts=1)
    wP = torch.zeros(Cin * 4 * Ct + 64, dtype=torch.bfloat16, device=dev)
    out, big = slots_out(Ct, Ho, Wo, dev, batch)
    assert not ops.convT2x2_fwd_slots_anymap(P, wP, torch.zeros(Ct, device=dev), out, Ct)
    torch.cuda.synchronize()
    assert all_sentinel(big)
