"""Fused eval-mode inference (Settings.fused_eval): a straight-line forward plan on the pre-split kernels.

In eval BatchNorm is a fixed per-channel affine map, so `relu(bn(z))` rides in the convolution's epilogue and the activation leaves
the convolution as 16-byte slots: no pre-activation tensor, no BatchNorm pass, half the HBM bytes per activation element of the
default eval path.  No autograd Function is involved: the plan reads the module tree's parameters and buffers and calls `ops`
directly.

THE TABLE.  Every fused convolution launch is one row of ops.EVAL_ENTRIES, keyed by
  slot format   "fp16x2": fp16 (hi | mid) parts, fp32-level results; "bf16": ONE part of plain bf16 -- the operands conv == "bf16"
                trains with, one MFMA per product term instead of three and 2-byte slot elements (_Format);
  level mode    what the maps of a level are (_Level.mode, below);
  epilogue      "act" (a fused unit), "act_pool" (a unit in front of a max-pool as ONE launch: skip slots, L at level 0 and the 2 x 2
                maximum from the same accumulators), "head" (the last unit of a labels-only call), "plain" (fp32 z: the last unit
                elsewhere, and the first pass of a two-pass pooled unit).
The plan names the mode of each level once (_build_plan) and its units look their launch up (_launch); nothing else decides a launch.

LEVELS AND MODES.  Level k is the part of the U-Net on maps of H >> k x W >> k.  The plan is fused down to depth d, the deepest level
all of whose layers the level's predicate accepts (_depth); the levels below run the existing eval kernels on fp32 tensors (the pooled
tensor of level d - 1 is written as fp32 going down, ops.convT2x2_fwd_p writes slots coming back up).  A fused level's mode is the
narrowest of
  "full"     maps made of full 16 x 32 tiles: every value, every level (256 x 256 down to its 32-pixel level);
  "ragged"   even H, W % 4 == 0, wider than 16 pixels (the *_ragged entries: the same kernels, bounds-checked loads that return zero
             and guarded stores): the "+ragged" and "+anymap" values, every level -- the data sets' 224 x 224 down to its 28-pixel
             level, 200 x 200 down to 100;
  "anymap"   ANY H and W above the width floor: the "+anymap" values, levels k >= 1 -- 200 x 200 (200, 100, 50, 25, 12) down to its
             25-pixel level.  The pooling rounds down, as nn.MaxPool2d(2) does, and a unit in front of a pool on an odd map writes
             the floor-pooled tensor.  Level 0 keeps the ragged domain (the stem's pass and the head's float4 accesses need
             W % 4 == 0 and even H).  One-part format only: without it H and W must be multiples of 2^k at level k;
  "pairs"    level 4, and level 4 alone, where its map is ops.PAIRS_MIN_W .. 16 pixels wide (16 x 16, 14 x 14, 12 x 12 for inputs of
             256, 224, 200 pixels): the "+pairs" values of either format.  One image fills at most half of a 16 x 32 tile there, so
             the launch puts TWO images side by side per tile.  The level has no pooled unit and no head; a level k < 4 that narrow
             stays a fall-back level (its pooled unit would need a pooled pair launch).
and the predicate a level is asked with is the widest one its value enables there (_asked_mode), which says yes wherever the narrower
ones do.  On a map a narrower mode takes, the launches, their order and the bits are those of the value without the wider mode: a
256 x 256 input runs the plan of "bf16+pool" / "fp16x2+pool" down to its 32-pixel level under every value.
  value                          format   pooled units   modes
  True                           fp16x2   two passes     full
  "fp16x2+pool"                  fp16x2   one launch     full
  "fp16x2+ragged"                fp16x2   one launch     full, ragged
  "fp16x2+ragged+pairs"          fp16x2   one launch     full, ragged, pairs
  "bf16"                         bf16     two passes     full
  "bf16+pool"                    bf16     one launch     full
  "bf16+pool+ragged"             bf16     one launch     full, ragged
  "bf16+pool+anymap"             bf16     one launch     full, ragged, anymap
  "bf16+pool+anymap+pairs"       bf16     one launch     full, ragged, anymap, pairs
  "bf16+pool+anymap+pairs+up"    bf16     one launch     ... and the any-map ConvTranspose2d edge (below)
A pooled unit in two passes is a plain convolution writing the fp32 pre-activation and one BatchNorm + ReLU + pooling pass reading it
back; as one launch it writes the same bits.

What is not in the table:

MAGNITUDE SLOTS (fp16x2 alone: bf16 has fp32's exponent range, so that format carries none -- scale = amax = None on every tensor, no
bound launches).  Every tensor kept as slots carries two sets:
  scale   an upper BOUND of max |a|, known before the launch that writes the tensor (ops.conv3x3_act_bound from the weights, the
          coefficients and the input's magnitude; ops.convT2x2_out_bound): the fp16 parts are those of 2^k a with the guard k these
          slots select, and the consumers undo 2^k from the same slots;
  amax    the EXACT max |a| the fused epilogue recorded -- what the next layer's bound starts from, so that the looseness of a bound
          never exceeds one convolution (one ConvTranspose2d + one convolution behind a ConvTranspose2d).  Producers without an
          exact record (the stem's and the pooled units' BatchNorm passes) hand their bound on: at most three bounds chain
          (measured: 56-183x per convolution, up to 1.4e4x where two chain -- profiles/r07_fused_eval.md).
A pooled unit hands on its bound as scale AND amax in one launch as in two passes, so every launch behind it sees the same magnitude
slots and the forward is bit-identical either way.  On a ragged or pair level amax is the EXACT maximum over the map's own pixels of
the batch's own images (those instances mask their record: relu(bn(.)) of an out-of-map accumulator is not zero and would otherwise
loosen every later bound; an absent image of an odd batch's last pair tile is masked likewise).
One exception, the hand-off in front of an fp16 pair level (_pooled_unit(record=True)): down3.c2 also records the exact maximum of its
activation and hands it on with the POOLED tensor -- otherwise down4.c1's bound would chain two bounds over its 4608-term sums
(measured: 1.45e4 - 1.70e4 x the exact maximum on small maps, above the full-tile plan's 1.4e4 x); down3.c2's skip tensor keeps the
bound, as every other pooled unit's tensors do.

CONVTRANSPOSE2D EDGES.  The ConvTranspose2d of level k reads the output of level k + 1 and fills the up-sampled groups of level k's
concat buffer; _Level.route names its launch, a row of _ROUTES: what the edge reads and, for the slot routes, the edge mode of its row
in ops.CONVT_ENTRIES.  _up_edge decides the route, _conv_t looks the launch up and runs it; a refusal is an error, never another route:
  "slots"         the slot-operand GEMM, from the slots of a fused level below (h w % 128 == 0);
  "slots_ragged"  its ragged entry (h w % 128 != 0, even w; two parts on fp16x2) where ops.convt_slots_ok_ragged holds;
  "gemm"          from an fp32 tensor -- a fall-back level's output, or a fused level's fp32 copy where the switches or the channel
                  counts keep the slot GEMM off -- by the fp32-operand GEMM that writes slots (ops.convT2x2_fwd_p), and nothing else;
  "pack"          where that GEMM does not take the map: the general kernel into an fp32 tensor of the concat map's size, then one
                  conversion pass (two parts scaled by the ConvTranspose2d's own bound on fp16x2).  On any-map levels also wherever
                  the output must be padded (level k is odd) or the input map has odd w -- the slot GEMMs keep their dense 2h x 2w,
                  even-w domain -- at the reference's F.pad offsets (diffY // 2, diffX // 2; the pad strip zeroed first);
  "slots_anymap"  "+up" alone: ONE launch of the slot-operand GEMM's any-map entry on exactly those padded / odd-w edges between fused
                  levels where ops.convt_slots_ok_anymap holds -- at 200 x 200 up1 (12 -> 24, placed in 25) and up2 (25 -> 50).  It
                  puts the 2h x 2w block at the top-left corner of the concat map (floor pooling leaves at most one row and one
                  column over, so the reference's F.pad offsets are 0) and writes the pad strip as zero slots itself: no memset, no
                  general kernel, no conversion pass.
keep_fp32: where an edge reads fp32 from a FUSED level ("pack", "gemm"), that level's last unit also writes its activation as fp32
(_Unit.keep_fp32); under "+up" an edge between fused levels reads slots, so the pair launch of down4.c2 and the any-map launch below
an odd level write slots alone.
Why "+up" is a value of its own: its edge reads bf16-rounded slots where `pack` read the unrounded fp32 activation, so its results
differ in the last bf16 digit.  An edge from a fall-back level keeps `pack`; whole-tile and ragged even-w edges keep their routes: an
input without a padded or odd-w edge (224 x 224, 256 x 256) launches what "bf16+pool+anymap+pairs" launches, the same bits.

LABELS-ONLY CALLS (scores, segment(head="fused")): the same plan on either slot format, ending in ONE launch for the last unit and the
head's channel product (epilogue "head": relu(bn(.)) on the accumulators, times L, summed over the unit's 64 channels, V the only
store) followed by ops.softmax2_labels.  The last unit's fp32 pre-activation -- the largest tensor of the forward -- is never written,
the head kernel does not run, and segment does not materialise S.  Onet.forward does not take this route: under every setting it
launches what it launched before these calls existed.

The validation step (validate, EvalCounts): the scores of a batch -- by the labels-only plan where it applies, the ordinary forward
elsewhere -- then ONE launch (ops.score_counts) that forms the labels and adds each image's confusion counts against the ground truth
into a device tensor; nothing synchronises, and metrics.epoch_metrics turns an epoch's rows into the reference's metrics on the host.
A new call: the functions above launch and return what they did without it.

Every decision about what runs where is taken once per U-Net pass, by _build_plan: the query (unet_plan, fused_eval_plan) prints its
record, the executor (_unet_pass) follows it, and _gate is the one place that says whether the plan runs at all and on which passes.
The slot format is chosen once per plan (_format); the units below take it from there."""
from __future__ import annotations

from collections import namedtuple

import torch

from . import ops


_ENC = ("inc", "down1", "down2", "down3", "down4")        # the encoder block of level k
_DEC = ("up4", "up3", "up2", "up1")                       # the Up block of level k (up4: the full-size level's, the last one applied)


def _blocks(unet):
    """-> (encoder DoubleConvs by level 0 .. 4, Down modules by level 1 .. 4, Up modules by level 0 .. 3)"""
    downs = (unet.down1, unet.down2, unet.down3, unet.down4)
    enc = (unet.inc,) + tuple(d.maxpool_conv[1] for d in downs)
    return enc, downs, (unet.up4, unet.up3, unet.up2, unet.up1)


def _units(blk):
    s = blk.double_conv
    return s[0], s[1], s[3], s[4]


# The slot format of a plan: parts per slot, the weight pack, whether tensors carry magnitude slots (without them: scale = amax = None
# everywhere, no bound launches) and whether the pooled tensors are traced (the one-part plan's trace is complete -- every convolution's
# exact input can be rebuilt); modes, upmap: the level modes and the ConvTranspose2d rule the setting's value enables (ops._FusedEval)
_Format = namedtuple("_Format", "operands parts pack magnitude trace_pool modes upmap")
_FORMATS = {"bf16": (1, "plain16", False, True), "fp16x2": (2, "split", True, False)}
# (slot format, the widest mode a level is asked with) -> the layer predicate in `ops` (by name: read at call time, printed in reasons)
_LAYER_OK = {("fp16x2", "full"): "eval_layer_ok", ("fp16x2", "ragged"): "eval_layer_ok_ragged_fp16", ("fp16x2", "pairs"): "eval_layer_ok_pairs_fp16",
             ("bf16", "full"): "eval_layer_ok_bf16", ("bf16", "ragged"): "eval_layer_ok_ragged", ("bf16", "anymap"): "eval_layer_ok_anymap",
             ("bf16", "pairs"): "eval_layer_ok_pairs"}


def _format():
    """The format and modes Settings.fused_eval selects (off: the fp16 format's fields around operands = None)"""
    v = ops._fused_eval_value()
    return _Format(v.format, *_FORMATS[v.format or "fp16x2"], v.modes, v.upmap)


def _asked_mode(fmt, k, w):
    """The mode whose predicate level k (maps w pixels wide) is asked with: the widest the value enables there -- level 4 takes pairs
    where w <= 16, level 0 never takes any-map"""
    if k == 4 and w <= 16 and "pairs" in fmt.modes:
        return "pairs"
    if k and "anymap" in fmt.modes:
        return "anymap"
    return "ragged" if "ragged" in fmt.modes else "full"


def _layer_ok(fmt, mode):
    return getattr(ops, _LAYER_OK[fmt.operands, mode])


def _static_reason(unet, fmt):
    """Why the plan cannot run on this U-Net whatever the input (None: it can)."""
    from .modules import ConvT2x2, _hooked
    if unet.training:
        return "the module is in training mode"
    if getattr(unet, "bilinear", False) or not all(isinstance(u.up, ConvT2x2) for u in _blocks(unet)[2]):
        return "bilinear Up blocks"
    for m in unet.modules():
        if isinstance(m, torch.nn.BatchNorm2d) and (m.training or m.running_mean is None or m.running_var is None):
            return "a BatchNorm without running statistics (or in training mode)"
    if _hooked(unet):
        return "a forward hook watches a block"
    if fmt.parts == 1:
        if not ops.presplit():
            return "pre-split storage is off under the effective convolution algorithm"
    elif not (ops.presplit() and ops.p16_parts() == 2):
        return "the effective convolution algorithm is not the fp16-split one with pre-split storage"
    return None


def _level_units(unet):
    """-> [level] -> (encoder units, decoder units) of that level's maps, each [(name, conv, bn)] in execution order, of the 3x3
    convolutions the plan runs on pre-split operands (all but the stem)"""
    def named(name, blk):
        c1, b1, c2, b2 = _units(blk)
        return [(name + ".c1", c1, b1), (name + ".c2", c2, b2)]
    enc, _, ups = _blocks(unet)
    out = [(named(_ENC[k], enc[k]), named(_DEC[k], ups[k].conv) if k < 4 else []) for k in range(5)]
    out[0] = (out[0][0][1:], out[0][1])
    return out


def _level_layers(unet):
    """-> [level] -> [(name, conv)] of the 3x3 convolutions on that level's maps that the plan runs on pre-split operands"""
    return [[(name, conv) for name, conv, _ in e + d] for e, d in _level_units(unet)]


def _depth(units, ups, fmt, N, H, W):
    """-> (d, why level d is not fused | None): levels 0 .. d - 1 are fused.  With any-map levels level k is H >> k x W >> k (floor
    pooling) whatever the input's divisibility; without, the input size must be a multiple of 2^k"""
    anymap = "anymap" in fmt.modes
    for k, (e, d) in enumerate(units):
        if not anymap and ((H % (1 << k)) or (W % (1 << k))):
            return k, f"level {k}: the input size is not a multiple of {1 << k}"
        h, w = H >> k, W >> k
        if anymap and (h <= 0 or w <= 0):
            return k, f"level {k}: the map is empty"
        mode = _asked_mode(fmt, k, w)
        layer_ok = _layer_ok(fmt, mode)
        for name, conv, _ in e + d:
            if not layer_ok(N, conv.in_channels, conv.out_channels, h, w):
                # (on a map made of full tiles, or no wider than 16 pixels, the ragged and any-map predicates ARE the full-tile one, and
                # the reason says so: the answer of the value without those modes)
                beyond = mode in ("ragged", "anymap") and w > 16 and not ops.full_tiles(h, w)
                ok_name = (layer_ok if beyond or mode == "pairs" else _layer_ok(fmt, "full")).__name__
                why = f"level {k}: {name} ({conv.in_channels} -> {conv.out_channels} on {N} maps of {h} x {w}) is outside ops.{ok_name}"
                if beyond and mode == "ragged" and (w % 4 or h % 2):
                    why += f": W = {w} must be a multiple of 4 and H = {h} even"
                return k, why
        if k < 4:
            C, up = e[-1][1].out_channels, ups[k].up
            if C % 32 or d[0][1].in_channels != C + up.out_channels or up.out_channels % 8:
                return k, f"level {k}: the concat buffer's channel groups do not fit the slot layout"
    return 5, None


def _head_ok(unet):
    """Does the last unit fit the convolution with the head epilogue (ops.conv3x3_*_pre_head: one 64-channel tile per pixel)?"""
    return _units(_blocks(unet)[2][0].conv)[2].out_channels == 64


def _check_head(head):
    if head not in (None, "fused"):
        raise ValueError(f"onet_amd: head must be None or 'fused', not {head!r}")


# ----------------------------------------------------------------------------- the plan record
# One unit (Conv-BatchNorm-ReLU) of a pass.  kind: what unet_plan prints; keep_fp32: a unit that writes slots also writes fp32, for a
# ConvTranspose2d that reads it as "fp32->slots"
_Unit = namedtuple("_Unit", "name conv bn kind keep_fp32")
# One level: its encoder and decoder units in execution order, the ConvTranspose2d that fills its concat buffer with its kind ("slots":
# from the slots of the level below; "fp32->slots": from an fp32 tensor; level 4 has none), whether the pooled tensor leaves as slots
# (fp32: for the fall-back levels), the level's mode ("full" | "ragged" | "anymap" | "pairs": the key its units look their launches up
# with; None: a fall-back level) and the route of the launch(es) behind `convt` (module docstring)
_Level = namedtuple("_Level", "enc dec up convt pooled_slots mode route", defaults=(None, None))
# One U-Net pass.  reason: why the plan does not run (None: it runs); static: the part of it that holds whatever the input;
# levels 0 .. depth - 1 are fused, fallback_reason says why level `depth` is not; head: the last unit ends in the head-epilogue launch
_Plan = namedtuple("_Plan", "fmt batch reason static depth fallback_reason unet levels head", defaults=(None, 0, None, None, (), False))

_WHY_CHANNELS = "the input's channels do not match the stem"


def _build_plan(unet, shape, head=None):
    """The record of a pass of `unet` over an input of `shape` = (N, C, H, W) under the active settings -- every decision the query
    announces and the executor follows, taken here and nowhere else.  Built per call (training flags, hooks, settings and running
    statistics may change between calls); touches no device beyond ops.n_cu()."""
    N, C, H, W = shape
    fmt = _format()
    why = _static_reason(unet, fmt)
    if why is not None:
        return _Plan(fmt, N, why, why)
    if C != unet.inc.double_conv[0].in_channels:
        return _Plan(fmt, N, _WHY_CHANNELS)
    units, ups = _level_units(unet), _blocks(unet)[2]
    d, why_d = _depth(units, ups, fmt, N, H, W)
    if d == 0:
        return _Plan(fmt, N, why_d, None, 0, why_d)
    edges = [_up_edge(fmt, d, k, N, up.up.in_channels, up.up.out_channels, (H >> (k + 1), W >> (k + 1)), (H >> k, W >> k)) for k, up in enumerate(ups)]
    convt = [e[0] for e in edges]
    with_head = head == "fused" and _head_ok(unet)
    # pooled units: plain convolution + BatchNorm / ReLU / pooling pass writing slots, or -- "+pool" -- all of it in the convolution's launch
    pooled_kind = "fused+pool" if ops.fused_eval_pool() else "two-pass"
    levels = []
    for k, (e, dec) in enumerate(units):
        kind = dict.fromkeys((name for name, _, _ in e + dec), "fused" if k < d else "fallback")
        if k < min(d, 4):
            kind[e[-1][0]] = pooled_kind
        if k == 0:
            e = [("inc.c1",) + _units(unet.inc)[:2]] + e
            kind["inc.c1"], kind[dec[-1][0]] = "stem", ("fused+head" if with_head else "plain+head")
        keep = {(dec or e)[-1][0]} if 0 < k < d and convt[k - 1] == "fp32->slots" else ()
        enc_u, dec_u = ([_Unit(name, conv, bn, kind[name], name in keep) for name, conv, bn in us] for us in (e, dec))
        levels.append(_Level(enc_u, dec_u, ups[k].up if k < 4 else None, convt[k] if k < 4 else None, k + 1 < d,
                             _level_mode(fmt, k, H >> k, W >> k) if k < d else None,
                             edges[k][1] if k < 4 else None))
    return _Plan(fmt, N, None, None, d, why_d, unet, tuple(levels), with_head)


def _level_mode(fmt, k, h, w):
    """_Level.mode of fused level k on h x w maps: the narrowest mode that holds the map (a fused map no wider than 16 pixels is there
    by the pair predicate alone)"""
    if ops.full_tiles(h, w):
        return "full"
    if k == 4 and w <= 16 and "pairs" in fmt.modes:
        return "pairs"
    return "ragged" if ops._ragged_map(h, w) else "anymap"


# The ConvTranspose2d edges: route -> (what the edge reads = _Level.convt, the mode of its launch in ops.CONVT_ENTRIES | None: one of the
# two fp32 routes of _conv_t, the predicate in `ops` that accepted the shape)
_Route = namedtuple("_Route", "convt mode ok", defaults=(None, None))
_ROUTES = {"slots": _Route("slots", "full", "convt_slots_ok"), "slots_ragged": _Route("slots", "ragged", "convt_slots_ok_ragged"),
           "slots_anymap": _Route("slots", "anymap", "convt_slots_ok_anymap"), "gemm": _Route("fp32->slots"), "pack": _Route("fp32->slots")}


def _up_edge(fmt, d, k, N, cin, ct, lo, hi):
    """-> (convt, route) of the ConvTranspose2d (cin -> ct) that reads the output of level k + 1 (maps of lo = (h, w)) and fills level
    k's concat buffer (maps of hi): slots where level k + 1 is fused (k + 1 < d) and a slot-operand entry takes the map, else the fp32
    tensor its producer -- the last unit of level k + 1, or the fall-back levels -- leaves"""
    (h, w), ragged = lo, "ragged" in fmt.modes
    if k >= d:
        return "fallback", None
    if "anymap" in fmt.modes and (hi != (2 * h, 2 * w) or w % 2):
        # (any-map levels: the output is padded into the concat buffer -- level k is odd -- or the input map has odd w; the slot
        # GEMMs keep their dense 2h x 2w, even-w domain -- but for the any-map entry, which takes both and writes the pad strip)
        route = "slots_anymap" if fmt.upmap and k + 1 < d and ops.convt_slots_ok_anymap(N, cin, ct, h, w, *hi) else "pack"
    elif k + 1 < d and ops.convt_slots_ok(N, cin, ct, h, w, parts=fmt.parts):
        route = "slots"
    elif k + 1 < d and ragged and (h * w) % 128 and ops.convt_slots_ok_ragged(N, cin, ct, h, w, parts=fmt.parts):
        route = "slots_ragged"
    else:
        # (without ragged levels a fused level is made of full 16 x 32 tiles, so the map below it has h w % 128 == 0)
        route = "pack" if ragged and (h * w) % 128 else "gemm"
    return _ROUTES[route].convt, route


def _query(unet, shape, head=None, device=None):
    """_build_plan for a caller that has a shape and no tensor: behind the checks the executors make on the input itself"""
    fmt, shape = _format(), tuple(shape)
    if len(shape) != 4:
        return _Plan(fmt, 0, "the input is not 4-D")
    N, C, H, W = (int(v) for v in shape)
    if N <= 0:
        C = None        # (an empty batch is announced as a channel mismatch; the executors leave its refusal to the kernels)
    dev = device if device is not None else next(unet.parameters()).device
    if dev.type != "cuda":
        return _Plan(fmt, N, "the model is not on a GPU")
    if not ops.fused_eval():
        return _Plan(fmt, N, "Settings.fused_eval is off")
    with torch.cuda.device(dev):
        return _build_plan(unet, (N, C, H, W), head)


def _plan_dict(plan):
    out = {"fused": plan.reason is None, "reason": plan.reason, "depth": plan.depth, "batch": plan.batch, "layers": {}, "convt": {},
           "fallback_reason": plan.fallback_reason, "operands": plan.fmt.operands}
    for k, lv in enumerate(plan.levels):
        out["layers"].update((u.name, u.kind) for u in lv.enc + lv.dec)
        if lv.up is not None:
            out["convt"][_DEC[k]] = lv.convt
    return out


def unet_plan(unet, shape, device=None, head=None):
    """What the fused plan does with a U-Net pass over an input of `shape` = (N, C, H, W): a pure query, nothing is launched.
    -> {"fused": bool, "reason": why not | None, "depth": d, "batch": N, "layers": {name: "stem" | "fused" | "two-pass" | "fused+pool" |
    "plain+head" | "fused+head" | "fallback"}, "convt": {name: "slots" | "fp32->slots" | "fallback"}, "fallback_reason": why level d is not fused |
    None, "operands": the slot format the settings select, "fp16x2" | "bf16" (None: Settings.fused_eval is off)}
    head = "fused": the plan of the labels-only calls (scores, segment(head="fused")) -- "fused+head" where the last unit runs with the
    head in its epilogue; a last unit outside that kernel's domain (Cout != 64) sends those calls to the ordinary forward, whose plan
    this then is ("plain+head")."""
    _check_head(head)
    return _plan_dict(_query(unet, shape, head, device))


def _gate(model, shape, head=None, x=None):
    """Does the plan run for `model` (an Onet or a UNet) on an input of `shape`, and with which passes?  -> ([(unet, plan)], twin): one
    pass per U-Net, over a batch of 2 B where the twin batch is on; the plan runs where every record's reason is None (_runs).
    x: the input itself, for the executors (`shape` is then its own) -- an input or a mode the plan never takes gives no passes at all;
    None: a query by shape.
    head = "fused" holds only where the last unit of every U-Net fits the head-epilogue launch."""
    if x is not None:
        if not (ops.fused_eval() and not model.training and not torch.is_grad_enabled() and _input_ok(x)):
            return [], False
        shape = x.shape
    from .modules import Onet
    unets, twin, shape = (model,), False, tuple(shape)
    if isinstance(model, Onet):
        shared = model.dwnu is model.topu
        unets, twin = ((model.topu,) if shared else (model.topu, model.dwnu)), bool(shared and ops.twin_enabled())
    if twin and len(shape) == 4:
        shape = (2 * shape[0],) + shape[1:]
    if head == "fused" and not all(_head_ok(u) for u in unets):
        head = None
    build = _query if x is None else _build_plan
    return [(u, build(u, shape, head)) for u in unets], twin


def _runs(passes):
    return bool(passes) and all(plan.reason is None for _, plan in passes)


def fused_eval_plan(model, shape, head=None):
    """What `model(X)` does with an input of `shape` (B, C, H, W) under its settings: see unet_plan.  For an Onet the batch through
    each U-Net is 2 B when the weights are shared and the twin batch is on ("twin": True), B otherwise (two passes).
    head = "fused": what scores(model, X) / segment(model, X, head="fused") do instead ("fused+head" for up4.c2 where the fused launch
    runs; both U-Nets of an unshared model must qualify).
    The answer holds for the model's device: ops.eval_layer_ok follows the convolution dispatch, which asks for enough tiles to fill
    that device's compute units, so the fused depth of a small batch can differ between devices."""
    from .modules import Onet
    _check_head(head)
    if not isinstance(model, Onet):
        return unet_plan(model, tuple(shape))
    with ops.using(model.settings):
        passes, twin = _gate(model, shape, head)
        plan = _plan_dict(passes[0][1])
        plan["twin"] = twin
        for _, other in passes[1:]:
            if plan["fused"] and other.reason is not None:
                plan.update(fused=False, reason="dwnu: " + str(other.reason), depth=0)
        return plan


# Diagnostics (tests, tools): a list here receives (layer name, _T record) of every tensor the plan writes as slots, in order
TRACE = None


def _note(name, t):
    if TRACE is not None:
        TRACE.append((name, t))
    return t


def _input_ok(x):
    return isinstance(x, torch.Tensor) and x.dim() == 4 and x.is_cuda and x.dtype == torch.float32 and not ops.is_placeholder(x)


# ----------------------------------------------------------------------------- the plan's units
class _T:
    """An activation of the plan: P = slots (or None), F = fp32 tensor (or None), scale / amax = magnitude slots (module docstring);
    a concat buffer's are triples (skip set, up-sampled set, first channel of the second group)."""
    __slots__ = ("P", "F", "scale", "amax")

    def __init__(self, P=None, F=None, scale=None, amax=None):
        self.P, self.F, self.scale, self.amax = P, F, scale, amax


def _coeffs(bn):
    return ops.bn_eval_coeffs(bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps)


def _amax(t):
    return t.amax if t.amax is not None else ops.absmax_slots(t.F)


def _bound(fmt, conv, save, t):
    """The scale slots of relu(bn(conv(t))), from the magnitude of `t` (None on a format without magnitude slots)"""
    if not fmt.magnitude:
        return None
    s1, s2, ch = ops._slots3(_amax(t))
    return ops.conv3x3_act_bound(conv.weight, save, s1, s2, ch)


def _wq(fmt, conv):
    return conv.packed().get_pack(fmt.pack)[0]


def _slot_kw(fmt, t, **out):
    """The magnitude-slot arguments of a convolution launch on operand `t` (out: those of its output) -- none on a format without"""
    if not fmt.magnitude:
        return {}
    s1, s2, ch = ops._slots3(t.scale)
    return dict(out, slots=s1, slots2=s2, split_ch=ch)


def _stem_unit(fmt, u, x):
    """The stem: the existing direct kernel, then one BatchNorm + ReLU pass that writes slots"""
    N, _, H, W = x.shape
    z0 = ops.conv3x3_auto(x, u.conv.packed(), 0)
    save0 = _coeffs(u.bn)
    scale0 = _bound(fmt, u.conv, save0, _T(None, x))
    a0 = ops.p16_empty(N, u.conv.out_channels, H, W, x.device, parts=fmt.parts)
    ops.bn_relu_apply_split(z0, save0, a0, slots=scale0)
    return _T(a0, None, scale0, scale0)


def _launch(fmt, mode, epilogue, conv, t, *args, **kw):
    """The launch ops.EVAL_ENTRIES holds for a unit of this format on a level of `mode`, on the slots of `t` with conv's weight pack:
    the row's binding in `ops`, read at call time (tests and tools watch or replace a binding by its name)"""
    name = ops.eval_conv_name(fmt.operands, mode, epilogue)
    out = None if name is None else getattr(ops, name)(t.P, _wq(fmt, conv), conv.out_channels, *args, **kw)
    if out is None:
        raise RuntimeError(f"onet_amd: no {epilogue!r} launch of {fmt.operands} slots took a {mode!r} level the plan's layer predicate accepted "
                           f"({tuple(t.P.shape)} -> {conv.out_channels} channels)")
    return out


def _fused_unit(fmt, u, t, mode):
    """Conv-BatchNorm-ReLU in one launch, output as slots (+ fp32 when another reader needs it)"""
    conv = u.conv
    save = _coeffs(u.bn)
    scale = _bound(fmt, conv, save, t)
    B, _, H, _, W, _ = t.P.shape
    amax = ops.new_amax(t.P.device) if fmt.magnitude else None
    a = torch.empty((B, conv.out_channels, H, W), dtype=torch.float32, device=t.P.device) if u.keep_fp32 else None
    # (every mode takes the same magnitude-slot arguments: none on the one-part format, whose entries beyond "full" record no maximum;
    # the fp16 ones take aP_slots = the bound and a_amax = a fresh record)
    aP = _launch(fmt, mode, "act", conv, t, save, a=a, **_slot_kw(fmt, t, aP_slots=scale, a_amax=amax))
    return _T(aP, a, scale, amax)


def _plain_conv(fmt, conv, t, mode):
    if mode == "full":          # (the training forward's launch: not an eval entry)
        return ops.conv3x3_split_pre(t.P, _wq(fmt, conv), conv.out_channels, **_slot_kw(fmt, t))
    return _launch(fmt, mode, "plain", conv, t, **_slot_kw(fmt, t))


def _pooled_unit(fmt, u, t, skipP, want_L, pooled_slots, mode, record=False):
    """An encoder block's second unit, which writes the skip slots into the concat buffer, the pooled tensor (slots, or fp32 for a
    fall-back level) and -- level 0 -- the fp32 tensor the caller receives.  "two-pass": plain convolution, then ONE BatchNorm + ReLU +
    2 x 2 max-pooling pass; "fused+pool": all of it in the convolution's launch, the same bits (no exact maximum is taken from it: the
    unit hands on its bound either way, so every later launch sees the same magnitude slots).  -> (skip, pooled, L | None)
    record (the unit in front of a pair level of a format with magnitude slots, "fused+pool"): the launch also records the exact
    maximum of its activation -- which is the maximum of the pooled tensor -- and the POOLED tensor hands that on as its amax, so the
    bound of the pair level's first unit starts from an exact maximum instead of chaining two bounds; the skip tensor, and with it
    every launch of this level and above, keeps the bound"""
    save = _coeffs(u.bn)
    scale = _bound(fmt, u.conv, save, t)
    B, _, H, _, W, _ = t.P.shape
    C, dev = u.conv.out_channels, t.P.device
    z = None if u.kind == "fused+pool" else _plain_conv(fmt, u.conv, t, mode)
    L = torch.empty((B, C, H, W), dtype=torch.float32, device=dev) if want_L else None
    yP = ops.p16_empty(B, C, H // 2, W // 2, dev, parts=fmt.parts) if pooled_slots else None
    yF = None if pooled_slots else torch.empty((B, C, H // 2, W // 2), dtype=torch.float32, device=dev)
    amax = ops.new_amax(dev) if record and fmt.magnitude and z is None and pooled_slots else None
    out_kw = dict(aP_slots=scale) if amax is None else dict(aP_slots=scale, a_amax=amax)
    if z is None:
        _launch(fmt, mode, "act_pool", u.conv, t, save, out=skipP, a=L, yP=yP, y=yF, **_slot_kw(fmt, t, **out_kw))
    elif not ops.bn_relu_apply_pool_split(z, save, skipP, L, yP, yF, slots=scale):
        raise RuntimeError("onet_amd: the BatchNorm + pooling pass refused a shape ops.eval_layer_ok accepted")
    if yF is not None and fmt.magnitude:
        ops.tag_amax(yF, scale)           # (max-pooling keeps the bound: the in-staging kernel below takes it as its range guard)
    return _T(skipP, None, scale, scale), _T(yP, yF, scale, scale if amax is None else amax), L


def _conv_t(fmt, lv, t, catP, C2):
    """ConvTranspose2d(k=2, s=2) + bias into the up-sampled channel groups of the pre-split concat buffer, by the launches lv.route names
    -> their magnitude slots (None on a format without: the weight pack of that many parts, no slots on either side)"""
    up = lv.up
    Ct = up.out_channels
    s_up = None
    if fmt.magnitude:
        s_up = ops.convT2x2_out_bound(up.weight, up.bias, _amax(t))
    dst = catP[:, C2 // 8:]
    packed = up.packed()
    route = _ROUTES[lv.route]
    if route.mode is not None:
        # (the row's binding in `ops`, read at call time as _launch does; the magnitude slots of a format that has them)
        name = ops.eval_convt_name(fmt.operands, route.mode)
        kw = dict(x_slots=t.scale, slots=s_up) if fmt.magnitude else {}
        if name is None or not getattr(ops, name)(t.P, packed.slots(fmt.parts), up.bias, dst, Ct, kind="convt_slot_fwd_kernel", **kw):
            raise RuntimeError(f"onet_amd: route {lv.route!r}: the {route.mode!r} slot-operand ConvTranspose2d of {fmt.operands} slots ({name}) "
                               f"refused a shape ops.{route.ok} accepted")
    elif lv.route == "pack":
        # (the smallest maps of the pass: the general kernel into an fp32 tensor, then one conversion pass -- what the training forward
        # does where the GEMM's fast path does not take the map.  An odd concat map of an any-map level takes the up-sampled tensor at
        # the reference's F.pad offsets, the pad strip zero: the kernel writes its 2h x 2w window alone)
        B, _, h, w = t.F.shape
        Ho, Wo = catP.shape[2], catP.shape[4]
        padded = (Ho, Wo) != (2 * h, 2 * w)
        y = (torch.zeros if padded else torch.empty)((B, Ct, Ho, Wo), dtype=torch.float32, device=t.F.device)
        ops.convT2x2_fwd(t.F, packed[0], up.bias, y, Ct, (Ho - 2 * h) // 2, (Wo - 2 * w) // 2)
        ops.split_pack_act(y, out=dst, slots=s_up)
    # ("gemm": the map has h w % 128 == 0 -- _up_edge -- so the fp32-operand GEMM's fast path takes it)
    elif not ops.convT2x2_fwd_p(t.F, packed[0], up.bias, dst, Ct, 0, 0, slots=s_up):
        raise RuntimeError("onet_amd: route 'gemm': the ConvTranspose2d GEMM refused the fp32 input of a fused level")
    return s_up


def _tail(unet, k, xk):
    """The levels the plan does not take, on the existing eval kernels: encoder output of level k (fp32) -> decoder output of level k"""
    _, downs, ups = _blocks(unet)
    if k == 4:
        return xk
    return ups[k](_tail(unet, k + 1, downs[k](xk)), xk)


def _head_unit(fmt, u, t, L, mode):
    """The last Conv-BatchNorm-ReLU unit with the head's channel product in the epilogue -> V [N, 1, H, W]"""
    return _launch(fmt, mode, "head", u.conv, t, _coeffs(u.bn), L, **_slot_kw(fmt, t))


def _unet_pass(plan, x):
    """One pass as `plan` (_build_plan; its reason is None) says -> (L = inc's output fp32, z = the last unit's pre-activation, save =
    its coefficients): the head forms relu(bn(z)) on load.
    plan.head (labels-only calls): the last unit ends in the fused launch -> V [N, 1, H, W] = sum_c L[c] relu(bn(z))[c]; z is never
    written and L is dropped with the pass."""
    res = _unet_pass_L(plan, x)
    return res[1] if plan.head else res


def _unet_pass_L(plan, x):
    """_unet_pass, the same launches, which on a plan.head pass hands back (L, V): inc's fp32 output, which the head launch has just
    read, for a caller that goes on to the loss (validate(want_loss=True))"""
    fmt, fused = plan.fmt, plan.levels[:plan.depth]
    N, _, H, W = x.shape
    catP, skips, L = [None] * 4, [None] * 4, None
    for k, lv in enumerate(fused):
        for u in lv.enc:
            if u.kind == "stem":
                t = _note(u.name, _stem_unit(fmt, u, x))
            elif u.kind == "fused":
                t = _note(u.name, _fused_unit(fmt, u, t, lv.mode))
            else:
                C = u.conv.out_channels
                catP[k] = ops.p16_empty(N, C + lv.up.out_channels, H >> k, W >> k, x.device, parts=fmt.parts)
                # (fp16 pair level below: its first unit's bound starts from this unit's exact record, see _pooled_unit)
                record = k + 1 < len(fused) and fused[k + 1].mode == "pairs"
                skips[k], t, Lk = _pooled_unit(fmt, u, t, catP[k][:, :C // 8], k == 0, lv.pooled_slots, lv.mode, record)
                _note(u.name, skips[k])
                if fmt.trace_pool and lv.pooled_slots:
                    _note(_ENC[k] + ".pool", t)
                if k == 0:
                    L = Lk
    if plan.depth < 5:
        # the levels below: existing eval kernels on fp32 tensors, from the pooled tensor of level d - 1
        t = _T(None, _tail(plan.unet, plan.depth, _blocks(plan.unet)[0][plan.depth](t.F)), None, None)
        t.amax = ops.amax_of(t.F) if fmt.magnitude else None
    z = save = None
    for k in range(len(fused) - 1, -1, -1):
        lv = fused[k]
        if not lv.dec:
            continue
        u1, u2 = lv.dec
        C = lv.enc[-1].conv.out_channels
        s_up = _conv_t(fmt, lv, t, catP[k], C)
        cat = _T(catP[k], None, (skips[k].scale, s_up, C), (skips[k].amax, s_up, C)) if fmt.magnitude else _T(catP[k])
        _note(_DEC[k] + ".up", _T(catP[k][:, C // 8:], None, s_up, s_up))
        t = _note(u1.name, _fused_unit(fmt, u1, cat, lv.mode))
        catP[k] = None
        if u2.kind == "fused":
            t = _note(u2.name, _fused_unit(fmt, u2, t, lv.mode))
        elif u2.kind == "fused+head":
            return L, _head_unit(fmt, u2, t, L, lv.mode)
        else:
            z, save = _plain_conv(fmt, u2.conv, t, lv.mode), _coeffs(u2.bn)
    return L, z, save


def _run(passes, twin, X, bias=None):
    """The passes of a gated call (_gate, _runs) -> [_unet_pass's result per pass].  bias None: a U-Net alone, one pass over X; an Onet:
    one pass over the twin batch [X ; clip(1 - X + bias)] (shared weights: in eval both halves take the same coefficients), or one
    over X and one over the complement."""
    return _run_passes(_unet_pass, passes, twin, X, bias)


def _run_passes(unet_pass, passes, twin, X, bias):
    """_run with the pass function of the caller's choice (_unet_pass | _unet_pass_L)"""
    X = X.contiguous()
    ops.amax_arena_reset(X.device)
    if bias is None:
        return [unet_pass(passes[0][1], X)]
    if twin:
        return [unet_pass(passes[0][1], ops.twin_materialize(src=(X, bias)))]
    first = unet_pass(passes[0][1], X)
    return [first, unet_pass(passes[-1][1], ops.complement_clip(X, bias))]


def unet_forward(unet, x):
    """UNet.forward's (x1, y1) by the fused plan, or None where the plan does not apply (the caller runs the existing path)."""
    passes, twin = _gate(unet, None, x=x)
    if not _runs(passes):
        return None
    (L, z, save), = _run(passes, twin, x)
    return L, ops.bn_relu_apply(z, save)


def _onet_halves(onet, X, head, cut):
    """-> [_unet_pass's result for X, for its complement] by the fused plan (head = "fused": the one that ends in the head-epilogue
    launch), or None where it does not apply.  cut(result, slice): a batch slice of a result, for the halves of the twin batch.
    Called with the model's settings active."""
    passes, twin = _gate(onet, None, head, x=X)
    if not _runs(passes) or (head == "fused" and not passes[0][1].head):
        return None
    res = _run(passes, twin, X, float(onet.bias))
    B = X.shape[0]
    return [cut(res[0], slice(0, B)), cut(res[0], slice(B, 2 * B))] if twin else res


def onet_forward(onet, X):
    """Onet.forward's (Lt, Vt, Ld, Vd, S) by the fused plan, or None where it does not apply.  Called with the model's settings active."""
    res = _onet_halves(onet, X, None, lambda r, s: (r[0][s], r[1][s], r[2]))
    if res is None:
        return None
    (Lt, zt, st), (Ld, zd, sd) = res
    Vt, Vd, S = ops.head_softmax_fwd(Lt, zt, Ld, zd, h_norm=(st, sd))
    return Lt, Vt, Ld, Vd, S


def _head_scores(onet, X):
    """(Vt, Vd) [B, 1, H, W] by the fused plan ending in the head-epilogue launch, or None where that does not apply (the caller runs
    the ordinary forward).  Called with the model's settings active, under no_grad."""
    return _onet_halves(onet, X, "fused", lambda V, s: V[s])


def scores(onet, X):
    """(Vt, Vd, S) of `X` -- the forward's outputs 1, 3 and 4, same shapes and dtypes -- under no_grad.  Where the fused plan applies
    (`onet.settings.fused_eval` on, eval mode, a last unit of 64 channels) the last convolution carries the head in its epilogue
    (ops.conv3x3_*_pre_head): the fp32 pre-activation of the last unit, the forward's largest tensor, is never written and the head
    kernel's read of it is gone; Vt / Vd then agree with the forward's to the rounding of a 64-term dot product (another, fixed,
    summation order).  Elsewhere: the ordinary forward's tensors, bit for bit."""
    with torch.no_grad():
        with ops.using(onet.settings):
            VV = _head_scores(onet, X)
            if VV is not None:
                S, _ = ops.softmax2_labels(VV[0], VV[1], want_S=True, want_labels=False)
                return VV[0], VV[1], S
        out = onet(X)
        return out[1], out[3], out[4]


def segment(onet, X, head=None):
    """int64 [B, H, W] labels of `X`: predict_label of the forward under no_grad (the fused plan when `onet.settings.fused_eval` is on
    and the model qualifies), without keeping the five outputs alive.
    head = "fused": the labels of scores(onet, X) -- the last convolution with the head in its epilogue, then one streaming launch that
    writes the labels alone: neither the last pre-activation nor S is materialised.  Where that plan does not apply: as head=None."""
    _check_head(head)
    with torch.no_grad():
        if head == "fused":
            with ops.using(onet.settings):
                VV = _head_scores(onet, X)
                if VV is not None:
                    return ops.softmax2_labels(VV[0], VV[1], want_S=False, want_labels=True)[1]
        S = onet(X)[4]
        return onet.predict_label(S)


# ----------------------------------------------------------------------------- the validation step
def _head_scores_L(onet, X):
    """_head_scores whose halves are (L, V): inc's fp32 output beside the scores, the same launches.  Called like _head_scores."""
    passes, twin = _gate(onet, None, "fused", x=X)
    if not _runs(passes) or not passes[0][1].head:
        return None
    res = _run_passes(_unet_pass_L, passes, twin, X, float(onet.bias))
    B = X.shape[0]
    return [tuple(t[:B] for t in res[0]), tuple(t[B:] for t in res[0])] if twin else res


class EvalCounts:
    """The confusion counts of a validation epoch, kept on the device: an int64 [capacity, 4] tensor of per-image (TP, FP, FN, TN),
    zeroed once, that validate(..., into=self) adds each batch's images to, and the host-side list of the batch sizes appended so far.
    rows() is the epoch's one device-to-host copy; metrics.epoch_metrics(rows, batch_sizes, protocol) does the rest on the host."""

    def __init__(self, capacity, device):
        self.counts = torch.zeros((int(capacity), 4), dtype=torch.int64, device=device)
        self.batch_sizes = []

    def __len__(self):
        return sum(self.batch_sizes)

    def reset(self):
        self.counts.zero_()
        self.batch_sizes = []

    def reserve(self, B):
        """-> the first of the B rows the next batch adds to"""
        row = len(self)
        if row + B > self.counts.shape[0]:
            raise ValueError(f"onet_amd: EvalCounts of {self.counts.shape[0]} images cannot take {B} more after {row}")
        self.batch_sizes.append(int(B))
        return row

    def rows(self):
        """int64 [images so far, 4] on the host"""
        return self.counts[:len(self)].cpu()


Validation = namedtuple("Validation", "counts labels S Vt Vd loss")


def _loss_value(Lt, St, Ld, Sd):
    """The value of Onet.compute_loss(Lt, St, Ld, Sd), composed from the JSD forward launches it makes (on the channel sums where Lt, Ld
    are the tagged halves of one twin forward, as there), without its NaN assertion: that would synchronise.  -> 1-element tensor"""
    tag_t, tag_d = getattr(Lt, "_onet_twin", None), getattr(Ld, "_onet_twin", None)
    if (tag_t is not None and tag_d is not None and tag_t[0] is tag_d[0] and tag_t[1] == 0 and tag_d[1] == 1
            and tag_t[2] == Lt._version and tag_d[2] == Ld._version and tag_t[0][0].shape[0] == 2 * Lt.shape[0]):
        top, _ = ops.jsd_fwd(None, St, Sd, sums=tag_t[0][1])
        dwn, _ = ops.jsd_fwd(None, Sd, St, sums=tag_t[0][2])
    else:
        top, _ = ops.jsd_fwd(Lt, St, Sd)
        dwn, _ = ops.jsd_fwd(Ld, Sd, St)
    return (-(top + dwn) / 2).reshape(1)


def validate(onet, X, gt, into=None, want_labels=False, want_S=False, want_loss=False):
    """One validation step on the device: the scores of `X` (the labels-only plan of scores / segment(head="fused") where it applies,
    the ordinary forward elsewhere), then ONE launch (ops.score_counts) that forms the labels and adds each image's confusion counts
    (TP, FP, FN, TN) against `gt` ([B, H, W] or [B, 1, H, W] in its own dtype: uint8 / bool, int32, int64, float32; positive where
    != 0) -- into rows of `into` (an EvalCounts) or, without one, of a fresh [B, 4] tensor.  Under no_grad, with the model's settings;
    no host synchronisation: everything returned is a device tensor.
    -> Validation(counts = the [B, 4] view of this batch's rows, labels int64 [B, H, W] | None, S [B, 2, H, W] | None, Vt, Vd, loss |
    None).  labels / S: written by the same launch where asked for -- labels bit-equal to segment(onet, X, head="fused") on the
    labels-only plan, to onet.predict_label(S) of the forward elsewhere.  want_loss: the value of onet.compute_loss(Lt, St, Ld, Sd) on
    this call's own L and S as a 1-element tensor (the labels-only plan hands inc's output back beside V; the NaN assertion of
    compute_loss, a synchronisation, is the caller's to make on the value)."""
    with torch.no_grad():
        B = X.shape[0]
        Lt = Ld = S_fwd = None
        with ops.using(onet.settings):
            res = _head_scores_L(onet, X) if want_loss else _head_scores(onet, X)
            if res is not None and want_loss:
                (Lt, Vt), (Ld, Vd) = res
            elif res is not None:
                Vt, Vd = res
        if res is None:
            Lt, Vt, Ld, Vd, S_fwd = onet(X)
        with ops.using(onet.settings):
            if into is None:
                counts, row = torch.zeros((B, 4), dtype=torch.int64, device=Vt.device), 0
            else:
                counts, row = into.counts, into.reserve(B)
            # (the forward's own S where there is one: the same bits, and nothing more to store)
            S, labels = ops.score_counts(Vt, Vd, gt, counts, row=row, want_S=(want_S or want_loss) and S_fwd is None, want_labels=want_labels)
            S = S_fwd if S is None else S
            loss = _loss_value(Lt, S[:, :1], Ld, S[:, 1:]) if want_loss else None
        return Validation(counts[row:row + B], labels, S if want_S else None, Vt, Vd, loss)


# ----------------------------------------------------------------------------- the performance report: SNR gain, two-stage cascade
class EvalSnr:
    """get_psnr's moments of a validation epoch, kept on the device beside an EvalCounts: an fp64 [capacity, 9] tensor whose rows
    verify_step(..., snr=self) writes, one per image (ops.snr_moments' layout), and the host-side list of the batch sizes so far.
    rows() is the epoch's one device-to-host copy; metrics.snr_report(rows, count rows, batch_sizes) does the rest on the host."""

    def __init__(self, capacity, device):
        self.moments = torch.zeros((int(capacity), 9), dtype=torch.float64, device=device)
        self.batch_sizes = []

    def __len__(self):
        return sum(self.batch_sizes)

    def reset(self):
        self.moments.zero_()
        self.batch_sizes = []

    def reserve(self, B):
        """-> the first of the B rows the next batch writes"""
        row = len(self)
        if row + B > self.moments.shape[0]:
            raise ValueError(f"onet_amd: EvalSnr of {self.moments.shape[0]} images cannot take {B} more after {row}")
        self.batch_sizes.append(int(B))
        return row

    def rows(self):
        """float64 [images so far, 9] on the host"""
        return self.moments[:len(self)].cpu()


Verification = namedtuple("Verification", "counts moments labels Vt Vd")


def verify_step(onet, X, gt, into=None, snr=None, want_labels=False):
    """One step of BOTH loops of the reference's performance report (verify_onet_simclutter, TS:420-454) on one forward:
    validate(onet, X, gt, into, want_labels) -- test_simclutter's part: the same forward, the same ops.score_counts launch, its counts
    and labels -- then ops.snr_moments on that forward's Vt, Vd: measure_snr_on_fg's part (TS:46-95), the sums and maxima get_psnr
    takes of X, n(Vt) and n(Vd), per image, into rows of `snr` (an EvalSnr) or, without one, of a fresh [B, 9] tensor.  Which of
    n(Vt) / n(Vd) is the foreground follows from the batch's counts: metrics.snr_report decides on the host, once per epoch.  `X`
    must be [B, 1, H, W] (get_psnr asserts img.shape == label.shape); `into` and `snr` must stand at the same row.  No host
    synchronisation: everything returned is a device tensor.
    -> Verification(counts [B, 4], moments = the fp64 [B, 9] view of this batch's rows, labels | None, Vt, Vd)"""
    if X.dim() != 4 or X.shape[1] != 1:
        raise ValueError(f"onet_amd: verify_step takes a one-channel [B, 1, H, W] input (get_psnr compares it with the label map), got {tuple(X.shape)}")
    if into is not None and snr is not None and len(into) != len(snr):
        raise ValueError(f"onet_amd: verify_step: the EvalCounts stands at row {len(into)}, the EvalSnr at row {len(snr)}")
    B = X.shape[0]
    if snr is not None and len(snr) + B > snr.moments.shape[0]:       # (before validate reserves its rows)
        raise ValueError(f"onet_amd: EvalSnr of {snr.moments.shape[0]} images cannot take {B} more after {len(snr)}")
    v = validate(onet, X, gt, into=into, want_labels=want_labels)
    with torch.no_grad():
        if snr is None:
            moments, row = torch.empty((B, 9), dtype=torch.float64, device=v.Vt.device), 0
        else:
            moments, row = snr.moments, snr.reserve(B)
        ops.snr_moments(X, v.Vt, v.Vd, gt, moments, row=row)
    return Verification(v.counts, moments[row:row + B], v.labels, v.Vt, v.Vd)


def cascade_input(Vt, Vd, counts):
    """The second stage's input of the two-stage cascade (TS:327-332), X2 [B, 1, H, W] = tensor_normal_per_frame of Vt where the hard
    re-assignment flips the batch's labels and of Vd where it keeps them, the decision read on the device from `counts` (the [B, 4]
    rows validate returned for this batch): no torch.equal, no host round trip in the middle of the batch."""
    with torch.no_grad():
        return ops.cascade_input(Vt, Vd, counts)


def verify_cascade(onet, onet2nd, X, gt, into=None, into2=None):
    """One batch of test_2nd_stage_simclutter (TS:312-345): validate(onet, X, gt, into), cascade_input of its Vt, Vd and counts,
    validate(onet2nd, X2, gt, into2) -- each model under its own settings, nothing synchronises.  metrics.cascade_metrics turns the
    two EvalCounts into the report.  -> (Validation of the first stage, Validation of the second)"""
    v1 = validate(onet, X, gt, into=into)
    v2 = validate(onet2nd, cascade_input(v1.Vt, v1.Vd, v1.counts), gt, into=into2)
    return v1, v2
