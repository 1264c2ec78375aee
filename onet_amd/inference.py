"""Fused eval-mode inference (Settings.fused_eval): a straight-line forward plan on the pre-split kernels.

In eval BatchNorm is a fixed per-channel affine map, so `relu(bn(z))` rides in the convolution's epilogue and the activation leaves
the convolution as 16-byte slots (ops.conv3x3_split_pre_act): no pre-activation tensor, no BatchNorm pass, half the HBM bytes per
activation element of the default eval path.  No autograd Function is involved: the plan reads the module tree's parameters and
buffers and calls `ops` directly.

Every tensor kept as slots carries two sets of magnitude slots:
  scale   an upper BOUND of max |a|, known before the launch that writes the tensor (ops.conv3x3_act_bound from the weights, the
          coefficients and the input's magnitude; ops.convT2x2_out_bound): the fp16 parts are those of 2^k a with the guard k these
          slots select, and the consumers undo 2^k from the same slots;
  amax    the EXACT max |a| the fused epilogue recorded -- what the next layer's bound starts from, so that the looseness of a bound
          never exceeds one convolution (one ConvTranspose2d + one convolution behind a ConvTranspose2d).  Producers without an
          exact record (the stem's and the pooled units' BatchNorm passes) hand their bound on: at most three bounds chain
          (measured: 56-183x per convolution, up to 1.4e4x where two chain -- profiles/r07_fused_eval.md).

Levels: level k is the part of the U-Net on maps of H / 2^k x W / 2^k.  The plan is fused down to depth d, the deepest level all of
whose layers ops.eval_layer_ok accepts; the levels below run the existing eval kernels on fp32 tensors (the pooled tensor of level
d - 1 is written as fp32 going down, ops.convT2x2_fwd_p writes slots coming back up).

Settings.fused_eval = "bf16" runs the same plan on ONE part of plain bf16 per slot (ops.conv3x3_plain16_pre_act; layer predicate
ops.eval_layer_ok_bf16): the operands conv == "bf16" trains with, one MFMA per product term instead of three and 2-byte slot elements.
bf16 has fp32's exponent range, so that plan carries no magnitude slots at all: scale = amax = None on every tensor, no bound launches.

Labels-only calls (scores, segment(head="fused")): the same plan on either slot format, ending in ONE launch for the last unit and the
head's channel product (ops.conv3x3_plain16_pre_head / conv3x3_split_pre_head: relu(bn(.)) on the accumulators, times L, summed over
the unit's 64 channels, V the only store) followed by ops.softmax2_labels.  The last unit's fp32 pre-activation -- the largest tensor
of the forward -- is never written, the head kernel does not run, and segment does not materialise S.  Onet.forward does not take this
route: under every setting it launches what it launched before these calls existed."""
from __future__ import annotations

import torch

from . import ops


def _blocks(unet):
    """-> (encoder DoubleConvs by level 0 .. 4, Down modules by level 1 .. 4, Up modules by level 0 .. 3)"""
    downs = (unet.down1, unet.down2, unet.down3, unet.down4)
    enc = (unet.inc,) + tuple(d.maxpool_conv[1] for d in downs)
    return enc, downs, (unet.up4, unet.up3, unet.up2, unet.up1)


def _units(blk):
    s = blk.double_conv
    return s[0], s[1], s[3], s[4]


def _static_reason(unet):
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
    if _parts() == 1:
        if not ops.presplit():
            return "pre-split storage is off under the effective convolution algorithm"
    elif not (ops.presplit() and ops.p16_parts() == 2):
        return "the effective convolution algorithm is not the fp16-split one with pre-split storage"
    return None


def _parts():
    """Parts per slot of the active plan: 2 = fp16 (hi | mid), 1 = plain bf16 (Settings.fused_eval = "bf16")"""
    return 1 if ops.fused_eval_operands() == "bf16" else 2


def _level_layers(unet):
    """-> [level] -> [(name, conv)] of the 3x3 convolutions on that level's maps that the plan runs on pre-split operands"""
    enc, _, ups = _blocks(unet)
    names = ("inc", "down1", "down2", "down3", "down4")
    unames = ("up4", "up3", "up2", "up1")
    out = []
    for k in range(5):
        c1, _, c2, _ = _units(enc[k])
        lv = [(names[k] + ".c2", c2)] if k == 0 else [(names[k] + ".c1", c1), (names[k] + ".c2", c2)]
        if k < 4:
            d1, _, d2, _ = _units(ups[k].conv)
            lv += [(unames[k] + ".c1", d1), (unames[k] + ".c2", d2)]
        out.append(lv)
    return out


def _depth(unet, N, H, W):
    """-> (d, why level d is not fused | None): levels 0 .. d - 1 are fused"""
    enc, _, ups = _blocks(unet)
    levels = _level_layers(unet)
    layer_ok = ops.eval_layer_ok_bf16 if _parts() == 1 else ops.eval_layer_ok
    for k in range(5):
        if (H % (1 << k)) or (W % (1 << k)):
            return k, f"level {k}: the input size is not a multiple of {1 << k}"
        h, w = H >> k, W >> k
        for name, conv in levels[k]:
            if not layer_ok(N, conv.in_channels, conv.out_channels, h, w):
                return k, f"level {k}: {name} ({conv.in_channels} -> {conv.out_channels} on {N} maps of {h} x {w}) is outside ops.{layer_ok.__name__}"
        if k < 4:
            C = _units(enc[k])[2].out_channels
            d1 = _units(ups[k].conv)[0]
            if C % 32 or d1.in_channels != C + ups[k].up.out_channels or ups[k].up.out_channels % 8:
                return k, f"level {k}: the concat buffer's channel groups do not fit the slot layout"
    return 5, None


def _head_ok(unet):
    """Does the last unit fit the convolution with the head epilogue (ops.conv3x3_*_pre_head: one 64-channel tile per pixel)?"""
    return _units(_blocks(unet)[2][0].conv)[2].out_channels == 64


def unet_plan(unet, shape, device=None, head=None):
    """What the fused plan does with a U-Net pass over an input of `shape` = (N, C, H, W): a pure query, nothing is launched.
    -> {"fused": bool, "reason": why not | None, "depth": d, "batch": N, "layers": {name: "stem" | "fused" | "two-pass" | "plain+head"
    | "fused+head" | "fallback"}, "convt": {name: "slots" | "fp32->slots" | "fallback"}, "fallback_reason": why level d is not fused |
    None, "operands": the slot format the settings select, "fp16x2" | "bf16" (None: Settings.fused_eval is off)}
    head = "fused": the plan of the labels-only calls (scores, segment(head="fused")) -- "fused+head" where the last unit runs with the
    head in its epilogue; a last unit outside that kernel's domain (Cout != 64) sends those calls to the ordinary forward, whose plan
    this then is ("plain+head")."""
    if head not in (None, "fused"):
        raise ValueError(f"onet_amd: head must be None or 'fused', not {head!r}")
    out = {"fused": False, "reason": None, "depth": 0, "batch": int(shape[0]) if len(shape) == 4 else 0, "layers": {}, "convt": {},
           "fallback_reason": None, "operands": ops.fused_eval_operands()}
    if len(shape) != 4:
        out["reason"] = "the input is not 4-D"
        return out
    dev = device if device is not None else next(unet.parameters()).device
    if dev.type != "cuda":
        out["reason"] = "the model is not on a GPU"
        return out
    if not ops.fused_eval():
        out["reason"] = "Settings.fused_eval is off"
        return out
    why = _static_reason(unet)
    if why is not None:
        out["reason"] = why
        return out
    N, C, H, W = (int(v) for v in shape)
    if C != unet.inc.double_conv[0].in_channels or N <= 0:
        out["reason"] = "the input's channels do not match the stem"
        return out
    with torch.cuda.device(dev):
        d, why_d = _depth(unet, N, H, W)
    out["depth"], out["fallback_reason"] = d, why_d
    if d == 0:
        out["reason"] = why_d
        return out
    out["fused"] = True
    _, _, ups = _blocks(unet)
    unames = ("up4", "up3", "up2", "up1")
    out["layers"]["inc.c1"] = "stem"
    for k, lv in enumerate(_level_layers(unet)):
        for name, _ in lv:
            if k >= d:
                kind = "fallback"
            elif name == "up4.c2":
                kind = "fused+head" if head == "fused" and _head_ok(unet) else "plain+head"
            elif name.endswith(".c2") and name[:2] != "up" and k < 4:
                kind = "two-pass"             # pooled units: plain convolution + BatchNorm / ReLU / pooling pass writing slots
            else:
                kind = "fused"
            out["layers"][name] = kind
    for k in range(4):
        up = ups[k].up
        if k >= d:
            out["convt"][unames[k]] = "fallback"
        elif k + 1 < d and ops.convt_slots_ok(N, up.in_channels, up.out_channels, H >> (k + 1), W >> (k + 1), parts=_parts()):
            out["convt"][unames[k]] = "slots"
        else:
            out["convt"][unames[k]] = "fp32->slots"
    return out


def fused_eval_plan(model, shape, head=None):
    """What `model(X)` does with an input of `shape` (B, C, H, W) under its settings: see unet_plan.  For an Onet the batch through
    each U-Net is 2 B when the weights are shared and the twin batch is on ("twin": True), B otherwise (two passes).
    head = "fused": what scores(model, X) / segment(model, X, head="fused") do instead ("fused+head" for up4.c2 where the fused launch
    runs; both U-Nets of an unshared model must qualify).
    The answer holds for the model's device: ops.eval_layer_ok follows the convolution dispatch, which asks for enough tiles to fill
    that device's compute units, so the fused depth of a small batch can differ between devices."""
    from .modules import Onet
    if head not in (None, "fused"):
        raise ValueError(f"onet_amd: head must be None or 'fused', not {head!r}")
    if not isinstance(model, Onet):
        return unet_plan(model, tuple(shape))
    with ops.using(model.settings):
        twin = model.dwnu is model.topu and ops.twin_enabled()
        shp = tuple(shape)
        if len(shp) == 4 and twin:
            shp = (2 * shp[0],) + shp[1:]
        if head == "fused" and not (_head_ok(model.topu) and _head_ok(model.dwnu)):
            head = None
        plan = unet_plan(model.topu, shp, head=head)
        plan["twin"] = bool(twin)
        if plan["fused"] and model.dwnu is not model.topu:
            other = unet_plan(model.dwnu, shp, head=head)
            if not other["fused"]:
                plan.update(fused=False, reason="dwnu: " + str(other["reason"]), depth=0)
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


def _bound(conv, save, t):
    s1, s2, ch = ops._slots3(t.amax)
    return ops.conv3x3_act_bound(conv.weight, save, s1, s2, ch)


def _wq(conv, parts=2):
    return conv.packed().get_pack("split" if parts == 2 else "plain16")[0]


def _fused_unit(conv, bn, t, keep_fp32=False):
    """Conv-BatchNorm-ReLU in one launch, output as slots (+ fp32 when another reader needs it)"""
    save = _coeffs(bn)
    if t.P.shape[3] == 1:             # plain bf16: unscaled, nothing to bound or record
        B, _, H, _, W, _ = t.P.shape
        a = torch.empty((B, conv.out_channels, H, W), dtype=torch.float32, device=t.P.device) if keep_fp32 else None
        aP = ops.conv3x3_plain16_pre_act(t.P, _wq(conv, 1), conv.out_channels, save, a=a)
        if aP is None:
            raise RuntimeError("onet_amd: the fused eval kernel refused a shape ops.eval_layer_ok_bf16 accepted")
        return _T(aP, a)
    scale = _bound(conv, save, t)
    B, _, H, _, W, _ = t.P.shape
    amax = ops.new_amax(t.P.device)
    a = torch.empty((B, conv.out_channels, H, W), dtype=torch.float32, device=t.P.device) if keep_fp32 else None
    s1, s2, ch = ops._slots3(t.scale)
    aP = ops.conv3x3_split_pre_act(t.P, _wq(conv), conv.out_channels, save, scale, slots=s1, slots2=s2, split_ch=ch, a_amax=amax, a=a)
    if aP is None:
        raise RuntimeError("onet_amd: the fused eval kernel refused a shape ops.eval_layer_ok accepted")
    return _T(aP, a, scale, amax)


def _plain_conv(conv, t):
    if t.P.shape[3] == 1:
        return ops.conv3x3_split_pre(t.P, _wq(conv, 1), conv.out_channels)
    s1, s2, ch = ops._slots3(t.scale)
    return ops.conv3x3_split_pre(t.P, _wq(conv), conv.out_channels, slots=s1, slots2=s2, split_ch=ch)


def _pooled_unit(conv, bn, t, skipP, want_L, pooled_slots):
    """An encoder block's second unit: plain convolution, then ONE BatchNorm + ReLU + 2 x 2 max-pooling pass that writes the skip slots
    into the concat buffer, the pooled tensor (slots, or fp32 for a fall-back level) and -- level 0 -- the fp32 tensor the caller
    receives.  -> (skip, pooled, L | None)"""
    save = _coeffs(bn)
    parts = t.P.shape[3]
    scale = _bound(conv, save, t) if parts == 2 else None
    z = _plain_conv(conv, t)
    B, C, H, W = z.shape
    L = torch.empty_like(z) if want_L else None
    yP = ops.p16_empty(B, C, H // 2, W // 2, z.device, parts=parts) if pooled_slots else None
    yF = None if pooled_slots else torch.empty((B, C, H // 2, W // 2), dtype=torch.float32, device=z.device)
    if not ops.bn_relu_apply_pool_split(z, save, skipP, L, yP, yF, slots=scale):
        raise RuntimeError("onet_amd: the BatchNorm + pooling pass refused a shape ops.eval_layer_ok accepted")
    if yF is not None and scale is not None:
        ops.tag_amax(yF, scale)           # (max-pooling keeps the bound: the in-staging kernel below takes it as its range guard)
    return _T(skipP, None, scale, scale), _T(yP, yF, scale, scale), L


def _conv_t(up, t, catP, C2):
    """ConvTranspose2d(k=2, s=2) + bias into the up-sampled channel groups of the pre-split concat buffer -> their magnitude slots"""
    Ct = up.out_channels
    if catP.shape[3] == 1:            # plain bf16: the one-part weight pack, no magnitude slots on either side
        dst = catP[:, C2 // 8:]
        packed = up.packed()
        if t.P is not None and ops.convT2x2_fwd_slots(t.P, packed.slots(1), up.bias, dst, Ct, kind="convt_slot_fwd_kernel"):
            return None
        if t.F is None:
            raise RuntimeError("onet_amd: the slot-operand ConvTranspose2d refused a shape ops.convt_slots_ok accepted")
        if not ops.convT2x2_fwd_p(t.F, packed[0], up.bias, dst, Ct, 0, 0):
            raise RuntimeError("onet_amd: the ConvTranspose2d GEMM refused the fp32 input of a fused level")
        return None
    x_amax = t.amax if t.amax is not None else ops.absmax_slots(t.F)
    s_up = ops.convT2x2_out_bound(up.weight, up.bias, x_amax)
    dst = catP[:, C2 // 8:]
    packed = up.packed()
    if t.P is not None and ops.convT2x2_fwd_slots(t.P, packed.slots(2), up.bias, dst, Ct, x_slots=t.scale, slots=s_up,
                                                   kind="convt_slot_fwd_kernel"):
        return s_up
    if t.F is None:
        raise RuntimeError("onet_amd: the slot-operand ConvTranspose2d refused a shape ops.convt_slots_ok accepted")
    # (a fused level is made of full 16 x 32 tiles, so the map below it has h w % 128 == 0: the GEMM's fast path takes it)
    if not ops.convT2x2_fwd_p(t.F, packed[0], up.bias, dst, Ct, 0, 0, slots=s_up):
        raise RuntimeError("onet_amd: the ConvTranspose2d GEMM refused the fp32 input of a fused level")
    return s_up


def _tail(unet, k, xk):
    """The levels the plan does not take, on the existing eval kernels: encoder output of level k (fp32) -> decoder output of level k"""
    _, downs, ups = _blocks(unet)
    if k == 4:
        return xk
    return ups[k](_tail(unet, k + 1, downs[k](xk)), xk)


def _head_unit(conv, bn, t, L):
    """The last Conv-BatchNorm-ReLU unit with the head's channel product in the epilogue -> V [N, 1, H, W]"""
    save = _coeffs(bn)
    if t.P.shape[3] == 1:
        V = ops.conv3x3_plain16_pre_head(t.P, _wq(conv, 1), conv.out_channels, save, L)
    else:
        s1, s2, ch = ops._slots3(t.scale)
        V = ops.conv3x3_split_pre_head(t.P, _wq(conv), conv.out_channels, save, L, slots=s1, slots2=s2, split_ch=ch)
    if V is None:
        raise RuntimeError("onet_amd: the fused head kernel refused a shape the plan accepted")
    return V


def _unet_pass(unet, x, d, head=False):
    """-> (L = inc's output fp32, z = the last unit's pre-activation, save = its coefficients): the head forms relu(bn(z)) on load.
    head=True (labels-only calls; the caller has checked _head_ok): the last unit ends in the fused launch -> V [N, 1, H, W] =
    sum_c L[c] relu(bn(z))[c]; z is never written and L is dropped with the pass."""
    enc, downs, ups = _blocks(unet)
    N, _, H, W = x.shape
    dev = x.device
    # stem: the existing direct kernel, then one BatchNorm + ReLU pass that writes slots
    c1, b1, c2, b2 = _units(enc[0])
    P = _parts()
    z0 = ops.conv3x3_auto(x, c1.packed(), 0)
    save0 = _coeffs(b1)
    scale0 = _bound(c1, save0, _T(None, x, None, ops.absmax_slots(x))) if P == 2 else None
    a0 = ops.p16_empty(N, c1.out_channels, H, W, dev, parts=P)
    ops.bn_relu_apply_split(z0, save0, a0, slots=scale0)
    del z0
    t = _note("inc.c1", _T(a0, None, scale0, scale0))
    names, unames = ("inc", "down1", "down2", "down3", "down4"), ("up4", "up3", "up2", "up1")
    catP, skips, L = [None] * 4, [None] * 4, None
    for k in range(d):
        c1, b1, c2, b2 = _units(enc[k])
        if k > 0:
            t = _note(names[k] + ".c1", _fused_unit(c1, b1, t))
        if k == 4:
            up = ups[3].up
            t = _note("down4.c2", _fused_unit(c2, b2, t, keep_fp32=not ops.convt_slots_ok(N, up.in_channels, up.out_channels, H >> 4, W >> 4, parts=P)))
            break
        C = c2.out_channels
        catP[k] = ops.p16_empty(N, C + ups[k].up.out_channels, H >> k, W >> k, dev, parts=P)
        skips[k], t, Lk = _pooled_unit(c2, b2, t, catP[k][:, :C // 8], k == 0, k + 1 < d)
        _note(names[k] + ".c2", skips[k])
        if P == 1 and t.P is not None:
            _note(names[k] + ".pool", t)          # (the one-part plan's trace is complete: every convolution's exact input can be rebuilt)
        if k == 0:
            L = Lk
    if d < 5:
        # the levels below: existing eval kernels on fp32 tensors, from the pooled tensor of level d - 1
        t = _T(None, _tail(unet, d, enc[d](t.F)), None, None)
        t.amax = ops.amax_of(t.F) if P == 2 else None
    z = save = None
    for k in range(min(d, 4) - 1, -1, -1):
        C = _units(enc[k])[2].out_channels
        s_up = _conv_t(ups[k].up, t, catP[k], C)
        cat = _T(catP[k], None, (skips[k].scale, s_up, C), (skips[k].amax, s_up, C)) if P == 2 else _T(catP[k])
        c1, b1, c2, b2 = _units(ups[k].conv)
        _note(unames[k] + ".up", _T(catP[k][:, C // 8:], None, s_up, s_up))
        t = _note(unames[k] + ".c1", _fused_unit(c1, b1, cat))
        catP[k] = None
        if k > 0:
            up = ups[k - 1].up
            t = _note(unames[k] + ".c2", _fused_unit(c2, b2, t, keep_fp32=not ops.convt_slots_ok(N, up.in_channels, up.out_channels, H >> k, W >> k, parts=P)))
        elif head:
            return _head_unit(c2, b2, t, L)
        else:
            z, save = _plain_conv(c2, t), _coeffs(b2)
    return L, z, save


def unet_forward(unet, x):
    """UNet.forward's (x1, y1) by the fused plan, or None where the plan does not apply (the caller runs the existing path)."""
    if not (ops.fused_eval() and not torch.is_grad_enabled() and _input_ok(x)) or _static_reason(unet) is not None:
        return None
    if x.shape[1] != unet.inc.double_conv[0].in_channels:
        return None
    d, _ = _depth(unet, x.shape[0], x.shape[2], x.shape[3])
    if d == 0:
        return None
    x = x.contiguous()
    ops.amax_arena_reset(x.device)
    L, z, save = _unet_pass(unet, x, d)
    return L, ops.bn_relu_apply(z, save)


def onet_forward(onet, X):
    """Onet.forward's (Lt, Vt, Ld, Vd, S) by the fused plan, or None where it does not apply.  Called with the model's settings active."""
    if not (ops.fused_eval() and not onet.training and not torch.is_grad_enabled() and _input_ok(X)):
        return None
    shared = onet.dwnu is onet.topu
    twin = shared and ops.twin_enabled()
    B, C, H, W = X.shape
    N = 2 * B if twin else B
    for u in ((onet.topu,) if shared else (onet.topu, onet.dwnu)):
        if _static_reason(u) is not None or C != u.inc.double_conv[0].in_channels or _depth(u, N, H, W)[0] == 0:
            return None
    X = X.contiguous()
    ops.amax_arena_reset(X.device)
    if twin:
        # shared weights: [X ; clip(1 - X + bias)] as one batch of 2B -- in eval both halves take the same coefficients
        XX = ops.twin_materialize(src=(X, float(onet.bias)))
        L, z, save = _unet_pass(onet.topu, XX, _depth(onet.topu, N, H, W)[0])
        Vt, Vd, S = ops.head_softmax_fwd(L[:B], z[:B], L[B:], z[B:], h_norm=(save, save))
        return L[:B], Vt, L[B:], Vd, S
    Lt, zt, st = _unet_pass(onet.topu, X, _depth(onet.topu, N, H, W)[0])
    Xd = ops.complement_clip(X, float(onet.bias))
    Ld, zd, sd = _unet_pass(onet.dwnu, Xd, _depth(onet.dwnu, N, H, W)[0])
    Vt, Vd, S = ops.head_softmax_fwd(Lt, zt, Ld, zd, h_norm=(st, sd))
    return Lt, Vt, Ld, Vd, S


def _head_scores(onet, X):
    """(Vt, Vd) [B, 1, H, W] by the fused plan ending in the head-epilogue launch, or None where that does not apply (the caller runs
    the ordinary forward).  Called with the model's settings active, under no_grad."""
    if not (ops.fused_eval() and not onet.training and not torch.is_grad_enabled() and _input_ok(X)):
        return None
    shared = onet.dwnu is onet.topu
    twin = shared and ops.twin_enabled()
    B, C, H, W = X.shape
    N = 2 * B if twin else B
    for u in ((onet.topu,) if shared else (onet.topu, onet.dwnu)):
        if _static_reason(u) is not None or C != u.inc.double_conv[0].in_channels or _depth(u, N, H, W)[0] == 0 or not _head_ok(u):
            return None
    X = X.contiguous()
    ops.amax_arena_reset(X.device)
    if twin:
        XX = ops.twin_materialize(src=(X, float(onet.bias)))
        V = _unet_pass(onet.topu, XX, _depth(onet.topu, N, H, W)[0], head=True)
        return V[:B], V[B:]
    Vt = _unet_pass(onet.topu, X, _depth(onet.topu, N, H, W)[0], head=True)
    Xd = ops.complement_clip(X, float(onet.bias))
    Vd = _unet_pass(onet.dwnu, Xd, _depth(onet.dwnu, N, H, W)[0], head=True)
    return Vt, Vd


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
    if head not in (None, "fused"):
        raise ValueError(f"onet_amd.segment: head must be None or 'fused', not {head!r}")
    with torch.no_grad():
        if head == "fused":
            with ops.using(onet.settings):
                VV = _head_scores(onet, X)
                if VV is not None:
                    return ops.softmax2_labels(VV[0], VV[1], want_S=False, want_labels=True)[1]
        S = onet(X)[4]
        return onet.predict_label(S)
