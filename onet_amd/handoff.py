"""The records through which the autograd Functions of the training path (functional.py) and the modules that wire them
(modules.py) hand state to each other outside autograd.  Every record has fixed fields (`slots=True`): a misspelt one raises
AttributeError instead of quietly skipping a fusion.  Who publishes and who takes what: DESIGN.md, "Hand-off records"."""
from __future__ import annotations

from dataclasses import dataclass, field

from . import ops


def same_tensor(a, b):
    """The one identity rule of the hand-offs: is `b`, the gradient autograd hands over, the tensor `a` its producer reduced (or
    wrote pre-split)?  Same pointer, shape and stride.  Every placeholder of a device shares the sentinel storage
    (ops.fp32_placeholder), so between placeholders this is a check of shape and stride."""
    return a.data_ptr() == b.data_ptr() and a.shape == b.shape and a.stride() == b.stride()


@dataclass(slots=True)
class GradHandoff:
    """Per backward: "whoever wrote this `da` already reduced it".  rec / rec4: the BatchNorm-backward reduce records of the unit
    whose activation gradient `da` is (from an fp32 input-gradient launch / a pre-split one, the pooling backward or the head);
    da_amax: max |da| slots; gl: the head's (g, L), from which the last unit forms its never-written da = g L on load."""
    da: object = None
    rec: object = None
    rec4: object = None
    da_amax: object = None
    gl: object = None

    def publish(self, da, *, rec=None, rec4=None, da_amax=None, gl=None):
        """Replaces the whole payload: a second backward through a retained graph publishes anew."""
        self.da, self.rec, self.rec4, self.da_amax, self.gl = da, rec, rec4, da_amax, gl

    def take(self, da, strict=False):
        """-> the payload (its own GradHandoff) if it was published for exactly `da` (same_tensor), else None; the hand-off is empty
        afterwards either way, and an empty one gives None.  strict (the head's hand-off: da = g L exists nowhere, so `da` must be
        the placeholder the head returned for it and there is no tensor to fall back on): anything else raises."""
        if self.da is None:
            return None
        got = GradHandoff(self.da, self.rec, self.rec4, self.da_amax, self.gl)
        self.publish(None)
        if same_tensor(got.da, da) and (not strict or ops.is_placeholder(da)):
            return got
        if strict:
            raise RuntimeError("onet_amd: the head kept the gradient of the last activation unwritten, but autograd handed its unit "
                               "another tensor (a second consumer of that activation?)")
        return None             # autograd handed over something else (another consumer, a hook): the unfused pass runs


@dataclass(slots=True)
class PoolRequest:
    """UNet._forward asks the unit that writes an encoder output for its max-pooled tensor too; p16: pre-split (else fp32)."""
    p16: bool = False


@dataclass(slots=True)
class Pooled:
    """The pooled tensor a unit's BatchNorm + ReLU pass wrote: y (fp32) or yP (pre-split); pre: by the pre-split branch, whose
    SkipPoolFn passes a placeholder on where only yP exists."""
    y: object = None
    yP: object = None
    pre: bool = False


@dataclass(slots=True)
class UnitLink:
    """A Conv-BatchNorm-ReLU unit -> the consumer of its activation: the next unit of its DoubleConv, or the SkipPoolFn of a block's
    output.  The consumer's side sets the requests before the unit runs (defer: normalise on load, write no activation); the unit
    publishes its pre-activation and coefficients (z, save; deferred + slots: the consumer applies them in its operand staging) and
    the pooled tensor; in backward the consumer's launch leaves the unit's reduce records in `grad`."""
    defer: bool = False
    want_pool: PoolRequest | None = None
    z: object = None
    save: object = None
    deferred: bool = False
    slots: object = None
    pooled: Pooled | None = None
    grad: GradHandoff = field(default_factory=GradHandoff)

    def take_requests(self):
        """-> (want_pool, defer), once: the unit reads them before it refills the link."""
        req = (self.want_pool, self.defer)
        self.want_pool, self.defer = None, False
        return req

    def publish(self, z, save, deferred=False, slots=None):
        """Everything an earlier pass left is gone."""
        self.z, self.save, self.deferred, self.slots, self.pooled = z, save, deferred, slots, None
        self.grad.publish(None)

    def take_below(self):
        """-> (z, save) or (None, None).  They become saved tensors of the taker's node, where every backward through a retained graph
        finds them and where they are freed with the graph; the link forgets them: it lives as long as the caller holds the loss,
        i.e. into the next step, and must not keep a whole set of pre-activations alive."""
        below = (self.z, self.save) if self.z is not None else (None, None)
        self.z = self.save = None
        return below

    def take_pooled(self):
        pooled, self.pooled = self.pooled, None
        return pooled


@dataclass(slots=True)
class UnitIO:
    """What travels beside one unit's tensors.  In: x_amax (magnitude slots x's producer left on it, ops.tag_amax); pre-split storage:
    xP / x_slots (the pre-split form of x: the unit's three convolution kernels then run on pre-split operands, ops.pre_layer_ok),
    want (write the activation pre-split; out: its destination, e.g. the skip groups of a concat buffer, else allocated), keep_fp32
    (the fp32 activation has readers too), up_link / head_link (the unit is the first of a decoder block / the network's last).
    Out: aP, a_slots (the pre-split activation and its scale slots), a_amax (magnitude slots of an fp32 activation)."""
    x_amax: object = None
    xP: object = None
    x_slots: object = None
    want: bool = False
    out: object = None
    keep_fp32: bool = False
    up_link: UpLink | None = None
    head_link: HeadLink | None = None
    aP: object = None
    a_slots: object = None
    a_amax: object = None

    @property
    def pre_split(self):
        """Does the unit take the pre-split branch (ConvBNReLUFn._forward_pre)?"""
        return self.xP is not None or bool(self.want)


@dataclass(slots=True)
class BlockOut:
    """Pre-split storage of a DoubleConv's output: out = its pre-split destination (None: allocated); keep_fp32: write fp32 too."""
    out: object = None
    keep_fp32: bool = False


@dataclass(slots=True)
class ConcatIO:
    """Up.forward -> UpConvTCatFn under pre-split storage: catP, the pre-split concat buffer (skip groups written by the encoder;
    no fp32 concat exists), the scale slots of its up-sampled groups, x1 pre-split by its producer, and the block's UpLink."""
    catP: object
    up_slots: object = None
    x1P: object = None
    x1_slots: object = None
    up_link: UpLink | None = None


@dataclass(slots=True)
class UpLink:
    """An Up's ConvTranspose2d <-> the first convolution of its DoubleConv.  want = (C2, Ct), set by the ConvTranspose2d's forward: that
    convolution's input gradient writes the up-sampled half pre-split; it persists, so that every backward of a retained graph makes
    the same hand-off.  Per backward: dyP, dy_slots (that half and its bound) and da, the input gradient they belong to."""
    want: tuple | None = None
    dyP: object = None
    dy_slots: object = None
    da: object = None

    def publish(self, dyP, dy_slots, da):
        self.dyP, self.dy_slots, self.da = dyP, dy_slots, da

    def take(self, dcat):
        """-> (dyP, dy_slots) if they were published for exactly `dcat`, else None; the payload is gone afterwards either way."""
        dyP, dy_slots, da = self.dyP, self.dy_slots, self.da
        self.publish(None, None, None)
        return (dyP, dy_slots) if (dyP is not None and da is not None and same_tensor(da, dcat)) else None


@dataclass(slots=True)
class HeadLink:
    """The network's last unit <-> the head.  Forward: the unit writes no activation and publishes z, save (the head normalises and
    rectifies z on load) and bwd_fuse (it can take dH = g L unwritten).  Backward: the head's records come back in `grad`, taken
    strictly."""
    z: object = None
    save: object = None
    bwd_fuse: bool = False
    grad: GradHandoff = field(default_factory=GradHandoff)

    def take_forward(self):
        """-> (z, save, bwd_fuse) or (None, None, False); the link forgets them (see UnitLink.take_below)."""
        got = (self.z, self.save, self.bwd_fuse) if self.z is not None else (None, None, False)
        self.z, self.save, self.bwd_fuse = None, None, False
        return got
