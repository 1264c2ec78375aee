"""The hand-off records of the training path (onet_amd/handoff.py) on CPU tensors: the identity rule, publish / take of the
per-backward payloads, what a link forgets and what it keeps, and that no record takes a misspelt field."""
import dataclasses

import pytest
import torch

from onet_amd import handoff as H


def test_same_tensor_is_pointer_shape_and_stride():
    t = torch.zeros(4, 6)
    assert H.same_tensor(t, t)
    assert H.same_tensor(t, t.detach())                 # another object over the same memory, shape and stride
    assert H.same_tensor(t, t[:, :])                    # ... and a view that is all of it
    assert not H.same_tensor(t, t.view(6, 4))           # another shape at the same pointer
    assert not H.same_tensor(t, t[:, :3])               # a narrower view at the same pointer
    assert not H.same_tensor(t[:2, :3], t.t()[:2, :3])  # the same pointer and shape, another stride
    assert not H.same_tensor(t, t[1:])                  # another pointer
    assert not H.same_tensor(t, torch.zeros(4, 6))      # another tensor, equal in everything else


def test_grad_handoff_publish_and_take():
    da, other = torch.zeros(2, 3), torch.zeros(2, 3)
    h = H.GradHandoff()
    assert h.take(da) is None                           # empty
    h.publish(da, rec="r", da_amax="m")
    got = h.take(da)
    assert (got.da is da, got.rec, got.rec4, got.da_amax, got.gl) == (True, "r", None, "m", None)
    assert h.take(da) is None and h.da is None and h.rec is None        # taken once
    h.publish(da, rec4="r4")
    assert h.take(other) is None                        # another tensor: refused ...
    assert h.da is None and h.rec4 is None and h.take(da) is None       # ... and emptied all the same
    h.publish(other, rec="first", rec4="first4")
    h.publish(da, rec="last")                           # a second backward publishes anew: the whole payload is replaced
    got = h.take(da)
    assert (got.rec, got.rec4) == ("last", None)


def test_strict_take_raises_on_a_cpu_tensor_and_empties():
    da = torch.zeros(2, 3)
    h = H.GradHandoff()
    assert h.take(da, strict=True) is None              # empty: nothing to insist on
    h.publish(da, rec4="r4", gl=("g", "L"))
    with pytest.raises(RuntimeError, match="another tensor"):
        h.take(da, strict=True)                         # the same tensor, but no placeholder of the head's
    assert h.gl is None and h.take(da, strict=True) is None


def test_unit_link_requests_and_below():
    z, save = torch.zeros(1), torch.zeros(4)
    lk = H.UnitLink(defer=True, want_pool=H.PoolRequest(p16=True))
    want_pool, defer = lk.take_requests()
    assert want_pool.p16 is True and defer is True
    assert lk.take_requests() == (None, False)
    assert lk.take_below() == (None, None)
    lk.pooled = H.Pooled(y=z)
    lk.grad.publish(z, rec="stale")
    lk.publish(z, save, deferred=True, slots="s")
    assert lk.pooled is None and lk.grad.da is None     # what an earlier pass left is gone
    assert (lk.z is z, lk.save is save, lk.deferred, lk.slots) == (True, True, True, "s")
    below = lk.take_below()
    assert below[0] is z and below[1] is save
    assert lk.z is None and lk.save is None and lk.take_below() == (None, None)
    lk.pooled = H.Pooled(yP="P", pre=True)
    assert lk.take_pooled().yP == "P" and lk.take_pooled() is None


def test_up_link_keeps_the_request():
    dcat = torch.zeros(2, 4)
    up = H.UpLink()
    up.want = (8, 8)
    assert up.take(dcat) is None
    up.publish("dyP", "slots", dcat)
    assert up.take(dcat) == ("dyP", "slots")
    assert up.take(dcat) is None and up.want == (8, 8)
    up.publish("dyP", "slots", dcat)
    assert up.take(dcat.t()) is None                    # same pointer, another shape and stride
    assert up.dyP is None and up.da is None and up.want == (8, 8)
    up.publish("dyP", "slots", dcat.view(4, 2).t())
    assert up.take(dcat) is None                        # same pointer and shape, another stride


def test_head_link_forward_is_taken_once():
    z = torch.zeros(1)
    hl = H.HeadLink()
    assert hl.take_forward() == (None, None, False)
    hl.z, hl.save, hl.bwd_fuse = z, "save", True
    assert hl.take_forward() == (z, "save", True)
    assert hl.take_forward() == (None, None, False)


RECORDS = (H.GradHandoff, H.PoolRequest, H.Pooled, H.UnitLink, H.UnitIO, H.BlockOut, H.UpLink, H.HeadLink,
           lambda: H.ConcatIO(catP=None))


@pytest.mark.parametrize("make", RECORDS)
def test_a_misspelt_field_raises(make):
    rec = make()
    for f in dataclasses.fields(rec):
        setattr(rec, f.name, getattr(rec, f.name))      # every declared field takes a value
    for name in ("da_max", "rec_4", "want_pol", "deffered", "x_slot", "keep_f32", "cat_P", "dy_slot", "bwd_fused", "p_16"):
        with pytest.raises(AttributeError):
            setattr(rec, name, 1)


@pytest.mark.parametrize("xP, want, pre", [(None, False, False), (None, True, True), ("P", False, True), ("P", True, True)])
def test_unit_io_pre_split(xP, want, pre):
    assert H.UnitIO(xP=xP, want=want).pre_split is pre
    assert H.UnitIO().pre_split is False
