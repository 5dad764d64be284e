"""Routing of a layer's / a lane set's parameter gradients (engine/handover.py, HO.submit) with stub kernels: no GPU.  What
leaves submit is what _run_param_grads and ConvOp.wgrad_spec consume — (op, dc, x, gw, gb, nb, pro), or ("lanes", [those])."""
import pytest
import torch
import torch.nn as nn

from fsnet_amd.engine import handover
from fsnet_amd.engine.handover import HO
from fsnet_amd.engine.nets import ConvLayer


class _Op:
    def __init__(self, name):
        self.name = name

    def wgrad_spec(self, dc, x, gw, pro=None):
        return (self.name, dc, x, gw, pro)


@pytest.fixture
def calls(monkeypatch):
    """stub kernels: every launch is recorded instead"""
    rec = {"specs": [], "sums": []}
    monkeypatch.setattr(handover, "run_specs", lambda specs: rec["specs"].append(list(specs)))
    monkeypatch.setattr(handover.ops, "channel_sum", lambda dc, gb, nb: rec["sums"].append((dc, gb, nb)))
    HO._reset_pass()
    yield rec
    HO._reset_pass()


def _layer(bias=True, train_weight=True, co=3):
    conv = nn.Conv2d(2, co, 3, bias=bias)
    conv.weight.requires_grad_(train_weight)
    return ConvLayer(conv)


def test_frozen_weight_with_a_trainable_bias_takes_only_the_channel_sum(calls):
    cl, dc, x = _layer(train_weight=False), torch.ones(1, 4, 4, 3), torch.ones(1, 6, 6, 2)
    cl.accumulate_param_grads(_Op("a"), dc, x)
    assert calls["specs"] == []
    assert len(calls["sums"]) == 1
    got = calls["sums"][0]
    assert got[0] is dc and got[1] is cl.m.bias.grad and got[2] == 3
    # ... and as one lane among trained ones: its sum at once, the others' launch without it
    other = _layer(bias=False)
    HO.submit([(cl, _Op("a"), dc, x, None), (other, _Op("b"), dc, x, "pro")])
    assert len(calls["sums"]) == 2 and calls["sums"][1][1] is cl.m.bias.grad
    assert calls["specs"] == [[("b", dc, x, other.m.weight.grad, "pro")]]
    # a layer with nothing to train: nothing at all
    calls["specs"].clear()
    frozen = _layer(bias=False, train_weight=False)
    frozen.accumulate_param_grads(_Op("c"), dc, x)
    assert calls["specs"] == [] and len(calls["sums"]) == 2


def test_one_lane_and_several_lanes_run_inline_as_one_launch_each(calls):
    dc, x = torch.ones(1, 4, 4, 3), torch.ones(1, 6, 6, 2)
    a, b = _layer(), _layer(bias=False, co=5)
    a.accumulate_param_grads(_Op("a"), dc, x, pro="p")
    assert calls["specs"] == [[("a", dc, x, a.m.weight.grad, "p")]]
    assert [(s[1] is a.m.bias.grad, s[2]) for s in calls["sums"]] == [(True, 3)]
    HO.submit(zip([a, b], [_Op("a"), _Op("b")], [dc, dc], [x, x], [None, None]))
    assert calls["specs"][1] == [("a", dc, x, a.m.weight.grad, None), ("b", dc, x, b.m.weight.grad, None)]     # one launch
    assert len(calls["sums"]) == 2 and calls["sums"][1][1] is a.m.bias.grad
    assert not HO.tail and HO.queued is None and not any(h.items for h in HO.deferred.values())     # (nothing handed on)


def test_with_the_sink_set_items_go_to_the_sink_and_nowhere_else(calls):
    dc, x = torch.ones(1, 4, 4, 3), torch.ones(1, 6, 6, 2)
    a, b = _layer(), _layer(bias=False, co=5)
    opa, opb = _Op("a"), _Op("b")
    HO.tail_sink = sink = []
    a.accumulate_param_grads(opa, dc, x)
    HO.submit([(a, opa, dc, x, None), (b, opb, dc, x, "p")])
    assert calls["specs"] == [] and calls["sums"] == []
    assert not any(h.items for h in HO.deferred.values()) and not any(h.items for h in HO.inline_bias.values())
    one = (opa, dc, x, a.m.weight.grad, a.m.bias.grad, 3, None)
    assert len(sink) == 2 and sink[0] == one
    assert sink[1] == ("lanes", [one, (opb, dc, x, b.m.weight.grad, None, 0, "p")])
    # the items are what _run_param_grads takes: a batch of them collects its bias sums for one launch
    later = []
    for it in sink:
        handover._run_param_grads(*it, bias_later=later)
    assert [len(s) for s in calls["specs"]] == [1, 2] and calls["sums"] == []
    assert [(s[1] is a.m.bias.grad, s[2]) for s in later] == [(True, 3), (True, 3)]


def test_flush_tail_issues_every_entry_before_a_runner_s_bucket_is_reduced_once(calls, monkeypatch):
    """two tail entries of one runner (a decoder that ran two training forwards): both entries' weight gradients are issued
    before the runner's gradient bucket is reduced, and it is reduced once"""
    import contextlib
    from types import SimpleNamespace
    log = []

    class _Stream:
        device = "dev"

        def wait_event(self, ev):
            log.append(("wait", ev))

    side, chain = _Stream(), _Stream()
    monkeypatch.setattr(handover.RT, "side_stream", lambda device: side)
    monkeypatch.setattr(handover.torch.cuda, "stream", lambda s: contextlib.nullcontext())
    monkeypatch.setattr(handover, "_run_batch", lambda items: log.append(("batch", items)))
    monkeypatch.setattr(handover.RT, "dp", SimpleNamespace(grads_ready=lambda m: log.append(("reduce", m))))
    runner = SimpleNamespace(tail_pending=True, m=SimpleNamespace(_pending=0))
    other = SimpleNamespace(tail_pending=True, m=SimpleNamespace(_pending=1))      # (a backward of its module still to come)
    HO.tail += [handover.TailEntry("e1", chain, ["a"], runner), handover.TailEntry("e2", chain, ["b"], other),
                handover.TailEntry("e3", chain, ["c"], runner)]
    joined, kept = set(HO.pending_join), list(HO.pending_keep)
    try:
        HO.flush_tail()
        assert log == [("wait", "e1"), ("batch", ["a"]), ("wait", "e2"), ("batch", ["b"]), ("wait", "e3"), ("batch", ["c"]),
                       ("reduce", runner.m)]
        assert not runner.tail_pending and not other.tail_pending and not HO.tail
        assert (chain, side) in HO.pending_join and HO.pending_keep[len(kept):] == ["a", "b", "c"]
    finally:
        HO.pending_join, HO.pending_keep = joined, kept
