"""The weight-gradient hand-over: every layer's weight and bias gradient leaves its chain — for a companion stream, the pose
chain's stream or the end of the autograd pass — inside a hipGraph capture in the order that gives each chain and each
chain's weight gradients an executor stream of its own (docs/LAB_r06.md, "the executor's stream assignment").  One object,
HO, owns the state: what a backward pass collects (_reset_pass) and what lasts until the step's join (pending_*)."""
import ctypes as C
from collections import namedtuple
from contextlib import contextmanager

import torch

from ..hip import ops
from ..hip.binding import check, lib
from ..hip.conv import run_specs
from .runtime import RT, grad_of


Held = namedtuple("Held", "chain items")    # what a chain stream has collected and not yet issued (items, or bias sums)
# put off behind `event`, recorded on `chain` (inside a capture: at its `position`): a weight-gradient batch for `stream`,
# a call fn(event) (late_call), a network's weight gradients waiting for the end of the backward pass (defer_to_tail)
Batch = namedtuple("Batch", "event chain stream items position", defaults=(None,))
LateCall = namedtuple("LateCall", "event chain fn position")
TailEntry = namedtuple("TailEntry", "event chain items runner")


def _run_param_grads(*item, bias_later=None):
    """one layer's weight (+ bias) gradient — item = (op, dc, x, gw, gb, nb, pro) — or the same layer of two networks in
    one launch — item = ("lanes", [those tuples]) (fs_conv_wgrad2: one round of blocks, one slab arena, two dW)"""
    lanes = item[1] if item[0] == "lanes" else [item]
    run_specs([op.wgrad_spec(dc, x, gw, pro=pro) for (op, dc, x, gw, gb, nb, pro) in lanes])
    for (op, dc, x, gw, gb, nb, pro) in lanes:
        if gb is not None:
            if bias_later is not None:
                bias_later.append((dc, gb, nb))     # (the caller sums the batch's biases in one launch)
            else:
                ops.channel_sum(dc, gb, nb)


def _run_batch(items):
    """a batch's weight gradients on the current stream, its bias gradients in one launch"""
    sums = []
    for it in items:
        _run_param_grads(*it, bias_later=sums)
    if sums:
        ops.channel_sum_multi(sums)


def _position(chain):
    """token of `chain`'s position in the running capture (fs_capture_position: changes whenever the stream captures a node)"""
    tok = C.c_ulonglong(0)
    check(lib.fs_capture_position(C.c_void_p(chain.cuda_stream), C.byref(tok)), "fs_capture_position")
    return tok.value


class _Handover:
    def __init__(self):
        self.pending_join = set()   # (chain stream, companion stream) pairs with weight-gradient work in flight
        self.pending_keep = []      # tensors the companion kernels still read: kept alive until the join (no record_stream
        #                             bookkeeping in the allocator, and safe inside a hipGraph capture's private pool)
        self.counts = {"late": 0, "shared": 0}   # batches issued late / shared with the other chain's streams (tests read it)
        # per chain, in the order the chains first appeared (flush_deferred() walks them in it); their lists are per pass
        self.deferred = {}          # chain stream id -> Held: weight-gradient work items not yet handed over
        self.inline_bias = {}       # chain stream id -> Held: bias sums of inline weight gradients not yet issued
        self._reset_pass()

    def _reset_pass(self):
        """everything a backward pass collects: emptied when the pass has been issued (_end_of_backward) and, for a pass
        that raised — its end-of-backward callback never ran — by the next pass's first entry point (_drop_stale)"""
        self.queued = None          # id of the backward pass (graph task) whose end-of-backward callback is queued
        for held in (*self.deferred.values(), *self.inline_bias.values()):
            held.items.clear()
        self.late = []              # inside a hipGraph capture, put off: Batch and LateCall, in the order they were
        self.at_end = []            # Batch: parts of a batch issued once every node of the pass has been
        self.tail = []              # TailEntry
        self.tail_sink = None       # while a network's backward collects its weight gradients for the tail: their list
        self.encoder_end = False    # the last two stages and the stem of an encoder's backward are being issued
        self.begun_task, self.begun = None, []   # backward pass, chain streams whose backward has begun in it
        self.batch_no = 0           # (numbering of the FSNET_AMD_MARKS=1 marks around each batch)

    def _drop_stale(self):
        """leftovers of a backward pass that raised: not this pass's gradients (events of a dead capture, a sink nobody
        empties).  The running pass's own entries stay: it queued the callback, or nothing is queued."""
        if self.queued is not None and self.queued != torch._C._current_graph_task_id():
            self._reset_pass()

    def _queue_end_of_backward(self):
        # runs once, when the autograd engine has executed every node of this backward pass and before it synchronises the
        # streams it used with the caller's stream.  (Keyed by the pass: a backward that died in an exception never ran its
        # callback, and must not keep the next one from queueing its own.)
        task = torch._C._current_graph_task_id()
        if self.queued != task:
            torch.autograd.Variable._execution_engine.queue_callback(self._end_of_backward)
            self.queued = task

    def _end_of_backward(self):
        self.queued = None
        self.flush_tail()
        self.flush_inline_bias()
        self.flush_deferred(now=True)
        for b in self.at_end:
            if b.items:
                self._issue_batch(b.chain, b.stream, b.items, ev=b.event)
        self._reset_pass()
        self.join_companions()

    def submit(self, lanes):
        """wgrad + bias grad of one layer — lanes = [(layer, op, dc, x, pro)] — or of the same layer of the lanes of an
        EncoderPass into the parameters' gradient buffers (the lanes whose weights are trained share one launch).  They
        feed nothing downstream in the backward pass, so they run on a companion stream while the chain continues with
        the dgrad.  pro: x is a raw convolution output whose BatchNorm (+ ReLU) the weight gradient applies itself."""
        self._drop_stale()
        live = []
        for cl, op, dc, x, pro in lanes:
            gw = grad_of(cl.m.weight)
            gb = grad_of(cl.m.bias) if cl.m.bias is not None else None
            if gw is None:                       # frozen layer: nothing to accumulate (a lone trainable bias: its sum)
                if gb is not None:
                    ops.channel_sum(dc, gb, cl.m.bias.numel())
                continue
            live.append((op, dc, x, gw, gb, cl.m.bias.numel() if gb is not None else 0, pro))
        if not live:
            return
        item = live[0] if len(live) == 1 else ("lanes", live)
        _, dc, *_ = live[0]
        # (data parallel: inline on the chain stream, so that one event after a stage's last weight gradient covers
        # the arena slice its gradient bucket reduces — also inside a captured step)
        mode = RT.wgrad_streams if (dc.is_cuda and RT.overlap and (RT.dp is None or RT.dp.wgrad_companions)) else 0
        if self.tail_sink is not None:
            # (data parallel, "tail": issued when the backward pass has been issued.  Only DepthDecoderRunner.backward sets
            # the sink, and it has no lanes: a lane set never meets it)
            self.tail_sink.append(item)
        elif not mode:
            _run_param_grads(*item, bias_later=self._inline_bias_list(dc.device))
        else:
            cur = RT.current_stream(dc.device)
            held = self.deferred.setdefault(cur.cuda_stream, Held(cur, []))
            held.items.append(item)
            self._queue_end_of_backward()
            if len(held.items) >= (RT.wgrad_flush_even if RT.even_chains else RT.wgrad_flush):
                self.flush_deferred(cur)

    def at_encoder_end(self, flag):
        """EncoderPass.backward: layer2, layer1 and the stem are being issued (what flush_deferred may share, see there)"""
        self._drop_stale()
        self.encoder_end = flag

    @contextmanager
    def tail_of_pass(self, runner, device):
        """data parallel, weight gradients "tail": what `runner`'s backward submits inside is collected and handed to
        defer_to_tail — also when the backward raises, like every hand-over made before it did"""
        self._drop_stale()
        self.tail_sink = [] if (RT.dp is not None and RT.dp.decoder_tail and RT.overlap and device.type == "cuda"
                                and torch._C._current_graph_task_id() >= 0) else None
        try:
            yield
        finally:
            items, self.tail_sink = self.tail_sink, None
            if items:
                self.defer_to_tail(items, runner, device)

    def defer_to_tail(self, items, runner, device):
        """data parallel, weight gradients "tail" (DataParallelContext.wgrad_mode): the depth decoder's weight gradients —
        its chain goes on with the depth encoder's backward and ends the step, the pose chain's stream finishes earlier —
        are issued on the pose chain's stream once every node of the backward pass has been issued (flush_tail), behind
        that chain's own work; the decoder's gradient bucket follows them there."""
        self._drop_stale()
        chain = RT.current_stream(device)
        ev = torch.cuda.Event()
        ev.record(chain)
        runner.tail_pending = True
        self.tail.append(TailEntry(ev, chain, items, runner))
        self._queue_end_of_backward()

    def flush_tail(self):
        """every entry's weight gradients first, then each runner's gradient bucket once: two entries of one runner (a
        decoder that ran two training forwards) are both in the arena when its bucket is reduced"""
        for t in self.tail:
            side = RT.side_stream(t.chain.device)
            side.wait_event(t.event)
            with torch.cuda.stream(side):
                _run_batch(t.items)
        for t in {id(t.runner): t for t in self.tail}.values():
            t.runner.tail_pending = False
            if RT.dp is not None and t.runner.m._pending == 0:
                with torch.cuda.stream(RT.side_stream(t.chain.device)):
                    RT.dp.grads_ready(t.runner.m)        # the bucket's all-reduce picks up from this stream
        for t in self.tail:                     # (joined, and the operands released, like a companion's batch)
            self.pending_join.add((t.chain, RT.side_stream(t.chain.device)))
            self.pending_keep.extend(t.items)
        self.tail.clear()

    def _inline_bias_list(self, dev):
        """data parallel: the weight gradients run inline on their chain — their bias sums are still collected and issued
        as one launch per gradient bucket (flush_inline_bias from DataParallelContext._reduce_range) instead of one per
        layer (18 launches of ~10 us on the decoders' chains: tools/probes/dp_world1.py)"""
        if not (RT.dp is not None and dev.type == "cuda"):
            return None
        cur = RT.current_stream(dev)
        return self.inline_bias.setdefault(cur.cuda_stream, Held(cur, [])).items

    def drop_inline_bias(self):
        """a new step begins (DataParallelContext.begin_step): whatever a backward that raised left uncollected is not
        this step's gradient"""
        for held in self.inline_bias.values():
            held.items.clear()

    def flush_inline_bias(self, cur=None):
        """issue the collected bias sums of chain stream `cur` (default: every chain) on their chain"""
        for key in ([cur.cuda_stream] if cur is not None else list(self.inline_bias.keys())):
            held = self.inline_bias.get(key)
            if held is None or not held.items:
                continue
            with torch.cuda.stream(held.chain):
                ops.channel_sum_multi(held.items)
            held.items.clear()

    def _issue_batch(self, chain, ws, mine, ev=None):
        """weight-gradient items of `chain` on stream `ws`, behind the chain (ev: behind an event recorded on it earlier)"""
        if ev is None:
            ws.wait_stream(chain)                   # one cross-stream edge per batch
        else:
            ws.wait_event(ev)
        with torch.cuda.stream(ws):
            if RT._marks is not None:
                self.batch_no += 1
                tag = "wg.%s.%d" % ("pose" if RT.is_side(chain) else "depth", self.batch_no)
                RT.mark(tag + ".start")
            _run_batch(mine)
            if RT._marks is not None:
                RT.mark(tag + ".end(%d)" % len(mine))
        self.pending_join.add((chain, ws))

    def issue_late(self, chain=None, advanced=False):
        """issue what was put off on `chain` (default: every chain) inside a capture, in the order it was put off: weight-
        gradient batches (flush_deferred) and gradient-bucket reductions (late_call, from DataParallelContext._reduce_range).
        advanced: only what was put off at an EARLIER position of the chain than its current one — the chain has captured
        its next kernel since, which is all the putting-off is for (flush_deferred); what was put off where the chain still
        stands stays."""
        mine = [e for e in self.late if chain is None or e.chain.cuda_stream == chain.cuda_stream]
        if advanced and mine:
            here = _position(chain)
            mine = [e for e in mine if e.position != here]
        if not mine:
            return
        ids = {id(e) for e in mine}
        self.late[:] = [e for e in self.late if id(e) not in ids]
        for e in mine:
            if isinstance(e, LateCall):
                e.fn(e.event)                       # fn(event recorded on the chain where the call was put off)
            else:
                self._issue_batch(e.chain, e.stream, e.items, ev=e.event)

    def issue_advanced(self, device):
        """a cheap place to let go of what the current chain put off (block and level boundaries of the backward passes):
        under data parallelism a bucket's all-reduce takes its place in the communicator's launch order when it is ISSUED,
        and one issued at the end of the pass would run after every SyncBN exchange of the backward instead of beside it"""
        if self.late:
            self._drop_stale()
            self.issue_late(RT.current_stream(device), advanced=True)

    def late_call(self, chain, fn):
        """inside a capture: call fn(event) when every node of the backward pass has been issued (see flush_deferred) —
        `event` is recorded on `chain` now, and what fn issues on another stream behind it becomes a LATER successor of the
        chain's last node than the chain's next kernel.  Returns False, and does nothing, outside a capture or an autograd
        pass."""
        if not (RT.wgrad_late and torch.cuda.is_current_stream_capturing() and torch._C._current_graph_task_id() >= 0):
            return False
        self._drop_stale()
        self.issue_late(chain, advanced=True)
        ev = torch.cuda.Event()
        ev.record(chain)
        self.late.append(LateCall(ev, chain, fn, _position(chain)))
        self._queue_end_of_backward()
        return True

    def flush_deferred(self, cur=None, now=False):
        """hand the collected weight-gradient work of chain stream `cur` (default: all chains) to its companion.

        Inside a hipGraph capture the batch's kernels are ISSUED later (`now`: at once) — at the chain's next hand-over or
        block boundary that finds it further on (issue_late(advanced=True)), at the latest when the whole backward pass has
        been issued — behind the event recorded here.  Dependencies are the same; what changes is the ORDER of the edges that
        leave the chain's last node: the chain's next kernel becomes its first successor, the batch its second.  The HIP
        graph executor (ROCm 7.2) hands out its 4 streams by a depth-first walk in which a node's first successor stays on
        the node's stream and the k-th further one goes k streams on (mod 4); each stream runs its nodes in the order they
        were captured.  With the batch first, the weight gradients inherited the chain's stream and the chain hopped to one
        where it queued behind whatever the other chain had there (docs/LAB_r06.md, "the executor's stream assignment":
        DEBUG_HIP_GRAPH_DOT_PRINT dumps read with tools/probes/graph_streams.py)."""
        late = (RT.wgrad_late and not now and torch.cuda.is_current_stream_capturing()
                and torch._C._current_graph_task_id() >= 0)
        for key in ([cur.cuda_stream] if cur is not None else list(self.deferred.keys())):
            held = self.deferred.get(key)
            if held is None or not held.items:
                continue
            chain, items = held
            self.issue_late(chain, advanced=late)   # (what was put off goes first: the companion runs batches in this order)
            ws = RT.companion_stream(chain.device, chain)[1]
            ev = None
            capturing = late or torch.cuda.is_current_stream_capturing()
            if capturing:
                ev = torch.cuda.Event()
                ev.record(chain)
            mine = list(items)
            if (RT.wgrad_balance and RT.even_chains and capturing and self.encoder_end and RT.dp is None
                    and not RT.is_side(chain) and len(items) >= 2 and torch._C._current_graph_task_id() >= 0):
                # the end of the main chain's encoder: the chain's companion still has the depth decoder's weight gradients
                # to run when the encoder's arrive, and ends the step with them after the pose chain and its companion have
                # finished.  Half of each batch from layer2 on goes to the pose chain's stream, issued at the end of the pass
                # like everything else — behind the pose chain's own work; as the third successor of the hand-over point the
                # share lands on the executor's stream of the pose chain.  (Shares of the encoder's earlier batches run
                # beside the depth chain rather than after it: measured, they slow it more than they relieve the companion.)
                side = RT.side_stream(chain.device)
                others = [side, RT.companion_stream(chain.device, side)[1]][:RT.wgrad_balance]
                n = 1 + len(others)
                self.at_end.extend(Batch(ev, chain, o, items[1 + k::n]) for k, o in enumerate(others))
                self.counts["shared"] += 1
                mine = items[0::n]
            if late:
                self.late.append(Batch(ev, chain, ws, mine, _position(chain)))
                self.counts["late"] += 1
            else:
                self._issue_batch(chain, ws, mine, ev=ev)
            self.pending_keep.extend(items)
            items.clear()
        if not late:
            self.issue_late(cur)

    def chain_ends(self, device):
        """a chain has issued its last kernel (the end of an encoder's backward).  Inside a capture, with hand-overs put off:
        one empty launch on the chain, so that the last hand-over point has a first successor that stays on the chain's
        stream like every other one — otherwise the last batch inherits the chain's executor stream and the share that
        follows it the companion's, behind the companion's backlog."""
        if (RT.wgrad_late and (self.late or self.at_end) and device.type == "cuda" and torch.cuda.is_current_stream_capturing()
                and torch._C._current_graph_task_id() >= 0):
            RT.nop(device)
            self.issue_late(RT.current_stream(device))

    def chain_begins(self, device):
        """called where a network's backward begins on its chain (the decoders' autograd nodes).  Inside a hipGraph capture,
        when the SECOND chain of the pass begins, one empty launch is put on the first chain's companion, behind the second
        chain's pending dependencies — a third successor of the loss backward's last node, between the two chains' first
        kernels.  By the executor's rule (flush_deferred) the first chain then keeps that node's stream s, its weight
        gradients get s+1, the second chain s+2 and its weight gradients s+3: four streams, one each.  Without it the second
        chain shares s+1 with the first chain's weight gradients, behind them in launch order."""
        if not (RT.wgrad_late and device.type == "cuda" and RT.overlap and RT.wgrad_streams
                and torch.cuda.is_current_stream_capturing()):
            return
        task = torch._C._current_graph_task_id()
        if task < 0:
            return
        self._drop_stale()
        if self.begun_task != task:
            self.begun_task, self.begun = task, []
        cur = RT.current_stream(device)
        if any(c.cuda_stream == cur.cuda_stream for c in self.begun):
            return
        self.begun.append(cur)
        if len(self.begun) == 2:
            first = self.begun[0]
            ws = RT.companion_stream(device, first)[1]
            ws.wait_stream(cur)
            with torch.cuda.stream(ws):
                RT.nop(device)
            self.pending_join.add((first, ws))

    def pending_companions(self):
        """companion streams with weight-gradient work in flight in this step"""
        return {ws for _, ws in self.pending_join}

    def join_companions(self):
        """every chain stream waits for its companion.  Inside a hipGraph capture the join is left to
        join_companions_final(): joining a companion into a stream that is itself a fork of the capture stream and
        then joining that one crashes hipStreamEndCapture on ROCm 7.2 (tools/probes/graph_fork_probe.py, variants
        C/D), joining every companion straight into the capture stream does not (variant G)."""
        if not self.pending_join or torch.cuda.is_current_stream_capturing():
            return
        for cur, ws in list(self.pending_join):
            cur.wait_stream(ws)
        self.pending_join.clear()
        self.pending_keep.clear()

    def join_companions_final(self):
        """the current stream waits for every companion with work in flight (before the optimizer reads gradients)"""
        self.flush_inline_bias()
        self.flush_deferred(now=True)
        self.issue_late()
        if self.pending_join:
            cur = torch.cuda.current_stream()
            for ws in self.pending_companions():
                cur.wait_stream(ws)
            self.pending_join.clear()
            self.pending_keep.clear()


HO = _Handover()
