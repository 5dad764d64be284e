"""The captured data-parallel step with collectives that DO something, on the one GPU of the test box.

RCCL runs a single-rank all-reduce as nothing, so the world-size-1 tests (tests/test_dp_gpu.py) cannot see a gradient bucket
reduced before its weight gradients have landed; torch.distributed over gloo (tests/test_dp2_gpu.py) cannot be captured.  Here
two processes share the GPU, a stand-in for rccl_direct.DirectComm multiplies by the world size — the SUM over ranks that hold
the same values, as both ranks step on the same batch — and every step is captured and replayed.  A bucket reduced too early
scales an incomplete gradient and leaves what lands later unscaled; a SyncBN exchange at the wrong place scales the wrong sums.
Inside a capture every hand-over — weight-gradient batches, bucket reductions — is issued at the end of the backward pass behind
events (HO.flush_deferred / late_call, DataParallelContext._reduce_range): this is the test of those dependencies, for each
placement of the weight gradients and both encoder arrangements, against one process stepping without data parallelism."""
import os
import socket

import pytest
import torch

from oracle import fsnet_oracle as O

pytestmark = pytest.mark.gpu
B, H, W, STEPS = 2, 64, 128, 5


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


class _StandInComm:
    def __init__(self, device, world):
        self.device, self.world = device, world
        self.capture_ok, self.capture_test, self.agreement = True, "stand-in", None
        self.calls = 0

    def all_reduce_sum(self, t, out=None):
        self.calls += 1
        if out is None:
            t.mul_(float(self.world))
        else:
            torch.mul(t, float(self.world), out=out)

    def broadcast(self, t, root=0):
        pass

    def close(self):
        pass


def _build(dev, lanes):
    from fsnet_amd.configs import meta_arch_cfg, training_cfg
    from fsnet_amd.engine.runtime import RT
    from fsnet_amd.vision_base.networks.optimizers.optimizers import build_optimizer
    from fsnet_amd.vision_base.utils.builder import build
    RT.set_compute_dtype(torch.float32)
    RT.tie_noise = False
    RT.lanes = lanes
    m = build(**meta_arch_cfg(H, W, with_pose=True))
    m.load_state_dict(O.init_state(seed=17, with_pose=True), strict=True)
    m = m.to(dev).train()
    tc = training_cfg()
    return m, build_optimizer(m, **tc.optimizer), build(use_graph=True, graph_warmup=2, **tc.training_hook)


def _steps(hook, m, opt):
    losses, grads = [], None
    for it in range(STEPS):
        out = hook(dict(O.synthetic_batch(B, H, W, seed=800 + it)), m, opt)
        losses.append(float(out["loss"].detach()))
        if it == 2:
            # the captured step's first replay, on weights that two eager steps made (the same in every run up to summation
            # order; later steps' gradients differ by what Adam makes of that: 0.24 seen on the pose encoder's stem at step 5).
            # The gradients stay in the arena until the next step zeroes them: SUMs over the ranks under data parallelism.
            torch.cuda.synchronize()
            grads = {k: p.grad.detach().double().cpu() for k, p in m.named_parameters() if p.grad is not None}
    torch.cuda.synchronize()
    return losses, torch.cat([p.detach().flatten() for p in m.parameters()]).cpu(), grads


def _rank_main(rank, world, port, out_path, lanes, wgrad):
    import torch.distributed as dist
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    os.environ["FSNET_AMD_DP_WGRAD"] = wgrad
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    try:
        from fsnet_amd.engine.handover import HO
        from fsnet_amd.engine.dataparallel import DataParallelContext
        from fsnet_amd.engine.runtime import RT
        m, opt, hook = _build(dev, lanes)
        p0 = torch.cat([p.detach().flatten() for p in m.parameters()]).cpu()
        m.ensure_arena()
        RT.dp = DataParallelContext(m)
        fake = _StandInComm(dev, world)
        RT.dp._direct, RT.dp._comm_stream, RT.dp.capturable = fake, RT.new_stream(dev), True
        before = dict(HO.counts)
        losses, params, grads = _steps(hook, m, opt)
        assert hook.graph_captures == 1 and hook.graph_replays == STEPS - 3, (hook.graph_captures, hook.graph_replays)
        assert RT.dp.wgrad_mode == wgrad and bool(RT.lanes) == lanes
        if wgrad == "companion":
            assert HO.counts["late"] > before["late"]          # (batches put off inside the capture)
        assert not HO.late and not HO.at_end
        calls = fake.calls
        RT.dp._direct = None                                        # (nothing to close: the stand-in owns no communicator)
        RT.dp.close()
        RT.dp = None
        torch.save({"losses": losses, "update": params - p0, "calls": calls, "grads": grads}, out_path % rank)
    finally:
        dist.destroy_process_group()


def _reference(dev, lanes, out_path):
    """one process, no data parallelism, the same batches: what two ranks with identical shards must reproduce"""
    from fsnet_amd.engine.runtime import RT
    m, opt, hook = _build(dev, lanes)
    p0 = torch.cat([p.detach().flatten() for p in m.parameters()]).cpu()
    losses, params, grads = _steps(hook, m, opt)
    assert RT.dp is None
    torch.save({"losses": losses, "update": params - p0, "grads": grads}, out_path)


def _ref_main(out_path, lanes):
    torch.cuda.set_device(0)
    _reference(torch.device("cuda", 0), lanes, out_path)


@pytest.mark.parametrize("lanes,wgrad", [(False, "inline"), (False, "companion"), (False, "tail"), (True, "inline"),
                                         (True, "companion"), (True, "tail")])
def test_captured_two_rank_step_with_collectives_that_count(dev, tmp_path, lanes, wgrad):
    import torch.multiprocessing as mp
    from tests.test_dp_gpu import same_update
    ctx = mp.get_context("spawn")
    ref_path = str(tmp_path / "ref.pt")
    p = ctx.Process(target=_ref_main, args=(ref_path, lanes))
    p.start()
    p.join(timeout=600)
    assert p.exitcode == 0
    port = _free_port()
    out_path = str(tmp_path / "rank%d.pt")
    procs = [ctx.Process(target=_rank_main, args=(r, 2, port, out_path, lanes, wgrad)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=600)
        assert p.exitcode == 0, "rank process failed or hung (exit code %r)" % p.exitcode
    ref = torch.load(ref_path)
    for k in range(2):
        r = torch.load(out_path % k)
        assert r["calls"] > 50                                       # eager warm-up steps + the capture: SyncBN + buckets
        assert r["losses"][:2] == pytest.approx(ref["losses"][:2], rel=2e-4)
        assert r["losses"] == pytest.approx(ref["losses"], rel=5e-3)
        agree, rel = same_update(r["update"], ref["update"])
        assert agree > 0.97 and rel < 0.2, (k, lanes, wgrad, agree, rel)
        # Adam does not see a gradient's scale: the buckets themselves — every parameter's gradient is the SUM over the two
        # ranks (a bucket reduced before its weight gradients landed would hold 1x, or a mixture)
        gmax = max(float(g.norm()) for g in ref["grads"].values())
        for name, g in ref["grads"].items():
            if float(g.norm()) < 1e-6 * gmax:
                continue
            err = float((r["grads"][name] - 2.0 * g).norm() / (2.0 * g.norm()))
            assert err < 0.2, (k, lanes, wgrad, name, err)     # (run-to-run noise of single layers: up to 4e-2 — test_graph_gpu.py)
