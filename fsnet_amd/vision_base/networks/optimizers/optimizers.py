"""build_optimizer with the reference's signature (vision_base/networks/optimizers/optimizers.py:4-11).
'adam' / 'adamw' / 'sgd' return FusedAdam / FusedAdamW / FusedSGD: torch.optim's arithmetic (bias correction, eps
outside the sqrt, L2 or decoupled weight decay; momentum, dampening, nesterov) executed by the HIP clip+update kernel —
one hipGraph-replayable launch over the meta-arch's flat parameter arena, restricted to the runs of it that hold
trainable parameters (a frozen parameter is not touched, whatever the weight decay: torch.optim skips it because its
gradient is None, here its arena slot lies outside the run table)."""
import torch
import torch.nn as nn
import torch.optim as optim

from fsnet_amd.engine.handover import HO
from fsnet_amd.engine.runtime import RT
from fsnet_amd.hip import ops


def trainable_runs(arena):
    """[(lo, hi)] element ranges of the arena that hold trainable parameters: adjacent trainable slots merged, a slot
    taken with its padding to 4 elements (so every boundary is 16-byte aligned; the padding holds zeros with zero
    gradients, which no update moves).  Nothing frozen: the one run (0, arena.total)."""
    runs = []
    for p, o in zip(arena.params, arena.offsets):
        if not p.requires_grad:
            continue
        end = o + (p.numel() + 3) // 4 * 4
        if runs and runs[-1][1] == o:
            runs[-1][1] = end
        else:
            runs.append([o, end])
    return [tuple(r) for r in runs]


class ArenaOptimizer:
    """What the three fused optimizers share (mixed in ahead of a torch.optim class): the update's state as flat arrays
    beside the arena with per-parameter views in `self.state` (state_dict() keeps torch.optim's layout), the
    device-resident step count and learning rate the captured launch reads, the fused gradient norm, the run table.

    A subclass gives STATE (its state arrays' names in torch's state dict), _launch (the kernel call) and _plain_step
    (the step without an arena: a CPU module, a foreign module, more than one param group, an option the kernel does not
    implement)."""
    STATE = ()
    UNSUPPORTED = ("amsgrad", "maximize", "capturable", "differentiable", "foreach", "fused")

    def _init_arena(self, model):
        self._model = model
        self._arena_state = None
        self._readopt = False
        self._sumsq = None
        self._clean_sq = False
        self._step_count_fused = 0
        self._step_buf = None      # device-resident step count / lr: the step kernel is hipGraph-replayable
        self._lr_buf = None
        self._lr_host = None
        self._runs = None          # (arena, requires_grad mask, device run table or None)

    # -- flat path -------------------------------------------------------------------------------
    def _arena(self):
        m = self._model
        m = getattr(m, "module", m)
        arena = getattr(m, "_arena", None)
        if arena is None or len(self.param_groups) != 1:
            return None
        g0 = self.param_groups[0]
        if any(g0.get(k) for k in self.UNSUPPORTED):
            return None
        ps = g0["params"]
        if len(ps) != len(arena.params) or any(a is not b for a, b in zip(ps, arena.params)):
            return None
        return arena

    def _state_names(self):
        return self.STATE

    def _step_of(self, st):
        """step count recorded in one parameter's loaded state"""
        return int(st["step"])

    def _publish(self, arena, flat):
        """per-parameter views of the flat state in self.state, so that state_dict() keeps torch.optim's format"""
        names = self._state_names()
        for p, o in zip(arena.params, arena.offsets):
            st = {"step": torch.tensor(float(self._step_count_fused))}
            for name, f in zip(names, flat):
                st[name] = f[o:o + p.numel()].view(p.shape)
            self.state[p] = st

    def _flat_state(self, arena):
        names = self._state_names()
        cur = self._arena_state
        if cur is None or cur[0] is not arena or cur[1] != names or self._readopt:
            if cur is not None and cur[0] is arena and cur[1] == names:
                flat = [f.zero_() for f in cur[2]]          # same storage: graphs stay valid
            else:
                flat = [torch.zeros_like(arena.data) for _ in names]
            self._readopt = False
            step0 = 0
            for p, o in zip(arena.params, arena.offsets):   # adopt state loaded from a checkpoint
                st = self.state.get(p, None)
                if st and names and torch.is_tensor(st.get(names[0])):
                    for name, f in zip(names, flat):
                        f[o:o + p.numel()].copy_(st[name].reshape(-1))
                    step0 = self._step_of(st)
            self._arena_state = (arena, names, flat)
            self._step_count_fused = step0
            self._publish(arena, flat)
            if self._step_buf is not None:       # keep the pointer (a captured graph holds it), reset the value
                self._step_buf.fill_(step0)
        return self._arena_state[2]

    def run_mask(self, arena):
        """which arena parameters are trainable, or None when all are: part of the captured step's signature (the run
        table is baked into the launch, so freezing or unfreezing a parameter re-captures)"""
        mask = tuple(p.requires_grad for p in arena.params)
        return None if all(mask) else mask

    def _run_table(self, arena):
        mask = self.run_mask(arena)
        if self._runs is None or self._runs[0] is not arena or self._runs[1] != mask:
            table = None
            if mask is not None:
                runs = trainable_runs(arena) or [(0, 0)]
                table = torch.tensor(runs, dtype=torch.int64).to(arena.data.device)
            self._runs = (arena, mask, table)
        return self._runs[2]

    def _prezero(self):
        """(ops.prezero_all) the gradient-norm accumulator is about to be zeroed with the step's scratch"""
        if self._sumsq is None:
            return []
        self._clean_sq = True
        return [self._sumsq_buf]

    @torch.no_grad()
    def step(self, closure=None, max_norm=None, grad_scale=1.0):
        """max_norm: fused clip_grad_norm_ (joint L2 norm over all parameters) when given."""
        arena = self._arena()
        if arena is None:
            return self._plain_step(closure, max_norm, grad_scale)
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        g0 = self.param_groups[0]
        HO.join_companions_final()        # weight-gradient kernels still in flight on companion streams
        flat = self._flat_state(arena)
        runs = self._run_table(arena)
        dev = arena.data.device
        if self._step_buf is None or self._step_buf.device != dev:
            self._step_buf = torch.full((1,), self._step_count_fused, dtype=torch.int32, device=dev)
            self._lr_buf = torch.full((1,), float(g0["lr"]), dtype=torch.float32, device=dev)
            self._lr_host = float(g0["lr"])
        self.sync_lr()
        sq = None
        if max_norm is not None and max_norm > 0:
            if self._sumsq is None or self._sumsq.device != dev:
                # (16 bytes: the step's one-launch scratch zeroing takes 16-byte aligned spans)
                self._sumsq_buf = torch.zeros(2, dtype=torch.float64, device=dev)
                self._sumsq = self._sumsq_buf[:1]
                self._clean_sq = False
                ops.register_prezero(self, lambda o: o._prezero(), dev)
            if self._clean_sq:
                from fsnet_amd.engine.nets import join_pack
                join_pack(dev)
            else:
                self._sumsq.zero_()
            self._clean_sq = False
            # (over the whole arena: frozen parameters carry zero gradients)
            ops.sumsq(arena.grad, self._sumsq, step_counter=self._step_buf)   # also bumps the device step count
            sq = self._sumsq
        else:
            ops.counter_incr(self._step_buf)
        self._launch(arena, flat, g0, dict(max_norm=max_norm or 0.0, sumsq_buf=sq, grad_scale=grad_scale,
                                           step_buf=self._step_buf, lr_buf=self._lr_buf, runs=runs))
        self.note_step()
        RT.bump_weights()   # parameters changed through raw pointers: conv operands must be re-packed
        return loss

    def _torch_step(self, closure, max_norm, grad_scale):
        """the torch.optim base class's own step, after what the training hook does in front of a plain optimizer"""
        HO.join_companions_final()
        params = [p for g in self.param_groups for p in g["params"] if p.grad is not None]
        if grad_scale != 1.0:
            for p in params:
                p.grad.mul_(grad_scale)
        if max_norm is not None and max_norm > 0 and params:
            torch.nn.utils.clip_grad_norm_(params, max_norm)
        loss = super().step(closure)
        RT.bump_weights()
        return loss

    def note_step(self):
        """host-side bookkeeping of one (eager or graph-replayed) fused step"""
        self._step_count_fused += 1

    def _refresh_steps(self):
        if self._arena_state is not None:
            for p in self._arena_state[0].params:
                self.state[p]["step"].fill_(float(self._step_count_fused))

    def state_dict(self):
        self._refresh_steps()      # per-parameter "step" entries are only materialised when someone looks
        return super().state_dict()

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._readopt = True       # re-adopt the state arrays / step count from the loaded per-parameter state

    def prepare_replay(self):
        """before a captured step is replayed: adopt freshly loaded state in place, push the current lr"""
        arena = self._arena()
        if self._readopt and arena is not None:
            self._flat_state(arena)
        self.sync_lr()

    def sync_lr(self):
        """push a scheduler-changed learning rate to the device scalar the (possibly captured) kernel reads"""
        lr = float(self.param_groups[0]["lr"])
        if self._lr_buf is not None and lr != self._lr_host:
            self._lr_buf.fill_(lr)
            self._lr_host = lr

    def grad_norm(self):
        """sqrt of the last fused sum of squares (device tensor; no host sync)."""
        return None if self._sumsq is None else self._sumsq.sqrt()


class FusedAdam(ArenaOptimizer, optim.Optimizer):
    STATE = ("exp_avg", "exp_avg_sq")
    UNSUPPORTED = ("amsgrad", "maximize", "capturable", "differentiable")    # (its own param groups hold none of them:
    DECOUPLED = False                                                        # those of an adopted torch.optim.Adam may)

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, model=None):
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        super().__init__(params, defaults)
        self._init_arena(model)

    def _launch(self, arena, flat, g0, kw):
        ops.adamw_step(arena.data, arena.grad, flat[0], flat[1], g0["lr"], g0["betas"][0], g0["betas"][1], g0["eps"],
                       g0["weight_decay"], 1, decoupled=self.DECOUPLED, **kw)

    def _plain_step(self, closure, max_norm, grad_scale):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        HO.join_companions_final()
        params = [p for g in self.param_groups for p in g["params"] if p.grad is not None]
        sq = None
        if max_norm is not None and max_norm > 0 and params:
            sq = torch.zeros(1, dtype=torch.float64, device=params[0].device)
            for p in params:
                ops.sumsq(p.grad, sq)
        for g in self.param_groups:
            for p in g["params"]:
                if p.grad is None:
                    continue
                st = self.state[p]
                if not st:
                    st["step"] = torch.tensor(0.0)
                    st["exp_avg"] = torch.zeros_like(p)
                    st["exp_avg_sq"] = torch.zeros_like(p)
                st["step"] += 1
                ops.adam_step(p.data, p.grad, st["exp_avg"], st["exp_avg_sq"], g["lr"], g["betas"][0],
                              g["betas"][1], g["eps"], g["weight_decay"], int(st["step"]),
                              max_norm=max_norm or 0.0, sumsq_buf=sq, grad_scale=grad_scale)
        RT.bump_weights()
        return loss


class FusedAdamW(ArenaOptimizer, optim.AdamW):
    """torch.optim.AdamW whose step over a meta-arch's arena is the fused launch (decoupled weight decay)"""
    STATE = ("exp_avg", "exp_avg_sq")
    DECOUPLED = True
    _launch = FusedAdam._launch
    _plain_step = ArenaOptimizer._torch_step

    def __init__(self, params, *args, model=None, **kwargs):
        super().__init__(params, *args, **kwargs)
        self._init_arena(model)


class FusedSGD(ArenaOptimizer, optim.SGD):
    """torch.optim.SGD whose step over a meta-arch's arena is the fused launch.  torch's first step stores the gradient
    as the momentum buffer without dampening; the kernel takes that branch when the device-resident step count is 1, so
    a captured launch replays as steps 2, 3, ... and not as the first one again."""
    _plain_step = ArenaOptimizer._torch_step

    def __init__(self, params, *args, model=None, **kwargs):
        super().__init__(params, *args, **kwargs)
        self._init_arena(model)

    def _state_names(self):
        return ("momentum_buffer",) if self.param_groups[0]["momentum"] != 0 else ()

    def _step_of(self, st):
        return 1       # torch.optim.SGD keeps no count: a momentum buffer exists, so the first step is behind us

    def _publish(self, arena, flat):
        """torch's layout: no state before the first step, then {"momentum_buffer": tensor, or None without momentum}"""
        for p, o in zip(arena.params, arena.offsets):
            if self._step_count_fused == 0:
                self.state.pop(p, None)
            else:
                self.state[p] = {"momentum_buffer": flat[0][o:o + p.numel()].view(p.shape) if flat else None}

    def _refresh_steps(self):
        if self._arena_state is not None:
            self._publish(self._arena_state[0], self._arena_state[2])

    def _launch(self, arena, flat, g0, kw):
        ops.sgd_step(arena.data, arena.grad, flat[0] if flat else None, g0["lr"], g0["momentum"], g0["dampening"],
                     g0["nesterov"], g0["weight_decay"], 1, **kw)


def build_optimizer(model: nn.Module, name, **kwargs):
    if name.lower() == 'adam':
        return FusedAdam(model.parameters(), model=model, **kwargs)
    if name.lower() == 'sgd':
        return FusedSGD(model.parameters(), model=model, **kwargs)
    if name.lower() == 'adamw':
        return FusedAdamW(model.parameters(), model=model, **kwargs)
    raise NotImplementedError(name)
