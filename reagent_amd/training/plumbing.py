"""Host-side step plumbing shared by every trainer: the autograd bridge of the generator path (SegmentLoss), the
held-gradient / data-parallel / publish sequence of a HIP backward (TrainableNet.backward), the native-step marker and
its 1/world convention (dp_reduce, native_step), the mixin of the trainers with a native step (NativeStepMixin), the
critic on (state, panel) rows of the parametric and SlateQ trainers (PanelCriticMixin), and the graph-mode switches the
runtime loops call.  No kernel is launched from here except through the stacks and ops the callers hand in."""
import functools

import torch

from .. import ops
from ..engine import FusedMLP, ensure_slab, grad_views


class SegmentLoss(torch.autograd.Function):
    """Scalar loss whose backward runs a HIP backward closure (writes ``.grad`` in place)."""

    @staticmethod
    def forward(ctx, closure, loss_buf, *params):
        ctx.closure = closure
        ctx.n = len(params)
        return loss_buf.detach().clone().reshape(())

    @staticmethod
    def backward(ctx, grad_out):
        ctx.closure(grad_out)
        return (None, None) + (None,) * ctx.n


def dp_reduce(tr, slab):
    """Sum the gradient slab over the data-parallel group (RCCL).  Inside a native step the 1/world factor
    is folded into the Adam launch (grad_scale); on the generator / Lightning path the optimizers are
    stepped by the caller, so the sum is turned into the mean here and Adam, weight decay and any gradient
    clipping see what a single rank would on the concatenated batch."""
    torch.distributed.all_reduce(slab.grad, group=tr._dp_group)
    if not getattr(tr, "_native_active", False):
        slab.grad.mul_(1.0 / tr._dp_world)


class NativeStep:
    """marks the trainer as inside a native step (see dp_reduce)"""

    def __init__(self, tr):
        self.tr = tr

    def __enter__(self):
        self.prev = getattr(self.tr, "_native_active", False)
        self.tr._native_active = True

    def __exit__(self, *exc):
        self.tr._native_active = self.prev


def native_step(fn):
    """decorator for train_step_native of the trainers: the whole call runs as a native step"""

    @functools.wraps(fn)
    def wrapper(self, *a, **k):
        # (ops.deferred_ticks: the schedule ticks of the step's device-scheduled updates leave as ONE launch at its end)
        with NativeStep(self), ops.deferred_ticks():
            return fn(self, *a, **k)

    return wrapper


def held_gradients(slab, params):
    """A backward without a preceding zero_grad() accumulates in PyTorch, but the HIP backward OVERWRITES
    the gradient slab.  Returns copies of the gradients still published through p.grad (aliases of the
    slab) so that `publish_gradients` can add them back; empty when the gradients were cleared
    (`zero_grad(set_to_none=True)`, every native step)."""
    base = slab.grad.data_ptr()
    return [(i, slab.view(slab.grad, i).clone()) for i, p in enumerate(params)
            if p.grad is not None and p.grad.data_ptr() == base + 4 * slab.offsets[i]]


def publish_gradients(slab, params, held=()):
    """p.grad aliases the slab the backward wrote (gradients held over a missing zero_grad() are added
    back; foreign .grad tensors are accumulated into)"""
    for i, g in held:
        slab.view(slab.grad, i).add_(g)
    base = slab.grad.data_ptr()
    for i, p in enumerate(params):
        gv = slab.view(slab.grad, i)
        if p.grad is None or p.grad.data_ptr() == base + 4 * slab.offsets[i]:
            p.grad = gv
        else:
            p.grad.add_(gv)


class TrainableNet:
    """One trainable network of a step: its parameters, their flat slab, the FC stack and the slab's weight / bias
    gradient views in layer order.  Built from a module with `.fc`, once per engine (re)build; `reduce(net)` is the
    owning trainer's data-parallel sum of the slab's gradients (NativeStepMixin._dp_sum unless the trainer has its own)."""

    def __init__(self, net, reduce):
        self.fc = net.fc
        self.params = list(net.parameters())
        self.slab = ensure_slab(self.params)
        self.stack = net.fc.stack()
        self.reduce = reduce
        self.rebind_grads()

    def rebind_grads(self):
        """weight/bias gradient destinations = views of the flat gradient slab (again after slab.grad was re-pointed)"""
        self.dw, self.db = grad_views(self.fc, self.slab, self.params)

    def clear_grads(self):
        for p in self.params:
            p.grad = None

    def backward(self, d, xt, grad_out=None, reduce=True, held=None, **stack_kwargs):
        """The stack's backward from the output gradient `d` (times the autograd bridge's grad_out) and the transposed
        staged input `xt` into the slab, the data-parallel sum, and p.grad published with PyTorch's accumulation rule.
        reduce=False: the caller sums this slab itself, together with others.  held: gradients the caller took with
        `held_gradients` before it wrote slab views of its own (layers outside the stack)."""
        if grad_out is not None:
            d = d * grad_out
        if held is None:
            held = held_gradients(self.slab, self.params)
        self.stack.backward(d, xt, self.dw, self.db, **stack_kwargs)
        if reduce:
            self.reduce(self)
        publish_gradients(self.slab, self.params, held)

    def loss(self, backward, loss_buf):
        """the segment's loss for the generator path: `backward(grad_out)` runs when autograd reaches it"""
        return SegmentLoss.apply(backward, loss_buf, *self.params)


class NativeStepMixin:
    """What every trainer with a `train_step_native` shares: the data-parallel group, the optimizers of the native step,
    the input conversions and one segment of the step (clear, backward, scaled optimizer step)."""

    _dp_group = None
    _dp_world = 1
    # the native step folds 1/world into its Adam launches, which torch's own optimizers cannot (QStepCore's
    # _step_optimizer scales their gradients itself and says False)
    _dp_needs_grad_scaling_optimizers = True

    def native_optimizers(self):
        if getattr(self, "_native_opts", None) is None:
            made = self.configure_optimizers()
            self._native_opts = [o["optimizer"] for o in made]
            # lr schedulers of the optimizer configs (None where there is none): with Lightning its loop
            # steps them per epoch; a caller of the native loop does `for s in native_schedulers(): s.step()`
            self._native_scheds = [o.get("lr_scheduler") for o in made]
        return self._native_opts

    def native_schedulers(self):
        self.native_optimizers()
        return [s for s in self._native_scheds if s is not None]

    # ---- data parallel -------------------------------------------------------
    def enable_data_parallel(self, process_group=None):
        """All-reduce(sum) the flat fp32 gradient slab over RCCL after every backward; the 1/world
        factor is folded into the Adam kernel (FusedAdam.grad_scale)."""
        import torch.distributed as dist

        self._dp_group = process_group if process_group is not None else dist.group.WORLD
        self._dp_world = dist.get_world_size(self._dp_group)
        if self._dp_needs_grad_scaling_optimizers:
            require_grad_scaling_optimizers(self)
        return self

    def _dp_sum(self, net):
        if self._dp_group is not None:
            dp_reduce(self, net.slab)

    def _trainable(self, net):
        return TrainableNet(net, self._dp_sum)

    @staticmethod
    def _f32c(t: torch.Tensor) -> torch.Tensor:
        t = t if t.dtype == torch.float32 else t.float()
        return t if t.is_contiguous() else t.contiguous()

    @staticmethod
    def _net_in(t: torch.Tensor) -> torch.Tensor:
        """network input: fp32, or bf16 (the normalize-on-gather output of the bf16 path: the fused kernels would round
        the fp32 rows to the same bf16 values on load)"""
        if t.dtype not in (torch.float32, torch.bfloat16):
            t = t.float()
        return t if t.stride(-1) == 1 and t.is_contiguous() else t.contiguous()

    def _gamma_exponent(self, b):
        """exponent of gamma in the discount tensor (dqn_trainer.py:240-254), None = 1"""
        gamma_exp = None
        if self.use_seq_num_diff_as_time_diff:
            assert self.multi_steps is None
            gamma_exp = self._f32c(b.time_diff).reshape(-1)
        if self.multi_steps is not None:
            assert b.step is not None
            gamma_exp = self._f32c(b.step).reshape(-1)
        return gamma_exp

    def _native_segment(self, net, backward, opt, fused=None):
        """one segment of a native step: clear the network's .grad, run its backward, step its optimizer with the
        data-parallel 1/world folded into the launch.  backward=None: the gradients are already in the slab (summed
        in a bucket with another network's); fused: the network's engine.FusedUpdate, stepped in the optimizer's place"""
        if backward is not None:
            net.clear_grads()
            backward()
        if fused is not None:
            fused.step(1.0 / self._dp_world)
        else:
            opt.grad_scale = 1.0 / self._dp_world
            opt.step()


class PanelCriticMixin:
    """A critic evaluated on rows cat(state[r // M], panel[r]) (parametric DQN's candidate actions, SlateQ's documents)."""

    @staticmethod
    def _reads_panels(stack, state_dim: int) -> bool:
        """the fused kernels read cat(state, action) in place as two K-panels (the state panel tiled or not); every other
        engine, and a state width that is not a multiple of 32, takes the rows rg_tile_concat assembles"""
        return isinstance(stack, FusedMLP) and state_dim % 32 == 0

    def _cat_ws(self, rows, S, A, dev):
        """rows -> assembled [rows, S + A] critic input (engines that do not read panels); the trainer's `_engine` empties
        `self._cat` when the step's shapes change"""
        w = self._cat.get(rows)
        if w is None:
            w = self._cat[rows] = torch.empty(rows, S + A, dtype=torch.float32, device=dev)
        return w

    @staticmethod
    def _state_in(t, stack):
        """state rows as a network input: fp32, or network-ready bf16 rows for a fused stack"""
        if t.dtype == torch.bfloat16 and isinstance(stack, FusedMLP):
            return t if t.is_contiguous() else t.contiguous()
        return NativeStepMixin._f32c(t)

    def _critic_rows(self, stack, state, cand, out, M=1, save=False):
        """out = critic(cat(state[r // M], cand[r])) for every row r of cand; -> the transposed staged input a saving
        forward of the per-layer engine hands its backward (None on the fused kernels).  A SAVING forward on tiled rows
        always takes assembled rows: the fused kernels' tiled two-panel forward saves nothing for a backward"""
        S, A = state.shape[1], cand.shape[1]
        if self._reads_panels(stack, S) and not (save and M > 1):
            stack.forward(self._state_in(state, stack), out, save=save, x2=cand, x_tile=M)
            return None
        x = self._cat_ws(cand.shape[0], S, A, cand.device)
        ops.tile_concat(NativeStepMixin._f32c(state), cand, x, x_tile=M)
        xc, xt = stack.stage_input(x, need_transposed=save)
        stack.forward(xc, out, save=save)
        return xt


def enable_graph_mode(tr):
    """Switch every Adam of the trainer's native step to device-scheduled stepping (optimizer.AdamSchedule): what
    a HIP-graph capture of the step needs.  Eager steps keep working (and produce the same bits)."""
    if getattr(tr, "_graph_capture_refusal", None):  # a trainer whose step's launch shapes change from step to step
        raise NotImplementedError(f"{type(tr).__name__}: {tr._graph_capture_refusal}")
    if any(isinstance(m, torch.nn.Dropout) and m.p > 0.0 for m in tr.modules()):
        # rg_dropout's Philox offset is a host-side launch argument: a replayed graph would repeat one mask forever
        raise NotImplementedError("networks with dropout layers are not captured into a HIP graph: run the native step eagerly")
    for o in tr.native_optimizers():
        if type(o).__module__.startswith("torch.optim"):
            # torch's own optimizers (Optimizer__Union's other members) count their steps on the host
            raise NotImplementedError(f"{type(o).__name__}: only Adam steps are captured into a HIP graph; run the native step eagerly")
    for o in tr.native_optimizers():
        if hasattr(o, "enable_device_schedule"):
            o.enable_device_schedule()
    tr._graph_mode = True


def require_grad_scaling_optimizers(tr):
    """data parallel on the trainers that fold 1/world into their Adam launches (SAC, TD3, discrete CRR): one of torch's own
    optimizers (Optimizer__Union's other members) has no such argument — refuse rather than step on summed gradients"""
    if getattr(tr, "_dp_world", 1) == 1:
        return
    for o in tr.native_optimizers():
        if type(o).__module__.startswith("torch.optim"):  # (this package's own optimizer classes all scale in their launches)
            raise NotImplementedError(f"{type(tr).__name__}: data parallel needs Adam optimizers (got torch.optim.{type(o).__name__})")


def disable_graph_mode(tr):
    """back to scalar-argument Adam launches (host step counters brought up to date first)"""
    for o in tr.native_optimizers():
        if hasattr(o, "disable_device_schedule"):
            o.disable_device_schedule()
    tr._graph_mode = False


def note_graph_replays(tr, n: int):
    """host-side bookkeeping for n steps that ran as graph replays (no Python in between)"""
    if n <= 0:
        return
    for o in tr.native_optimizers():
        if hasattr(o, "note_device_steps"):
            o.note_device_steps(n)
        for g in o.param_groups:  # the compute-type weight copies of an eager call after the replays are re-staged
            for p in g["params"]:
                p._rg_version = getattr(p, "_rg_version", 0) + 1
    tr.all_batches_processed += n


def accumulating_backward(slab, params, trained, backward):
    """A HIP backward that OVERWRITES the gradient slab, made to accumulate over several batches (a trainer that steps its
    optimizer every k-th batch): the gradients still published through p.grad since the last zero_grad(set_to_none=True) are
    kept, `backward()` runs, and they are added back.  Only the parameters of `trained` (a subset of the slab's `params`) are
    published; the others keep p.grad = None, so an optimizer over all of `params` skips them as torch's would."""
    trained_ids = {id(p) for p in trained}
    held = [(i, slab.view(slab.grad, i).clone()) for i, p in enumerate(params) if id(p) in trained_ids and p.grad is not None]
    backward()
    for i, g in held:
        slab.view(slab.grad, i).add_(g)
    for i, p in enumerate(params):
        if id(p) in trained_ids:
            p.grad = slab.view(slab.grad, i)
