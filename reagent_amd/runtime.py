"""The offline batch-RL step loop on one GPU: what OfflineReplayBufferDataset + pl.Trainer.fit do in
the reference (reagent/gym/datasets/replay_buffer_dataset.py:153-206), without a
dataloader, Lightning or host synchronisation:

    indices = sample_index_batch(B)                       (device RNG)
    batch   = ReplayBuffer.sample_transition_batch     \
    input   = DiscreteDqnInputMaker(batch)              }  rg_replay_dqn_batch (one launch; generic stores:
    state, next_state = Preprocessor(...)              /   rg_replay_nstep + rg_replay_gather + rg_make_dqn_input)
    trainer.train_step_native(input)                       FC fwd x3, head, bwd, Adam, soft update
Everything is enqueued on torch's current stream; the loss stays on the device.
`prefetch=True` moves the sampling / gather / input-maker launches of batch k+1 to a second HIP stream
while step k computes.  Measured on one MI355X (same box, C2): 0.642 ms/step with it against 0.615
without — the fused MLP kernels fill every CU's registers and LDS, so the gather only runs in their
tails and slows them more than it hides; it is therefore OFF by default and kept as an option.
(Round 3: releasing the next batch's sampler only beside the step's WEIGHT GRADIENT — bound by its operand stream,
167 registers per wave, so the sampler's waves fit next to it on every CU — through a hook before that launch measured
0.616-0.622 ms/step against 0.568-0.571 without any prefetch and 0.607-0.610 with the free-running one, same box; bf16x3
1.237-1.241 against 1.179-1.181.  Two kernels sharing the memory system plus two cross-stream waits per step cost more
than the 40 us they hide; not kept.)
"""
from typing import Optional

import torch

from .core import types as rlt
from .preprocessing import DiscreteDqnInputMaker, Preprocessor
from .replay_memory import ReplayBuffer


class _GraphedLoop:
    """HIP-graph replay of the loop's step (SURVEY.md §8e / VERDICT r1 #6): `capture()` records ONE step — index
    draw, sampler, forwards, loss head, backward, wgrad, Adam + soft update + re-staging — and returns a callable
    that replays it; per step the host then issues one graph launch instead of ~10-40 ctypes calls.

    What makes a recorded step valid for every later step:
      * the index draw (torch.randint on the device) and SAC's N(0,1) draws use torch's graph-safe Philox state;
      * Adam's step-dependent coefficients are read from HBM (optimizer.AdamSchedule, rg_*_sched entry points) —
        launch arguments would be frozen at their capture-time values;
      * every buffer the step touches is either persistent (trainer workspaces) or allocated during capture from
        the graph's private pool (the batch), so addresses are stable.
    Data parallel (world > 1): three graphs — sample | update | forward+backward — with the RCCL all-reduce of the
    gradient slab launched eagerly between them, in the deferred-update order of `step()`: the collective is never
    captured, the next batch is still gathered under it.
    `flush()` brings the host-side counters (Adam steps, all_batches_processed) up to date."""

    _graph = None
    _replays = 0
    replay_steps = 1  # steps one replay() makes (capture(steps_per_replay=))
    # Index draws of `index_pool_steps` steps come from ONE torch.randint launch (the per-step draw was the last
    # torch kernel on the C2 step: 5 us of 540); a step then only slices the pool.  1 = a draw per step.  Inside a
    # graph capture the per-step draw stays (torch's graph-safe Philox state is what makes a replay draw afresh).
    index_pool_steps = 32
    _pool = None
    _pool_pos = 0
    _pool_key = None
    _pool_n = None  # the valid-slot count the pool was drawn for

    def _eager_step(self, indices=None):
        raise NotImplementedError

    def _ensure_pool(self, dev):
        """a pool with at least one undrawn row.  A full-size pool is refilled IN PLACE (a replayed graph may hold its
        address); the shorter rest a checkpoint restored is replaced by a full one once it is used up."""
        rb = self.rb
        n, cap = rb._num_valid_indices, rb._replay_capacity
        key = (n, cap, self.batch_size, self.index_pool_steps)
        shape = (self.index_pool_steps, self.batch_size)
        if self._pool is None or self._pool_key != key or (self._pool_pos >= self._pool.shape[0] and tuple(self._pool.shape) != shape):
            self._pool = torch.randint(n, shape, device=dev)
            self._pool_pos, self._pool_key = 0, key
        elif self._pool_pos >= self._pool.shape[0]:
            torch.randint(n, shape, out=self._pool)
            self._pool_pos = 0

    def _draw_indices(self):
        """indices of the next batch from the pool, or None = let the buffer draw (sample_index_batch).  Same
        distribution as sample_index_batch: uniform with replacement over the valid slots."""
        rb = self.rb
        dev = torch.device(rb.device)
        if self.index_pool_steps <= 1 or (dev.type == "cuda" and torch.cuda.is_current_stream_capturing()):
            return None
        n, cap = rb._num_valid_indices, rb._replay_capacity
        if n == 0:
            return None  # the buffer raises its own error
        if self._pool_n is None:
            self._pool_n = n
        elif n != self._pool_n:
            # The number of valid slots moved since the last draw: a buffer that is still filling (online / interleaved add
            # and train).  A pool keyed on it would be redrawn — 32 draws' worth of RNG — on every such step and its undrawn
            # rows dropped, so a checkpointed continuation would stop following the uninterrupted run.  The buffer draws
            # this step itself; pooling resumes once the count has stayed put for a step (a full or a static store).
            self._pool_n, self._pool = n, None
            return None
        self._ensure_pool(dev)
        pick = self._pool[self._pool_pos]
        self._pool_pos += 1
        return pick if n == cap else rb._valid_indices()[pick]

    # ---- checkpoint / resume (what pl.Trainer's checkpointing does for the reference: module + optimizer states) ----
    def checkpoint(self) -> dict:
        """Everything a bit-identical continuation of the loop needs besides the replay storage (ReplayBuffer.save
        writes that in the reference's own file layout): the trainer's state_dict (networks, targets, temperature),
        every optimizer's state_dict (Adam moments and step counts), the step counter and the RNG state the index /
        noise draws continue from.  A pending deferred update is applied first."""
        self.flush()
        tr = self.trainer
        dev = torch.device(self.rb.device)
        rng = torch.cuda.get_rng_state(dev) if dev.type == "cuda" else torch.get_rng_state()
        return dict(
            trainer=tr.state_dict(),
            optimizers=[o.state_dict() if hasattr(o, "state_dict") else None for o in tr.native_optimizers()],
            all_batches_processed=int(getattr(tr, "all_batches_processed", 0)),
            rng_state=rng,
            extras=tr.checkpoint_extras() if hasattr(tr, "checkpoint_extras") else None,
            # the undrawn rest of the index pool: the continuation draws what this loop would have drawn
            index_pool=None if self._pool is None else dict(pool=self._pool[self._pool_pos:].cpu(), key=self._pool_key),
            # the valid-slot count the last draw saw: it decides whether the NEXT step draws from a pool or lets the buffer
            # draw (a still-filling store), so the continuation has to start from the same value
            index_pool_n=self._pool_n,
        )

    def load_checkpoint(self, ckpt: dict):
        """restore `checkpoint()`'s dict into this loop's trainer (built with the same configuration)"""
        if self._graph is not None:
            self.release_graph()
        tr = self.trainer
        tr.load_state_dict(ckpt["trainer"])
        for o, sd in zip(tr.native_optimizers(), ckpt["optimizers"]):
            if sd is not None and hasattr(o, "load_state_dict"):
                o.load_state_dict(sd)
        if hasattr(tr, "all_batches_processed"):
            tr.all_batches_processed = ckpt["all_batches_processed"]
        if ckpt.get("extras") is not None:
            tr.load_checkpoint_extras(ckpt["extras"])
        for p in tr.parameters():  # the engines' staged weight copies follow the version counters
            p._rg_version = getattr(p, "_rg_version", 0) + 1
        dev = torch.device(self.rb.device)
        if dev.type == "cuda":
            torch.cuda.set_rng_state(ckpt["rng_state"].cpu(), dev)
        else:
            torch.set_rng_state(ckpt["rng_state"].cpu())
        ip = ckpt.get("index_pool")
        self._pool = self._pool_key = None
        self._pool_pos = 0
        self._pool_n = ckpt.get("index_pool_n")  # None (older checkpoints / a loop that never drew): the first draw sets it
        if ip is not None and ip["pool"].shape[0] > 0:
            # the rest is shorter than a full pool: it is used up, then a fresh pool is drawn from the restored RNG
            # state — exactly what the saved loop would have done
            self._pool, self._pool_key = ip["pool"].to(dev), tuple(ip["key"])

    def save(self, path: str):
        torch.save(self.checkpoint(), path)

    def load(self, path: str):
        self.load_checkpoint(torch.load(path, map_location="cpu", weights_only=False))

    def capture(self, warmup: int = 2, static_indices: bool = False, steps_per_replay: int = 1):
        """steps_per_replay > 1 (loops with a device-side index cursor only — the DQN family on the one-launch sampler and
        update): that many CONSECUTIVE steps are recorded as one graph, so a replay is that many steps.  Between two graph
        launches the queue idles ~8 us (between two kernels of a stream ~1 us); the cursor and the Adam step count live on the
        device and advance per captured step, so nothing else changes.  Must divide index_pool_steps; `replay.steps` tells
        the caller how many steps a call makes."""
        from .training.plumbing import enable_graph_mode

        tr = self.trainer
        dev = torch.device(self.rb.device)
        if not self._graphs_available(dev):
            raise RuntimeError("HIP graphs need the GPU")
        # every argument error BEFORE the trainer is switched to graph mode, warmed up or captured
        n_steps = max(1, int(steps_per_replay))
        dp = getattr(tr, "_dp_group", None) is not None
        pooled = not static_indices and self.index_pool_steps > 1
        if n_steps > 1:
            if dp or not pooled or type(self)._cursor_protocol is _GraphedLoop._cursor_protocol:
                raise NotImplementedError("steps_per_replay > 1 needs the device-side index cursor (DQN-family loop, one-launch sampler and update)")
            if self.index_pool_steps % n_steps:
                raise ValueError(f"steps_per_replay {n_steps} must divide index_pool_steps {self.index_pool_steps}")
        if dp and not hasattr(tr, "native_forward_backward"):
            raise NotImplementedError("data-parallel graph replay is built for the DQN-family native step")
        enable_graph_mode(tr)
        for _ in range(max(2, warmup)):  # eager: allocations, optimizer state, first-step staging; the step
            self.step()                  # after these is the steady-state launch sequence
        self.flush()
        if dev.type == "cuda":
            torch.cuda.synchronize()
        # Indices: a persistent buffer the captured sampler reads.  Filled by the caller (static_indices) or, by default,
        # from the loop's index pool right before each replay (one 512 KB device copy) — the in-graph torch.randint was
        # THREE kernel nodes (Philox offset bookkeeping + the draw: ~23 us per step, what made the replayed C2 step
        # slower than eager launches).  index_pool_steps <= 1 keeps the draw inside the graph.
        idx = torch.zeros(self.batch_size, dtype=torch.int64, device=dev) if (static_indices or pooled) else None
        done = tr.all_batches_processed
        cursor = None
        if not dp:
            extra = self._capture_buffers(dev)  # persistent inputs besides the indices (the policy loop's noise)
            tick = self._cursor_protocol(dev) if pooled else None
            g = torch.cuda.CUDAGraph()
            if tick is not None:
                # Device-side index cursor: the captured sampler reads row cursor[0] of the loop's index pool and counts
                # the step in the Adam schedule, the captured one-launch update advances the cursor — a replay is the
                # graph launch and nothing else (no index copy, no tick node)
                from . import ops as _ops

                cursor = tick["cursor"]
                tr._graph_tick = tick
                try:
                    with torch.cuda.graph(g, capture_error_mode="thread_local"):
                        for _ in range(n_steps):
                            out = self._eager_step(_ops.PooledIndices(self._pool, cursor, tick["sched"]))
                finally:
                    tr._graph_tick = None
                assert tick.get("used"), "the captured step did not take the one-launch update"
                idx = None
                if n_steps > 1:  # replays start on multiples of n_steps: the rows the warm-up left of its group are skipped
                    self._pool_pos = (self._pool_pos + n_steps - 1) // n_steps * n_steps
            else:
                with torch.cuda.graph(g, capture_error_mode="thread_local"):
                    out = self._eager_step(idx, **extra)
            graphs = (g,)
        else:
            pool = self._new_graph_pool()
            gs, batch = self._record(lambda: self.make_batch(idx), pool)  # recorded in replay order (shared pool)
            gu, _ = self._record(lambda: tr.native_update(), pool)
            gc, out = self._record(lambda: tr.native_forward_backward(batch), pool)
            graphs = (gs, gu, gc)
            self._graph_batch = batch
        tr.all_batches_processed = done  # the capture call ran the host side of a step, not the step
        if cursor is None:
            if n_steps > 1:  # the loop's cursor protocol declined at capture time (checked above; kept as a guard)
                self.release_graph()
                raise NotImplementedError("steps_per_replay > 1 needs the device-side index cursor (DQN-family loop, one-launch sampler and update)")
            n_steps = 1
        self._graph = dict(graphs=graphs, out=out, idx=idx, dp=dp, pending=None, pooled=pooled, extra=extra if not dp else {},
                           cursor=cursor, dev_pos=None, pool_ptr=self._pool.data_ptr() if cursor is not None else None,
                           steps=n_steps)
        self.replay_steps = n_steps
        return self.replay

    # ---- the three hooks through which capture() reaches the graph API (the world-2 gloo test of the data-parallel replay
    # order substitutes re-executing stand-ins for them: tests/test_graph_replay.py) ----
    @staticmethod
    def _graphs_available(dev) -> bool:
        return dev.type == "cuda"

    @staticmethod
    def _new_graph_pool():
        return torch.cuda.graph_pool_handle()

    @staticmethod
    def _record(fn, pool=None):
        """(graph, what fn returned): the launches fn enqueues, recorded as one HIP graph"""
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, pool=pool, capture_error_mode="thread_local"):
            out = fn()
        return g, out

    def _cursor_protocol(self, dev):
        """None, or what a capture with a device-side index cursor needs (the DQN-family loop on the one-launch sampler and
        the one-launch update: overridden there)"""
        return None

    def _capture_buffers(self, dev) -> dict:
        return {}

    def _refill_capture_buffers(self, extra: dict):
        pass

    def replay(self, indices=None):
        G = self._graph
        if G["cursor"] is not None:
            if indices is not None:
                raise ValueError("this loop was captured with a device-side index cursor: replay() draws from the index pool")
            dev = G["cursor"].device
            n = G["steps"]
            if n > 1 and self._pool_pos % n:  # eager steps in between drew from the pool: skip to the next group of rows
                self._pool_pos = (self._pool_pos + n - 1) // n * n
            self._ensure_pool(dev)
            if self._pool.data_ptr() != G["pool_ptr"]:
                raise RuntimeError("the index pool moved (replay buffer or batch size changed): capture the loop again")
            if G["dev_pos"] != self._pool_pos:  # first replay, or eager steps in between drew from the pool
                G["cursor"].fill_(self._pool_pos)
            G["graphs"][0].replay()
            self._pool_pos += n
            G["dev_pos"] = self._pool_pos % self.index_pool_steps
            self._replays += n
            return G["out"]
        if G["idx"] is not None:
            if indices is None:
                if not G["pooled"]:
                    raise ValueError("this loop was captured with static_indices=True: replay(indices) needs them")
                indices = self._draw_indices()
                if indices is None:
                    indices = self.rb.sample_index_batch(self.batch_size)
            G["idx"].copy_(indices)
        if G["extra"]:
            self._refill_capture_buffers(G["extra"])
        if not G["dp"]:
            G["graphs"][0].replay()
            self._replays += 1
            return G["out"]
        gs, gu, gc = G["graphs"]
        tr = self.trainer
        gs.replay()                    # batch k is gathered while all-reduce k-1 is in flight
        self._join_update()
        gc.replay()
        G["pending"] = torch.distributed.all_reduce(tr._slab.grad, group=tr._dp_group, async_op=True)
        return G["out"]

    def _join_update(self):
        G = self._graph
        if G is not None and G["pending"] is not None:
            G["pending"].wait()        # the compute stream waits for the collective; the host does not
            G["pending"] = None
            G["graphs"][1].replay()
            self._replays += 1

    def release_graph(self):
        """drop the captured graph(s) and return the optimizers to scalar-argument launches"""
        from .training.plumbing import disable_graph_mode

        self.flush()
        self._graph = None
        disable_graph_mode(self.trainer)

    def _flush_graph(self):
        from .training.plumbing import note_graph_replays

        self._join_update()
        note_graph_replays(self.trainer, self._replays)
        self._replays = 0


class OfflineDqnLoop(_GraphedLoop):
    def __init__(self, replay_buffer: ReplayBuffer, trainer, batch_size: int,
                 state_preprocessor: Optional[Preprocessor] = None, state_dtype=None, prefetch: bool = False):
        self.rb = replay_buffer
        self.trainer = trainer
        self.batch_size = batch_size
        self.pre = state_preprocessor
        self.maker = DiscreteDqnInputMaker(trainer.num_actions)
        self._presence = None
        self.state_dtype = state_dtype
        # 1:1 normalization tables ride along with the gather (no separate normalize pass)
        self.fuse_norm = state_preprocessor is not None and state_preprocessor.elementwise
        self.fused_sampling = True
        self.prefetch = prefetch and torch.device(replay_buffer.device).type == "cuda"
        self._side = None
        self._ready = None  # (batch, event) of the prefetched next batch

    def make_batch(self, indices: Optional[torch.Tensor] = None) -> rlt.DiscreteDqnInput:
        if self.fused_sampling and (self.fuse_norm or self.pre is None):
            # one launch: n-step bookkeeping + both state gathers (+ normalization) + input maker
            inp = self.rb.sample_dqn_input(self.trainer.num_actions, self.batch_size, indices=indices,
                                           state_preprocessor=self.pre, state_dtype=self.state_dtype)
            if inp is not None:
                return inp
            self.fused_sampling = False  # this store is not of the fused kernel's shape
        if self.fuse_norm:
            tup = self.rb.sample_transition_batch(self.batch_size, indices=indices, state_preprocessor=self.pre,
                                                  state_dtype=self.state_dtype)
            return self.maker(tup)
        tup = self.rb.sample_transition_batch(self.batch_size, indices=indices)
        inp = self.maker(tup)
        if self.pre is not None:
            s, ns = inp.state.float_features, inp.next_state.float_features
            if self._presence is None or self._presence.shape != s.shape or self._presence.device != s.device:
                self._presence = torch.ones(s.shape, dtype=torch.uint8, device=s.device)
            inp.state = rlt.FeatureData(self.pre(s, self._presence))
            inp.next_state = rlt.FeatureData(self.pre(ns, self._presence))
        return inp

    @staticmethod
    def _tensors(obj):
        if isinstance(obj, torch.Tensor):
            yield obj
        elif hasattr(obj, "__dataclass_fields__"):
            for name in obj.__dataclass_fields__:
                yield from OfflineDqnLoop._tensors(getattr(obj, name))

    def _launch_prefetch(self):
        main = torch.cuda.current_stream()
        if self._side is None:
            self._side = torch.cuda.Stream()
            self._side.wait_stream(main)  # once: after whatever filled the replay storage; later launches
            # depend on nothing the training step writes
        with torch.cuda.stream(self._side):
            batch = self.make_batch()
            ev = torch.cuda.Event()
            ev.record(self._side)
        for t in self._tensors(batch):  # allocated on the side stream, consumed on the main one
            t.record_stream(main)
        return batch, ev

    def step(self, indices: Optional[torch.Tensor] = None) -> torch.Tensor:
        # data parallel: the previous step's gradient all-reduce is still in flight here, and the
        # gather does not depend on it — the trainer joins it right before Adam
        if not self.prefetch or indices is not None:
            batch = self.make_batch(indices if indices is not None else self._draw_indices())
            return self.trainer.train_step_native(batch, defer_update=True)
        if self._ready is None:
            self._ready = self._launch_prefetch()
        batch, ev = self._ready
        torch.cuda.current_stream().wait_event(ev)
        loss = self.trainer.train_step_native(batch, defer_update=True)
        self._ready = self._launch_prefetch()  # batch k+1 travels while step k computes
        return loss

    def _eager_step(self, indices=None):
        return self.trainer.train_step_native(self.make_batch(indices if indices is not None else self._draw_indices()))

    def _cursor_protocol(self, dev):
        tr, rb = self.trainer, self.rb
        if not (self.fused_sampling and (self.fuse_norm or self.pre is None)) or rb._num_valid_indices != rb._replay_capacity:
            return None
        if getattr(tr, "_cpe", None) is not None or not isinstance(getattr(tr, "_fused_plan", None), dict):
            return None  # (the warm-up steps of capture() have run: the one-launch update has shown itself by now)
        opts = tr.native_optimizers()
        sched = opts[0].schedule_for(0) if hasattr(opts[0], "schedule_for") else None
        if sched is None:
            return None
        self._ensure_pool(dev)
        if tuple(self._pool.shape) != (self.index_pool_steps, self.batch_size):
            self._pool_pos = self._pool.shape[0]  # (the short rest of a restored checkpoint: start a full pool)
            self._ensure_pool(dev)
        return dict(cursor=torch.zeros(1, dtype=torch.int64, device=dev), mod=self.index_pool_steps, sched=sched.buf, used=False)

    def flush(self):
        """apply an update left pending by the last step (call before reading parameters)"""
        self._flush_graph()
        self.trainer.apply_pending_update()


class OfflineTableLoop:
    """Epochs over an offline (post-timeline) table resident in HBM: what the reference's petastorm
    DataLoader + DiscreteDqnBatchPreprocessor + pl.Trainer.fit do for batch RL from a dataset
    (reagent/data/oss_data_fetcher.py, reagent/preprocessing/batch_preprocessor.py:35-66,
    reagent/workflow/training.py), with the table as one device array per column:

        for indices in table.epoch(batch_size):             (device permutation, no host sync)
            batch = batch_preprocessor.from_table(table, indices)     rg_table_dqn_batch (one launch)
            trainer.train_step_native(batch)                 FC fwd x3, head, bwd, Adam, soft update
    """

    def __init__(self, table, trainer, batch_preprocessor, batch_size: int, shuffle: bool = True,
                 generator: Optional[torch.Generator] = None):
        self.table, self.trainer, self.bp = table, trainer, batch_preprocessor
        self.batch_size, self.shuffle, self.generator = batch_size, shuffle, generator
        self.batches_done = 0

    def run_epoch(self) -> Optional[torch.Tensor]:
        """one pass over the table (the last partial batch is dropped); returns the last loss (device)"""
        loss = None
        deferred = hasattr(self.trainer, "apply_pending_update")
        for indices in self.table.epoch(self.batch_size, shuffle=self.shuffle, generator=self.generator):
            batch = self.bp.from_table(self.table, indices)
            loss = self.trainer.train_step_native(batch, defer_update=True) if deferred \
                else self.trainer.train_step_native(batch)
            self.batches_done += 1
        if deferred:
            self.trainer.apply_pending_update()
        return loss


class OfflinePolicyLoop(_GraphedLoop):
    """The same loop for continuous-action trainers (SAC / TD3, BASELINE C4): uniform index draw ->
    ReplayBuffer.sample_transition_batch (rg_replay_nstep + rg_replay_gather, state rows normalized on the
    way when a 1:1 Preprocessor is given) -> PolicyNetworkInputMaker -> trainer.train_step_native, the
    actor's N(0,1) draws taken from the device RNG."""

    def __init__(self, replay_buffer: ReplayBuffer, trainer, batch_size: int, input_maker,
                 state_preprocessor: Optional[Preprocessor] = None, state_dtype=None):
        """state_dtype=torch.bfloat16 (with a state_preprocessor, bf16 engine): the gather writes the normalized state
        rows in the networks' operand type — half the bytes for the sampler to write and for each of the step's eight
        forwards to read, the same bf16 values the kernels would make of the fp32 rows"""
        self.rb, self.trainer, self.batch_size, self.maker = replay_buffer, trainer, batch_size, input_maker
        self.pre = state_preprocessor
        self.state_dtype = state_dtype if state_preprocessor is not None else None
        if state_preprocessor is not None and not state_preprocessor.elementwise:
            raise NotImplementedError("normalize-on-gather needs a 1:1 column table")

    def make_batch(self, indices: Optional[torch.Tensor] = None) -> rlt.PolicyNetworkInput:
        # rg_replay_policy_batch (one launch) where the store has the shape it serves, else the three-launch path
        if hasattr(self.rb, "sample_policy_input"):
            batch = self.rb.sample_policy_input(self.maker, self.batch_size, indices=indices, state_preprocessor=self.pre,
                                                state_dtype=self.state_dtype)
            if batch is not None:
                return batch
        tup = self.rb.sample_transition_batch(self.batch_size, indices=indices, state_preprocessor=self.pre,
                                              state_dtype=self.state_dtype)
        return self.maker(tup)

    # The actor's two N(0,1) draws of `noise_pool_steps` steps come from ONE torch.randn launch (SAC: noise_next, noise_cur of
    # train_step_native; a draw per step is two launches in an eager step and six kernel nodes in a captured one).  1 = a draw
    # per step inside the trainer.  Same distribution, another position in torch's random stream; the pool is re-drawn from
    # its recorded RNG state when a checkpoint is restored.
    noise_pool_steps = 8
    _npool = None
    _npool_pos = 0
    _npool_key = None
    _npool_rng = None
    _noise_dim = None

    def _noise_pooled(self) -> bool:
        if getattr(self, "_noise_ok", None) is None:
            import inspect

            params = inspect.signature(self.trainer.train_step_native).parameters
            self._noise_ok = "noise_next" in params and "noise_cur" in params
        return self._noise_ok and self.noise_pool_steps > 1

    def _draw_noise(self, A: int, dev) -> dict:
        if not self._noise_pooled() or (dev.type == "cuda" and torch.cuda.is_current_stream_capturing()):
            return {}
        key = (self.batch_size, A, self.noise_pool_steps)
        if self._npool is None or self._npool_key != key or self._npool_pos >= self.noise_pool_steps:
            self._npool_rng = torch.cuda.get_rng_state(dev) if dev.type == "cuda" else torch.get_rng_state()
            self._npool = torch.randn(self.noise_pool_steps, 2, self.batch_size, A, device=dev)
            self._npool_pos, self._npool_key = 0, key
        row = self._npool[self._npool_pos]
        self._npool_pos += 1
        return dict(noise_next=row[0], noise_cur=row[1])

    def step(self, indices: Optional[torch.Tensor] = None, **noise):
        batch = self.make_batch(indices if indices is not None else self._draw_indices())
        if not noise:
            a = batch.action.float_features
            self._noise_dim = a.shape[1]
            noise = self._draw_noise(a.shape[1], a.device)
        return self.trainer.train_step_native(batch, **noise)

    def _eager_step(self, indices=None, **noise):
        return self.step(indices, **noise)

    def _capture_buffers(self, dev) -> dict:
        if not self._noise_pooled() or self._noise_dim is None:
            return {}
        shape = (self.batch_size, self._noise_dim)
        return dict(noise_next=torch.zeros(shape, device=dev), noise_cur=torch.zeros(shape, device=dev))

    def _refill_capture_buffers(self, extra: dict):
        dev = extra["noise_next"].device
        row = self._draw_noise(self._noise_dim, dev)
        extra["noise_next"].copy_(row["noise_next"])
        extra["noise_cur"].copy_(row["noise_cur"])

    def checkpoint(self) -> dict:
        ck = super().checkpoint()
        if self._npool is not None and self._npool_pos < self.noise_pool_steps:
            ck["noise_pool"] = dict(rng=self._npool_rng, pos=self._npool_pos, key=self._npool_key)
        return ck

    def load_checkpoint(self, ckpt: dict):
        super().load_checkpoint(ckpt)
        self._npool = self._npool_key = None
        self._npool_pos = 0
        np_ = ckpt.get("noise_pool")
        if np_ is not None:  # re-draw the pool the saved loop was in the middle of, from the RNG state it was drawn at
            dev = torch.device(self.rb.device)
            cuda = dev.type == "cuda"
            now = torch.cuda.get_rng_state(dev) if cuda else torch.get_rng_state()
            (torch.cuda.set_rng_state(np_["rng"].cpu(), dev) if cuda else torch.set_rng_state(np_["rng"].cpu()))
            B, A, P = np_["key"]
            self._npool = torch.randn(P, 2, B, A, device=dev)
            self._npool_pos, self._npool_key, self._npool_rng = int(np_["pos"]), tuple(np_["key"]), np_["rng"]
            (torch.cuda.set_rng_state(now, dev) if cuda else torch.set_rng_state(now))

    def flush(self):
        self._flush_graph()
