"""CEMPlannerNetwork with the surface of reagent/models/cem_planner.py, executed on the HIP kernels of csrc/cem.hip.

The reference evaluates cem_num_iterations x cem_population_size x ensemble_population_size x plan_horizon_length
mem_net(state, action) calls one at a time on the host.  Here an iteration is a batch on the device: rg_cem_sample draws the
population, rg_cem_group sorts the P * E trajectories by their world model into tiles, rg_cem_rollout rolls them out for the
whole horizon in one launch, rg_cem_refit selects the elites and refits mean and var.  All iterations are enqueued at once
(every launch returns at once after the done flag is set: the reference's early `break`) and the host reads back ONCE.

Kept quirks: the LSTM state is ZERO at every planning step (mem_net is called without a hidden state, :197); the step input
is cat([action, state]).

Departures, each deliberate:
  * ensemble_population_size > 1 gives the mean over a solution's trajectories (in double, in index order).  The reference
    assigns a length-E array to a scalar slot (:186) and raises ValueError for any E > 1.
  * one seed per forward() is drawn from torch's HOST generator (torch.manual_seed reproduces a plan); the reference draws
    from numpy, scipy, `random` and torch's distributions.  The noise recipe is stated in include/reagent_hip.h.
  * the reference's ZeroDivisionError for cem_population_size < 10 is an artefact of a debug log line (:184) and is not kept.
  * the discrete planner draws floor(u * action_dim) per step instead of random.choices over the enumerated product: the
    same distribution without the enumeration.

The members' parameters are read in place through a table of device pointers (rebuilt when a parameter moves), so a training
step's update is seen by the next plan; nothing is copied.
"""
from typing import List, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn

from .. import _lib as L
from .. import ops
from ..core import types as rlt
from ..core.parameters import CONTINUOUS_TRAINING_ACTION_RANGE
from ..preprocessing.trainer_preprocessor import rescale_actions
from . import lstm_stack
from .world_model import MemoryNetwork

F32, F64, I32 = torch.float32, torch.float64, torch.int32


class CEMPlannerNetwork(nn.Module):
    def __init__(
        self,
        mem_net_list: List[MemoryNetwork],
        cem_num_iterations: int,
        cem_population_size: int,
        ensemble_population_size: int,
        num_elites: int,
        plan_horizon_length: int,
        state_dim: int,
        action_dim: int,
        discrete_action: bool,
        terminal_effective: bool,
        gamma: float,
        alpha: float = 0.25,
        epsilon: float = 0.001,
        action_upper_bounds: Optional[np.ndarray] = None,
        action_lower_bounds: Optional[np.ndarray] = None,
    ):
        super().__init__()
        mem_net_list = list(mem_net_list)
        if not mem_net_list:
            raise ValueError("CEMPlannerNetwork: mem_net_list is empty")
        for m in mem_net_list:
            if not isinstance(m, MemoryNetwork) or not hasattr(m.mdnrnn, "_run"):
                raise NotImplementedError(f"CEMPlannerNetwork: every world model must be a reagent_amd MemoryNetwork (got "
                                          f"{type(m).__name__}): the rollout reads its MDNRNN's parameters in place")
        if len(mem_net_list) > L.CEM_MAX_MODELS:
            raise NotImplementedError(f"CEMPlannerNetwork: {len(mem_net_list)} world models are not supported (at most {L.CEM_MAX_MODELS})")
        first = mem_net_list[0]
        dims = lambda m: (m.state_dim, m.action_dim, m.num_hiddens, m.num_hidden_layers, m.num_gaussians)  # noqa: E731
        for m in mem_net_list:
            if dims(m) != dims(first):
                raise NotImplementedError(f"CEMPlannerNetwork: world models of differing dimensions {dims(first)} and {dims(m)}")
        if (first.state_dim, first.action_dim) != (state_dim, action_dim):
            raise NotImplementedError(f"CEMPlannerNetwork: state_dim / action_dim ({state_dim}, {action_dim}) are not the world "
                                      f"models' ({first.state_dim}, {first.action_dim})")
        if state_dim + action_dim > L.CEM_MAX_INPUT:
            raise NotImplementedError(f"CEMPlannerNetwork: state_dim + action_dim = {state_dim + action_dim} is not supported "
                                      f"(at most {L.CEM_MAX_INPUT})")
        if cem_population_size < 1 or ensemble_population_size < 1 or cem_num_iterations < 1 or plan_horizon_length < 1:
            raise ValueError("CEMPlannerNetwork: population, ensemble, iterations and horizon must be at least 1")
        if cem_population_size * ensemble_population_size >= L.CEM_MAX_TRAJECTORIES:
            raise NotImplementedError(f"CEMPlannerNetwork: cem_population_size * ensemble_population_size = "
                                      f"{cem_population_size * ensemble_population_size} is not supported (below 2^20)")
        if plan_horizon_length > L.CEM_MAX_HORIZON:
            raise NotImplementedError(f"CEMPlannerNetwork: plan_horizon_length {plan_horizon_length} is not supported "
                                      f"(at most {L.CEM_MAX_HORIZON})")
        if not discrete_action and not 1 <= num_elites <= cem_population_size:
            raise ValueError(f"CEMPlannerNetwork: num_elites {num_elites} is outside [1, cem_population_size = {cem_population_size}]")
        self.mem_net_list = nn.ModuleList(mem_net_list)
        self.cem_num_iterations = cem_num_iterations
        self.cem_pop_size = cem_population_size
        self.ensemble_pop_size = ensemble_population_size
        self.num_elites = num_elites
        self.plan_horizon_length = plan_horizon_length
        self.state_dim = state_dim
        self.action_dim = action_dim
        self.terminal_effective = terminal_effective
        self.gamma = gamma
        self.alpha = alpha
        self.epsilon = epsilon
        self.discrete_action = discrete_action
        if not discrete_action:
            if action_upper_bounds is None or action_lower_bounds is None:
                raise ValueError("CEMPlannerNetwork: continuous planning needs action_upper_bounds and action_lower_bounds")
            action_upper_bounds, action_lower_bounds = np.asarray(action_upper_bounds), np.asarray(action_lower_bounds)
            assert action_upper_bounds.shape == action_lower_bounds.shape == (action_dim,)
            assert np.all(action_upper_bounds >= action_lower_bounds)
            self.action_upper_bounds = np.tile(action_upper_bounds, self.plan_horizon_length)
            self.action_lower_bounds = np.tile(action_lower_bounds, self.plan_horizon_length)
            self.orig_action_upper = torch.tensor(action_upper_bounds)
            self.orig_action_lower = torch.tensor(action_lower_bounds)
        self._table = None  # (key, int64 tensor [M, 3 L + 2] of parameter pointers)
        self._const = {}  # device -> gamma_pow and the tiled bounds, resident
        self.last_plan = None  # what the last forward() read back (iterations run; the discrete tallies)

    # ---- plumbing --------------------------------------------------------------------------------------------------
    def _device(self):
        devs = {p.device for m in self.mem_net_list for p in m.parameters()}
        if len(devs) != 1:
            raise NotImplementedError(f"CEMPlannerNetwork: the world models live on different devices {sorted(map(str, devs))}")
        return next(iter(devs))

    def _member_params(self, m):
        net = m.mdnrnn
        out = []
        for k in range(net.num_hidden_layers):
            w_ih, _w_hh, b_ih, b_hh = lstm_stack.layer_params(net.rnn, k)
            out += [w_ih, b_ih, b_hh]
        return out + [net.gmm_linear.weight, net.gmm_linear.bias]

    def _pointer_table(self, dev):
        """device pointers of every member's rnn.weight_ih_l*, bias_ih_l*, bias_hh_l*, gmm_linear.weight / bias: the
        parameters themselves (shared with the trainers), so an optimizer step is seen by the next plan"""
        params = [p for m in self.mem_net_list for p in self._member_params(m)]
        for p in params:
            assert p.dtype == F32 and p.is_contiguous(), "world-model parameters are contiguous fp32"
        key = tuple(p.data_ptr() for p in params)
        if self._table is None or self._table[0] != key or self._table[1].device != dev:
            cols = len(params) // len(self.mem_net_list)
            self._table = (key, torch.tensor(key, dtype=torch.int64).view(len(self.mem_net_list), cols).to(dev))
        return self._table[1]

    def _constants(self, dev):
        c = self._const.get(dev)
        if c is None:
            c = {"gamma_pow": torch.tensor([self.gamma ** j for j in range(self.plan_horizon_length)], dtype=F32).to(dev)}
            if not self.discrete_action:
                c["lower"] = torch.from_numpy(self.action_lower_bounds.astype(np.float64)).to(dev)
                c["upper"] = torch.from_numpy(self.action_upper_bounds.astype(np.float64)).to(dev)
            self._const[dev] = c
        return c

    def _refuse_capture(self):
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            raise NotImplementedError("CEMPlannerNetwork: planning is not captured into a HIP graph (it allocates its buffers "
                                      "and reads the plan back); run it eagerly")

    @staticmethod
    def _draw_seed() -> int:
        return int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())  # torch's HOST generator

    def _rollout(self, init_state, solutions, action_idx, out, *, seed=0, iteration=0, done=None, noise=None, trace=False,
                 grouping=None):
        """one iteration's accumulated rewards into out [P] (float64).  noise: None (drawn in the kernels from seed and
        iteration) or a dict u_model [N], u_mix [T, N], eps [T, N, S], u_term [T, N]; grouping: None or (rowmap, tile_model)
        in place of rg_cem_group's; trace: also return the [T, N, S + W + 2] trace"""
        dev = out.device
        first = self.mem_net_list[0]
        P, E, T, S = out.numel(), self.ensemble_pop_size, self.plan_horizon_length, self.state_dim
        N, M = P * E, len(self.mem_net_list)
        tiles = ops.cem_rollout_tiles(N, M)
        noise = noise or {}
        if grouping is None:
            rowmap = torch.empty(tiles * 32, dtype=I32, device=dev)
            tile_model = torch.empty(tiles, dtype=I32, device=dev)
            ops.cem_group(noise.get("u_model"), seed, iteration, N, M, done, rowmap, tile_model)
        else:
            rowmap, tile_model = grouping
        W = (2 * S + 1) * first.num_gaussians + 2
        tr = torch.zeros(T, N, S + W + 2, dtype=F32, device=dev) if trace else None
        traj = torch.empty(N, dtype=F64, device=dev) if E > 1 else None
        ops.cem_rollout(self._pointer_table(dev), rowmap, tile_model, init_state, solutions, action_idx,
                        self._constants(dev)["gamma_pow"], self.action_dim, first.num_gaussians, first.num_hiddens,
                        self.terminal_effective, E, out, traj=traj, u_mix=noise.get("u_mix"), eps=noise.get("eps"),
                        u_term=noise.get("u_term"), seed=seed, iteration=iteration, done=done, trace=tr)
        return tr

    def _init_state(self, state: rlt.FeatureData, dev):
        x = state.float_features
        assert x.shape == (1, self.state_dim)
        return x.detach().to(dev).float().contiguous().view(-1)

    # ---- the reference's surface -----------------------------------------------------------------------------------
    @torch.no_grad()
    def forward(self, state: rlt.FeatureData):
        assert state.float_features.shape == (1, self.state_dim)
        if self.discrete_action:
            return self.discrete_planning(state)
        return self.continuous_planning(state)

    @torch.no_grad()
    def acc_rewards_of_all_solutions(self, state: rlt.FeatureData, solutions: torch.Tensor, seed: Optional[int] = None,
                                     iteration: int = 0) -> np.ndarray:
        """:170-190 — the accumulated reward of each of solutions [cem_pop_size, plan_horizon_length, action_dim]: a float64
        vector of cem_pop_size (with ensemble_population_size > 1 the mean over a solution's trajectories: a departure)"""
        self._refuse_capture()
        dev = self._device()
        seed = self._draw_seed() if seed is None else seed
        sol = solutions.detach().to(dev).float().contiguous()
        assert sol.shape[1:] == (self.plan_horizon_length, self.action_dim)
        out = torch.empty(sol.shape[0], dtype=F64, device=dev)
        self._rollout(self._init_state(state, dev), sol, None, out, seed=seed, iteration=iteration)
        return out.cpu().numpy()

    @torch.no_grad()
    def acc_rewards_of_one_solution(self, init_state: torch.Tensor, solution: torch.Tensor, solution_idx: int,
                                    seed: Optional[int] = None):
        """:121-168 — the rewards of the ensemble_pop_size trajectories of one solution [plan_horizon_length, action_dim]: the
        same kernels on one row per trajectory"""
        self._refuse_capture()
        dev = self._device()
        seed = self._draw_seed() if seed is None else seed
        E = self.ensemble_pop_size
        sol = solution.detach().to(dev).float().reshape(1, self.plan_horizon_length, self.action_dim)
        sol = sol.repeat(E, 1, 1).contiguous()  # a population of E copies, one trajectory each
        out = torch.empty(E, dtype=F64, device=dev)
        single = CEMPlannerNetwork.__new__(CEMPlannerNetwork)
        single.__dict__.update(self.__dict__)
        single.ensemble_pop_size = 1
        single._rollout(init_state.detach().to(dev).float().contiguous().view(-1), sol, None, out, seed=seed, iteration=solution_idx)
        return out.cpu().numpy()

    @torch.no_grad()
    def sample_reward_next_state_terminal(self, state: rlt.FeatureData, action: rlt.FeatureData, mem_net: MemoryNetwork,
                                          seed: Optional[int] = None):
        """:192-215 — one step of one trajectory under mem_net: (reward, next_state, not_terminal, not_terminal_prob)"""
        self._refuse_capture()
        dev = self._device()
        seed = self._draw_seed() if seed is None else seed
        one = CEMPlannerNetwork([mem_net], 1, 1, 1, 1, 1, self.state_dim, self.action_dim, True, self.terminal_effective, 1.0)
        out = torch.empty(1, dtype=F64, device=dev)
        sol = action.float_features.detach().to(dev).float().reshape(1, 1, self.action_dim).contiguous()
        init = state.float_features.detach().to(dev).float().contiguous().view(-1)
        tr = one._rollout(init, sol, None, out, seed=seed, trace=True).cpu()
        S, G = self.state_dim, mem_net.num_gaussians
        z = tr[0, 0, S:-2]
        k, nt = int(tr[0, 0, -2]), int(tr[0, 0, -1])
        mu = z[k * S:(k + 1) * S].double()
        sigma = torch.exp(z[G * S + k * S:G * S + (k + 1) * S].double())
        eps = torch.empty(1, 1, S, dtype=F32, device=dev)
        scratch = [torch.empty(1, dtype=F32, device=dev), torch.empty(1, 1, dtype=F32, device=dev), torch.empty(1, 1, dtype=F32, device=dev)]
        ops.cem_fill_noise(seed, 0, scratch[0], scratch[1], eps, scratch[2])
        next_state = (mu + sigma * eps.cpu().view(-1).double()).float()
        prob = torch.sigmoid(z[-1]) if self.terminal_effective else 1.0
        return z[-2], next_state, nt, prob

    def constrained_variance(self, mean, var):
        lb_dist, ub_dist = (mean - self.action_lower_bounds, self.action_upper_bounds - mean)
        return np.minimum(np.minimum((lb_dist / 2) ** 2, (ub_dist / 2) ** 2), var)

    @torch.no_grad()
    def continuous_planning(self, state: rlt.FeatureData, *, seed: Optional[int] = None, noise=None, record=None) -> torch.Tensor:
        """:224-270 — all cem_num_iterations iterations are enqueued, then ONE readback: mean[:action_dim] and the number of
        iterations run.  noise: None or a list, per iteration, of dicts tn [P, D] float64, u_model, u_mix, eps, u_term (the
        explicit noise of include/reagent_hip.h); record: a list that receives, per iteration, device copies of the
        solutions, the accumulated rewards and the planner state (tests)."""
        if self.discrete_action:
            raise ValueError("continuous_planning on a discrete-action planner")
        self._refuse_capture()
        dev = self._device()
        seed = self._draw_seed() if seed is None else seed
        c = self._constants(dev)
        P, T, A = self.cem_pop_size, self.plan_horizon_length, self.action_dim
        D = T * A
        mean = (self.action_upper_bounds + self.action_lower_bounds) / 2
        var = (self.action_upper_bounds - self.action_lower_bounds) ** 2 / 16
        ps = torch.from_numpy(np.concatenate([mean, var, [0.0, 0.0]]).astype(np.float64)).to(dev)
        done = ps[2 * D:]
        init = self._init_state(state, dev)
        sol, sol32 = torch.empty(P, D, dtype=F64, device=dev), torch.empty(P, D, dtype=F32, device=dev)
        rewards = torch.zeros(P, dtype=F64, device=dev)
        flags = torch.empty(P, dtype=I32, device=dev)
        for i in range(self.cem_num_iterations):
            nz = noise[i] if noise is not None else {}
            ops.cem_sample(ps, c["lower"], c["upper"], seed, i, sol, sol32, tn=nz.get("tn"))
            self._rollout(init, sol32.view(P, T, A), None, rewards, seed=seed, iteration=i, done=done, noise=nz)
            ops.cem_refit(rewards, sol, self.num_elites, self.alpha, self.epsilon, ps, flags)
            if record is not None:
                record.append(dict(solutions=sol.clone(), rewards=rewards.clone(), state=ps.clone(), elites=flags.clone()))
        host = ps.cpu().numpy()  # the one readback
        self.last_plan = dict(iterations=int(host[2 * D + 1]), seed=seed, mean=host[:D].copy(), var=host[D:2 * D].copy())
        raw_action = host[:A].reshape(-1)
        low = torch.tensor(CONTINUOUS_TRAINING_ACTION_RANGE[0])
        high = torch.tensor(CONTINUOUS_TRAINING_ACTION_RANGE[1])
        return rescale_actions(torch.tensor(raw_action), new_min=low, new_max=high, prev_min=self.orig_action_lower,
                               prev_max=self.orig_action_upper)

    @torch.no_grad()
    def discrete_planning(self, state: rlt.FeatureData, *, seed: Optional[int] = None, noise=None, actions=None,
                          record=None) -> Tuple[int, torch.Tensor]:
        """:272-307 — random shooting: (best_next_action_idx, its one-hot), with one readback (the tallies).  actions: None or
        the [P, T] int32 action indices in place of the draw; noise as in continuous_planning (one dict)."""
        if not self.discrete_action:
            raise ValueError("discrete_planning on a continuous-action planner")
        self._refuse_capture()
        dev = self._device()
        seed = self._draw_seed() if seed is None else seed
        P, T, A = self.cem_pop_size, self.plan_horizon_length, self.action_dim
        if actions is None:
            actions = torch.empty(P, T, dtype=I32, device=dev)
            ops.cem_sample_discrete(seed, 0, A, actions)
        else:
            actions = actions.to(dev).to(I32).contiguous()
        rewards = torch.empty(P, dtype=F64, device=dev)
        self._rollout(self._init_state(state, dev), None, actions, rewards, seed=seed, noise=noise)
        tally = torch.empty(3 * A + 1, dtype=F64, device=dev)
        ops.cem_tally(actions, rewards, A, tally)
        if record is not None:
            record.append(dict(actions=actions.clone(), rewards=rewards.clone()))
        host = tally.cpu().numpy()  # the one readback
        self.last_plan = dict(first_action_tally=host[:A], reward_tally=host[A:2 * A], seed=seed)
        best = int(host[3 * A])
        if best < 0:
            raise ValueError("All-NaN slice encountered")  # np.nanargmax's
        best_next_action_idx = np.int64(best)
        best_next_action_one_hot = torch.zeros(A).float()
        best_next_action_one_hot[best] = 1
        return best_next_action_idx, best_next_action_one_hot
