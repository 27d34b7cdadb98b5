"""Seeded synthetic transition data of SURVEY.md §8(d): the same CPU generator feeds the oracle,
the parity tests and bench.py (tensors are created on the CPU from a seeded torch.Generator and
then moved), so reference and HIP paths see identical inputs."""
from typing import Dict, Optional

import numpy as np

import torch
import torch.nn.functional as F


def dqn_batch(batch: int, state_dim: int, num_actions: int, seed: int = 0, p_terminal: float = 0.1,
              p_impossible: float = 0.0, with_steps: bool = False,
              n_extra_metrics: int = 0, with_propensity: bool = False) -> Dict[str, torch.Tensor]:
    """Fields of rlt.DiscreteDqnInput as a plain dict of CPU fp32 tensors."""
    g = torch.Generator().manual_seed(seed)
    state = torch.randn(batch, state_dim, generator=g)
    next_state = torch.randn(batch, state_dim, generator=g)
    reward = torch.rand(batch, 1, generator=g)
    not_terminal = (torch.rand(batch, 1, generator=g) > p_terminal).float()
    action = F.one_hot(torch.randint(num_actions, (batch,), generator=g), num_actions).float()
    next_action = F.one_hot(torch.randint(num_actions, (batch,), generator=g), num_actions).float()
    pna = torch.ones(batch, num_actions)
    if p_impossible > 0:
        pna = (torch.rand(batch, num_actions, generator=g) >= p_impossible).float()
        keep = torch.randint(num_actions, (batch,), generator=g)
        pna[torch.arange(batch), keep] = 1.0  # never a non-terminal state without a possible action
    if with_steps:
        step = torch.randint(1, 4, (batch, 1), generator=g).float()
        time_diff = torch.randint(1, 5, (batch, 1), generator=g).float()
    else:
        step = torch.ones(batch, 1)
        time_diff = torch.ones(batch, 1)
    out = dict(state=state, next_state=next_state, reward=reward, not_terminal=not_terminal,
               action=action, next_action=next_action, possible_actions_mask=torch.ones(batch, num_actions),
               possible_next_actions_mask=pna, step=step, time_diff=time_diff)
    if n_extra_metrics:  # extras.metrics of the CPE heads (drawn last: earlier fields keep their values)
        out["metrics"] = torch.rand(batch, n_extra_metrics, generator=g)
    if with_propensity:  # extras.action_probability of the logging policy, in (0.05, 1]
        out["action_probability"] = 0.05 + 0.95 * torch.rand(batch, 1, generator=g)
    return out


def policy_batch(batch: int, state_dim: int, action_dim: int, seed: int = 0,
                 p_terminal: float = 0.1) -> Dict[str, torch.Tensor]:
    """Fields of rlt.PolicyNetworkInput (actions already in the training range)."""
    g = torch.Generator().manual_seed(seed)
    return dict(
        state=torch.randn(batch, state_dim, generator=g),
        next_state=torch.randn(batch, state_dim, generator=g),
        action=torch.rand(batch, action_dim, generator=g) * 1.8 - 0.9,
        next_action=torch.rand(batch, action_dim, generator=g) * 1.8 - 0.9,
        reward=torch.rand(batch, 1, generator=g),
        not_terminal=(torch.rand(batch, 1, generator=g) > p_terminal).float(),
        step=torch.ones(batch, 1), time_diff=torch.ones(batch, 1),
    )


def parametric_batch(batch: int, state_dim: int, action_dim: int, max_num_actions: int, seed: int = 0,
                     p_terminal: float = 0.1, p_impossible: float = 0.0, n_fully_masked: int = 0,
                     with_steps: bool = False) -> Dict[str, torch.Tensor]:
    """Fields of rlt.ParametricDqnInput as a plain dict of CPU fp32 tensors: every state has max_num_actions candidate
    actions (feature vectors, [batch * max_num_actions, action_dim], state-major) and a mask over them.  The first
    n_fully_masked states have no possible next action and are terminal (a non-terminal one would put the -1e9 penalty
    into the TD target); every other state keeps at least one."""
    g = torch.Generator().manual_seed(seed)
    M = max_num_actions
    state = torch.randn(batch, state_dim, generator=g)
    next_state = torch.randn(batch, state_dim, generator=g)
    reward = torch.rand(batch, 1, generator=g)
    not_terminal = (torch.rand(batch, 1, generator=g) > p_terminal).float()
    pa = torch.rand(batch * M, action_dim, generator=g) * 2.0 - 1.0
    pna = torch.rand(batch * M, action_dim, generator=g) * 2.0 - 1.0
    action = pa.reshape(batch, M, action_dim)[torch.arange(batch), torch.randint(M, (batch,), generator=g)].clone()
    next_action = pna.reshape(batch, M, action_dim)[torch.arange(batch), torch.randint(M, (batch,), generator=g)].clone()
    pnm = torch.ones(batch, M)
    if p_impossible > 0:
        pnm = (torch.rand(batch, M, generator=g) >= p_impossible).float()
        pnm[torch.arange(batch), torch.randint(M, (batch,), generator=g)] = 1.0
    if n_fully_masked:
        pnm[:n_fully_masked] = 0.0
        not_terminal[:n_fully_masked] = 0.0
    if with_steps:
        step = torch.randint(1, 4, (batch, 1), generator=g).float()
        time_diff = torch.randint(1, 5, (batch, 1), generator=g).float()
    else:
        step, time_diff = torch.ones(batch, 1), torch.ones(batch, 1)
    return dict(state=state, next_state=next_state, reward=reward, not_terminal=not_terminal, action=action,
                next_action=next_action, possible_actions=pa, possible_actions_mask=torch.ones(batch, M),
                possible_next_actions=pna, possible_next_actions_mask=pnm, step=step, time_diff=time_diff)


def to_parametric_input(d: Dict[str, torch.Tensor], device=None):
    from .core import types as rlt

    t = (lambda x: x.to(device)) if device is not None else (lambda x: x)
    fd = lambda k: rlt.FeatureData(t(d[k]))  # noqa: E731
    return rlt.ParametricDqnInput(
        state=fd("state"), next_state=fd("next_state"), reward=t(d["reward"]), time_diff=t(d["time_diff"]),
        step=t(d["step"]), not_terminal=t(d["not_terminal"]), action=fd("action"), next_action=fd("next_action"),
        possible_actions=fd("possible_actions"), possible_actions_mask=t(d["possible_actions_mask"]),
        possible_next_actions=fd("possible_next_actions"),
        possible_next_actions_mask=t(d["possible_next_actions_mask"]),
        extras=rlt.ExtraData(metrics=t(d["metrics"]) if "metrics" in d else None),
    )


def slateq_batch(batch: int, state_dim: int, doc_dim: int, num_candidates: int, slate_size: int, seed: int = 0,
                 p_terminal: float = 0.1, p_absent: float = 0.3, n_terminal: int = 2, n_sparse: int = 2,
                 with_time_diff: bool = False) -> Dict[str, torch.Tensor]:
    """Fields of rlt.SlateQInput as a plain dict of CPU tensors under the keys rlt.SlateQInput.from_dict reads: every state
    and next state has num_candidates documents (features, a boolean presence mask, a value in (0.05, 1]) and a logged slate
    of slate_size indices into them, drawn over ALL candidates (padded documents get selected).  Every state keeps at least
    one present document.  The first n_terminal rows are terminal with a non-zero first next_action index; the n_sparse
    rows after them have fewer than slate_size present documents in state and next state (slate_size > 1); the last row's
    reward_mask is all false and the one before it has a true entry."""
    g = torch.Generator().manual_seed(seed)
    B, C, K = batch, num_candidates, slate_size
    assert C >= 2 and B >= n_terminal + n_sparse + 2

    def docs():
        features = torch.rand(B, C, doc_dim, generator=g) * 2.0 - 1.0
        mask = torch.rand(B, C, generator=g) >= p_absent
        mask[torch.arange(B), torch.randint(C, (B,), generator=g)] = True
        for i in range(n_terminal, n_terminal + n_sparse):
            mask[i] = False
            mask[i, torch.randperm(C, generator=g)[:1 + (i % max(K - 1, 1))]] = True
        return features, mask, 0.05 + 0.95 * torch.rand(B, C, generator=g)

    cand, item_mask, item_prob = docs()
    next_cand, next_item_mask, next_item_prob = docs()
    not_terminal = (torch.rand(B, 1, generator=g) > p_terminal).float()
    action = torch.randint(C, (B, K), generator=g)
    next_action = torch.randint(C, (B, K), generator=g)
    not_terminal[:n_terminal] = 0.0
    not_terminal[n_terminal:n_terminal + n_sparse] = 1.0
    next_action[:n_terminal, 0] = 1 + torch.randint(C - 1, (n_terminal,), generator=g)
    reward_mask = torch.rand(B, K, generator=g) > 0.5
    reward_mask[B - 1] = False
    reward_mask[B - 2, 0] = True
    time_diff = torch.randint(1, 5, (B, 1), generator=g).float() if with_time_diff else torch.ones(B, 1)
    return dict(state_features=torch.randn(B, state_dim, generator=g), next_state_features=torch.randn(B, state_dim, generator=g),
                candidate_features=cand, next_candidate_features=next_cand, item_mask=item_mask, next_item_mask=next_item_mask,
                item_probability=item_prob, next_item_probability=next_item_prob, action=action, next_action=next_action,
                position_reward=torch.rand(B, K, generator=g), reward_mask=reward_mask, time_diff=time_diff,
                not_terminal=not_terminal)


def to_slateq_input(d: Dict[str, torch.Tensor], device=None):
    from .core import types as rlt

    return rlt.SlateQInput.from_dict({k: (v.to(device) if device is not None else v) for k, v in d.items()})


def pg_trajectory(length: int, state_dim: int, num_actions: int, seed: int = 0, with_mask: bool = False,
                  behaviour_scale: float = 1.0) -> Dict[str, torch.Tensor]:
    """One trajectory under the keys rlt.PolicyGradientInput.from_dict reads: observation [T, S], action [T, A] one-hot
    (int64) drawn from a random behaviour policy (softmax of behaviour_scale * N(0, 1) logits over the allowed actions),
    log_prob [T] of it under that policy, reward [T] ~ N(0, 1), and with_mask a possible_actions_mask [T, A] (fp32) that
    always allows the logged action and at least one more"""
    g = torch.Generator().manual_seed(seed)
    T, A = length, num_actions
    obs = torch.randn(T, state_dim, generator=g)
    logits = torch.randn(T, A, generator=g) * behaviour_scale
    allowed = torch.ones(T, A, dtype=torch.bool)
    if with_mask:
        allowed = torch.rand(T, A, generator=g) < 0.7
        first = torch.randint(A, (T,), generator=g)
        allowed[torch.arange(T), first] = True
        allowed[torch.arange(T), (first + 1 + torch.randint(A - 1, (T,), generator=g)) % A] = True
    logp = torch.log_softmax(logits.masked_fill(~allowed, float("-inf")), dim=1)
    a = torch.multinomial(logp.exp(), 1, generator=g).reshape(T)
    d = dict(observation=obs, action=F.one_hot(a, A), reward=torch.randn(T, generator=g), log_prob=logp[torch.arange(T), a])
    if with_mask:
        d["possible_actions_mask"] = allowed.float()
    return d


def to_pg_input(d: Dict[str, torch.Tensor], device=None):
    from .core import types as rlt

    return rlt.PolicyGradientInput.from_dict({k: (v.to(device) if device is not None else v) for k, v in d.items()})


def memory_network_batch(seq_len: int, batch: int, state_dim: int, action_dim: int, seed: int = 0,
                         p_terminal: float = 0.2) -> Dict[str, torch.Tensor]:
    """The keys rlt.MemoryNetworkInput.from_dict reads, sequence first: state / next_state [T, B, S] ~ N(0, 1) (next_state =
    a noisy linear mix of state and action, so there is something to learn), action [T, B, A] ~ N(0, 1), reward [T, B] ~
    N(0, 1), not_terminal [T, B] in {0, 1} mixed, time_diff ones, step None"""
    g = torch.Generator().manual_seed(seed)
    T, B, S, A = seq_len, batch, state_dim, action_dim
    state = torch.randn(T, B, S, generator=g)
    action = torch.randn(T, B, A, generator=g)
    mix_s = torch.randn(S, S, generator=g) / S ** 0.5
    mix_a = torch.randn(A, S, generator=g) / A ** 0.5
    next_state = state @ mix_s + action @ mix_a + 0.1 * torch.randn(T, B, S, generator=g)
    reward = torch.randn(T, B, generator=g)
    not_terminal = (torch.rand(T, B, generator=g) > p_terminal).float()
    return dict(state=state, action=action, next_state=next_state, reward=reward, not_terminal=not_terminal,
                time_diff=torch.ones(T, B), step=None)


def to_memory_network_input(d: Dict[str, torch.Tensor], device=None):
    from .core import types as rlt

    return rlt.MemoryNetworkInput.from_dict({k: (v.to(device) if device is not None and v is not None else v)
                                             for k, v in d.items()})


def seq2reward_batch(seq_len: int, batch: int, state_dim: int, num_actions: int, seed: int = 0,
                     max_valid_step: Optional[int] = None) -> Dict[str, torch.Tensor]:
    """memory_network_batch's keys for the Seq2Reward trainers: action [T, B, A] one-hot, valid_step [B, 1] int64 in 1 ..
    seq_len (mixed: both ends occur once the batch allows; 1 .. max_valid_step when given: the step predictor has
    multi_steps classes, which may be fewer than seq_len), and a reward [T, B] that depends on the first state and on the
    actions taken (a fixed random score per (state feature, action) plus a per-action offset plus noise), so that planning
    over actions has something to find"""
    g = torch.Generator().manual_seed(seed)
    T, B, S, A = seq_len, batch, state_dim, num_actions
    top = T if max_valid_step is None else min(T, int(max_valid_step))
    state = torch.randn(T, B, S, generator=g)
    next_state = torch.randn(T, B, S, generator=g)
    idx = torch.randint(0, A, (T, B), generator=g)
    action = (idx.unsqueeze(-1) == torch.arange(A)).float()
    score = torch.randn(S, A, generator=g) / S ** 0.5
    offset = torch.randn(A, generator=g)
    reward = ((state[0] @ score).unsqueeze(0).expand(T, B, A).gather(2, idx.unsqueeze(-1)).squeeze(-1) + offset[idx]
              + 0.1 * torch.randn(T, B, generator=g))
    valid_step = torch.randint(1, top + 1, (B, 1), generator=g)
    if B >= 2:
        valid_step[0, 0], valid_step[-1, 0] = 1, top
    return dict(state=state, action=action, next_state=next_state, reward=reward.contiguous(),
                not_terminal=torch.ones(T, B), time_diff=torch.ones(T, B), step=None, valid_step=valid_step)


def to_seq2reward_input(d: Dict[str, torch.Tensor], device=None):
    """MemoryNetworkInput with valid_step (from_dict, as the reference's, does not read it)"""
    b = to_memory_network_input({k: v for k, v in d.items() if k != "valid_step"}, device)
    b.valid_step = d["valid_step"].to(device) if device is not None else d["valid_step"]
    return b


def synthetic_reward_batch(seq_len: int, batch: int, state_dim: int, action_dim: int, seed: int = 0, binary_reward: bool = False,
                           sequence: bool = False) -> Dict[str, torch.Tensor]:
    """A batch for the synthetic-reward nets, as create_data / create_sequence_data of the reference's
    test_synthetic_reward_training.py make theirs: state and action 2 * randn [T, B, .], valid_step [B, 1] int64 in 1 ..
    seq_len (both ends occur once the batch allows), and reward [B, 1] = the sum over each row's last valid_step steps of a
    per-step reward that is a fixed linear function (weights from seed 0 of the shape: every batch has the same task) of
    cat(state, action) (its sigmoid with binary_reward) or, with sequence, of the masked features of the steps before and
    after"""
    T, B, S, A, scale = seq_len, batch, state_dim, action_dim, 2
    weight = scale * torch.randn(S + A, generator=torch.Generator().manual_seed(1000 * S + A))
    g = torch.Generator().manual_seed(seed)
    state = scale * torch.randn(T, B, S, generator=g)
    action = scale * torch.randn(T, B, A, generator=g)
    valid_step = torch.randint(1, T + 1, (B, 1), generator=g)
    if B >= 2:
        valid_step[0, 0], valid_step[-1, 0] = 1, T
    mask = (torch.arange(T).repeat(B, 1) >= (T - valid_step)).float()  # [B, T]
    feature = torch.cat((state, action), dim=2)
    if sequence:
        masked = feature * mask.transpose(0, 1).unsqueeze(-1)
        zero = torch.zeros(1, B, S + A)
        feature = torch.cat((masked[1:], zero), dim=0) + torch.cat((zero, masked[:-1]), dim=0)
    reward_matrix = torch.matmul(feature, weight).transpose(0, 1)
    if binary_reward:
        reward_matrix = torch.sigmoid(reward_matrix)
    reward = (reward_matrix * mask).sum(dim=1).reshape(-1, 1)
    return dict(state=state, action=action, valid_step=valid_step, reward=reward.contiguous())


def to_synthetic_reward_input(d: Dict[str, torch.Tensor], device=None):
    """MemoryNetworkInput with valid_step and reward [B, 1]; the fields the reward trainer does not read are empty, as in the
    reference's test data"""
    from .core import types as rlt

    t = (lambda x: x.to(device)) if device is not None else (lambda x: x)
    empty = torch.tensor([])
    return rlt.MemoryNetworkInput(state=rlt.FeatureData(t(d["state"])), action=rlt.FeatureData(t(d["action"])),
                                  valid_step=t(d["valid_step"]), reward=t(d["reward"]), next_state=empty, step=empty,
                                  not_terminal=empty, time_diff=empty)


def bandit_reward_batch(batch: int, state_dim: int, num_actions: int, seed: int = 0, with_propensities: bool = False,
                        device=None):
    """A seeded rlt.BanditRewardModelInput of logged bandit data: state randn [B, S], a uniformly logged one-hot action [B, A],
    reward [B, 1] = a fixed linear function of the state per action (weights from the shape: every batch has the same task)
    plus 0.1 randn and, with_propensities, action_prob [B, 1] in (0, 1]"""
    from .core import types as rlt

    B, S, A = batch, state_dim, num_actions
    weight = torch.randn(A, S, generator=torch.Generator().manual_seed(1000 * S + A))
    g = torch.Generator().manual_seed(seed)
    state = torch.randn(B, S, generator=g)
    idx = torch.randint(0, A, (B,), generator=g)
    action = torch.nn.functional.one_hot(idx, A).float()
    reward = ((state @ weight.t()).gather(1, idx.view(B, 1)) + 0.1 * torch.randn(B, 1, generator=g)).contiguous()
    prob = (1.0 - 0.9 * torch.rand(B, 1, generator=g)) if with_propensities else None
    t = (lambda x: x.to(device)) if device is not None else (lambda x: x)
    return rlt.BanditRewardModelInput(state=rlt.FeatureData(t(state)), action=t(action), reward=t(reward),
                                      action_prob=t(prob) if prob is not None else None)


def to_dqn_input(d: Dict[str, torch.Tensor], device=None):
    from .core import types as rlt

    t = (lambda x: x.to(device)) if device is not None else (lambda x: x)
    return rlt.DiscreteDqnInput(
        state=rlt.FeatureData(t(d["state"])), next_state=rlt.FeatureData(t(d["next_state"])),
        reward=t(d["reward"]), time_diff=t(d["time_diff"]), step=t(d["step"]),
        not_terminal=t(d["not_terminal"]), action=t(d["action"]), next_action=t(d["next_action"]),
        possible_actions_mask=t(d["possible_actions_mask"]),
        possible_next_actions_mask=t(d["possible_next_actions_mask"]),
        extras=rlt.ExtraData(action_probability=t(d["action_probability"] if "action_probability" in d
                                                  else torch.ones_like(d["reward"])),
                             metrics=t(d["metrics"]) if "metrics" in d else None),
    )


def to_policy_input(d: Dict[str, torch.Tensor], device=None):
    from .core import types as rlt

    t = (lambda x: x.to(device)) if device is not None else (lambda x: x)
    return rlt.PolicyNetworkInput(
        state=rlt.FeatureData(t(d["state"])), next_state=rlt.FeatureData(t(d["next_state"])),
        reward=t(d["reward"]), time_diff=t(d["time_diff"]), step=t(d["step"]),
        not_terminal=t(d["not_terminal"]), action=rlt.FeatureData(t(d["action"])),
        next_action=rlt.FeatureData(t(d["next_action"])), extras=None,
    )


def replay_contents(capacity: int, obs_dim: int, num_actions: int, seed: int = 0,
                    p_terminal: float = 0.005) -> Dict[str, torch.Tensor]:
    """Column contents of a full replay buffer in the gym `Transition` schema."""
    g = torch.Generator().manual_seed(seed)
    return dict(
        observation=torch.randn(capacity, obs_dim, generator=g),
        action=torch.randint(num_actions, (capacity,), generator=g),
        reward=torch.rand(capacity, generator=g),
        terminal=torch.rand(capacity, generator=g) < p_terminal,
        possible_actions_mask=torch.ones(capacity, num_actions),
        log_prob=torch.zeros(capacity),
    )


def fc_init(dims, activations, seed: int = 0):
    """Seeded weights for a FullyConnected stack, drawn like the reference's initialiser
    (reagent/models/fully_connected_network.py:21-23,122-126: W ~ N(0, (gain * sqrt(1/fan_in))^2), b = 0)
    from an explicit CPU generator.  The BASELINE-shape goldens (oracle/make_golden.py, `baseline_*`) load
    these into the reference networks and the parity tests load them into the HIP-backed ones, so fixtures
    of 0.6-2.2 M parameters do not have to carry their initial weights."""
    import math

    g = torch.Generator().manual_seed(seed)
    out = []
    for i, (fan_in, fan_out) in enumerate(zip(dims, dims[1:])):
        try:
            gain = torch.nn.init.calculate_gain(activations[i])
        except ValueError:
            gain = 1.0
        out.append(torch.randn(fan_out, fan_in, generator=g) * (gain * math.sqrt(1.0 / fan_in)))
        out.append(torch.zeros(fan_out))
    return out


def normalization_table(n_features: int, seed: int = 7):
    """(mean, stddev) of n CONTINUOUS features: mean ~ N(0,1), stddev ~ U[0.5, 2)."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n_features, generator=g), torch.rand(n_features, generator=g) * 1.5 + 0.5


class ScriptedEnv:
    """A deterministic stand-in for a gym environment with the attributes the replay-buffer training flow touches
    (`reset`, `step`, `possible_actions_mask`, `action_space`; reagent/gym/datasets/replay_buffer_dataset.py:96-137):
    observations, rewards and masks are closed forms of (episode, step) with exactly representable values, episodes
    end after `episode_lengths[episode % len]` steps.  Used by the parity tests and by oracle/make_golden.py, which
    drives the reference's ReplayBufferDataset with the same script."""

    class _Discrete:
        def __init__(self, n):
            self.n = n

    class _Box:
        def __init__(self, low, high):
            self.low, self.high = np.asarray(low, dtype=np.float32), np.asarray(high, dtype=np.float32)
            self.shape = self.low.shape

    def __init__(self, obs_dim: int, num_actions: int = None, action_low=None, action_high=None,
                 episode_lengths=(5, 3, 7), with_mask: bool = True):
        self.obs_dim, self.episode_lengths = obs_dim, tuple(episode_lengths)
        self.action_space = (self._Discrete(num_actions) if num_actions is not None else self._Box(action_low, action_high))
        self.num_actions, self.with_mask = num_actions, with_mask and num_actions is not None
        self.episode, self.t = -1, 0

    def _obs(self):
        i = np.arange(self.obs_dim)
        return (((self.episode * 31 + self.t * 17 + i * 7) % 23) / 8.0 - 1.0).astype(np.float32)

    @property
    def possible_actions_mask(self):
        if not self.with_mask:
            return None
        m = np.ones(self.num_actions, dtype=np.float32)
        m[(self.episode * 3 + self.t) % self.num_actions] = float((self.episode + self.t) % 3 != 0)
        return m

    def reset(self):
        self.episode += 1
        self.t = 0
        return self._obs()

    def step(self, action):
        a = float(np.asarray(action, dtype=np.float64).sum())
        self.t += 1
        reward = ((self.episode * 5 + self.t * 3) % 11) / 4.0 - 1.0 + 0.125 * a
        terminal = self.t >= self.episode_lengths[self.episode % len(self.episode_lengths)]
        return self._obs(), reward, terminal, {"episode": self.episode, "t": self.t}


class ScriptedAgent:
    """(action, log_prob) as a closed form of a call counter; `post_step` is None (replay_buffer_dataset.py:139)"""

    post_step = None

    def __init__(self, env: ScriptedEnv):
        self.env, self.calls = env, 0

    def act(self, obs, possible_actions_mask=None):
        k = self.calls
        self.calls += 1
        log_prob = -0.125 - 0.25 * (k % 5)
        if self.env.num_actions is not None:
            return int((k * 5 + 3) % self.env.num_actions), log_prob
        sp = self.env.action_space
        frac = ((k * 3 + np.arange(sp.low.size) * 5) % 8) / 8.0  # inside [low, high): rescale_actions asserts the range
        return (sp.low + frac.astype(np.float32) * (sp.high - sp.low)).astype(np.float32), log_prob


def ranking_batch(batch: int, src_seq_len: int, tgt_seq_len: int, state_dim: int, candidate_dim: int, seed: int = 0, device=None):
    """A seeded rlt.PreprocessedRankingInput of logged slates, built through from_input: state randn [B, state_dim], candidates
    randn [B, S, candidate_dim], the logged slate action [B, T] = the first T of a random permutation of the S candidates (distinct
    in a row), its logged propensity in [0.05, 1) (strictly positive) and slate_reward [B, 1] = a fixed linear function (weights
    from the shapes: every batch has the same task) of the state and of the chosen candidates, earlier positions weighing more,
    plus 0.1 randn"""
    from .core import types as rlt

    B, S, T = batch, src_seq_len, tgt_seq_len
    assert 1 <= T <= S, (T, S)
    task = torch.Generator().manual_seed(1000 * state_dim + candidate_dim)
    w_state, w_cand = torch.randn(state_dim, generator=task), torch.randn(candidate_dim, generator=task)
    g = torch.Generator().manual_seed(seed)
    state, candidates = torch.randn(B, state_dim, generator=g), torch.randn(B, S, candidate_dim, generator=g)
    action = torch.stack([torch.randperm(S, generator=g)[:T] for _ in range(B)])
    logged = 0.05 + 0.95 * torch.rand(B, 1, generator=g)
    chosen = candidates.gather(1, action.unsqueeze(2).expand(B, T, candidate_dim))
    position = 1.0 / torch.arange(1, T + 1, dtype=torch.float32)
    reward = (state @ w_state).view(B, 1) + ((chosen @ w_cand) * position).sum(dim=1, keepdim=True) + 0.1 * torch.randn(B, 1, generator=g)
    return rlt.PreprocessedRankingInput.from_input(state=state, candidates=candidates, device=device if device is not None else "cpu",
                                                   action=action, logged_propensities=logged, slate_reward=reward)
