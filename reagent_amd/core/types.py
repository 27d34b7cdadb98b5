"""Batch containers with the field names of the reference's ``reagent.core.types`` ("rlt").

Only what the DQN / QR-DQN / SAC hot path touches: FeatureData (:312-347), ExtraData (:440-450),
ActorOutput (:245-249), DocList (:252-288), BaseInput (:688-769), DiscreteDqnInput (:772-816), SlateQInput (:819-863),
ParametricDqnInput (:866-896), PolicyNetworkInput (:899-915), PolicyGradientInput (:918-974), MemoryNetworkInput (:1017-1046), MemoryNetworkOutput (:1057-1066), Seq2RewardOutput (:1069-1071), SyntheticRewardNetworkOutput, BanditRewardModelInput (:977-995), PreprocessedRankingInput (:453-685), RankingOutput (:1091-1113), CBInput (:1136-1207) and the tensor-method forwarding of TensorDataClass (:49-108).  The trainers in this
package only read attributes, so instances of the reference's own classes work as well.

When the reference package itself is importable (a ReAgent installation this package is dropped into), its OWN
classes are re-exported from here instead of the restatements below: the reference looks trainers' input types up
by class OBJECT — `make_trainer_preprocessor` reads the annotation of `train_step_gen` and indexes a map keyed by
`rlt.DiscreteDqnInput` / `rlt.PolicyNetworkInput` (reagent/gym/preprocessors/trainer_preprocessor.py:39-48) — so
`DQNTrainer.train_step_gen(training_batch: rlt.DiscreteDqnInput, ...)` must name the reference's class there.
`REAGENT_AMD_OWN_TYPES=1` keeps the restatements.
"""
import dataclasses
import logging
from dataclasses import dataclass, field
from typing import Optional

import torch
import torch.nn.functional as F


@dataclass
class TensorDataClass:
    def __getattr__(self, attr):
        if attr.startswith("__") and attr.endswith("__"):
            raise AttributeError(attr)
        tensor_attr = getattr(torch.Tensor, attr, None)
        if tensor_attr is None or not callable(tensor_attr):
            raise AttributeError(f"{type(self).__name__} doesn't have {attr} attribute.")

        def continuation(*args, **kwargs):
            def f(v):
                if isinstance(v, (torch.Tensor, TensorDataClass)) and getattr(v, attr, None) is not None:
                    return getattr(v, attr)(*args, **kwargs)
                if isinstance(v, dict):
                    return {kk: f(vv) for kk, vv in v.items()}
                if isinstance(v, tuple):
                    return tuple(f(vv) for vv in v)
                return v

            return type(self)(**f(self.__dict__))

        return continuation

    def cuda(self, *args, **kwargs):
        out = {}
        for k, v in self.__dict__.items():
            if isinstance(v, torch.Tensor):
                kwargs["non_blocking"] = kwargs.get("non_blocking", True)
                out[k] = v.cuda(*args, **kwargs)
            elif isinstance(v, TensorDataClass):
                out[k] = v.cuda(*args, **kwargs)
            else:
                out[k] = v
        return type(self)(**out)

    def cpu(self):
        out = {}
        for k, v in self.__dict__.items():
            out[k] = v.cpu() if isinstance(v, (torch.Tensor, TensorDataClass)) else v
        return type(self)(**out)


@dataclass
class ActorOutput(TensorDataClass):
    action: torch.Tensor
    log_prob: Optional[torch.Tensor] = None
    squashed_mean: Optional[torch.Tensor] = None


@dataclass
class DocList(TensorDataClass):
    # (batch_size, num_candidates, num_document_features)
    float_features: torch.Tensor
    # (batch_size, num_candidates): whether the candidate is present (torch.bool), and a context dependent value (an
    # action probability, or the document's score from another model)
    mask: torch.Tensor = None
    value: torch.Tensor = None

    def __post_init__(self):
        assert len(self.float_features.shape) == 3, f"Unexpected shape: {self.float_features.shape}"
        if self.mask is None:
            self.mask = self.float_features.new_ones(self.float_features.shape[:2], dtype=torch.bool)
        if self.value is None:
            self.value = self.float_features.new_ones(self.float_features.shape[:2])

    @torch.no_grad()
    def select_slate(self, action: torch.Tensor):
        """:277-284.  A utility entry point: the SlateQ step gathers with rg_slate_gather and never builds this."""
        row_idx = torch.repeat_interleave(torch.arange(action.shape[0], device=action.device).unsqueeze(1), action.shape[1], dim=1)
        return DocList(self.float_features[row_idx, action], self.mask[row_idx, action], self.value[row_idx, action])

    def as_feature_data(self):
        _batch_size, _slate_size, feature_dim = self.float_features.shape
        return FeatureData(self.float_features.view(-1, feature_dim))


_FLOAT_FEATURES_USAGE = ("For sequence features, use `stacked_float_features`."
                         "For document features, use `candidate_doc_float_features`.")
_warned_3d = False  # the reference's no_dup_logger: the message once per process


@dataclass
class FeatureData(TensorDataClass):
    float_features: torch.Tensor
    # sparse / sequence members of the reference type are outside this hot path
    id_list_features: Optional[object] = None
    id_score_list_features: Optional[object] = None
    stacked_float_features: Optional[torch.Tensor] = None
    candidate_docs: Optional[object] = None
    time_since_first: Optional[torch.Tensor] = None

    def __post_init__(self):
        # run_post_init_validation (:294-309): 3-D (the world model's [seq_len, batch, dim]) passes with one warning
        ff = self.float_features
        if not isinstance(ff, torch.Tensor) or ff.ndim == 2:
            return
        if ff.ndim == 3:
            global _warned_3d
            if not _warned_3d:
                _warned_3d = True
                logging.getLogger(__name__).warning(f"`float_features` should be 2D.\n{_FLOAT_FEATURES_USAGE}")
            return
        raise ValueError(f"float_features should be 2D; got {ff.shape}.")

    def get_tiled_batch(self, num_tiles: int):
        """:349-364 — tiled[i * num_tiles:(i + 1) * num_tiles] == float_features[i].  A utility entry point: the
        parametric DQN step reads the tiled rows in place (rg_mlp_desc.x_tile / rg_tile_concat) and never builds them."""
        feat = self.float_features
        assert len(feat.shape) == 2, f"Need feat shape to be (batch_size, feature_dim), got {feat.shape}."
        return FeatureData(float_features=feat.repeat_interleave(repeats=num_tiles, dim=0))


@dataclass
class ExtraData(TensorDataClass):
    mdp_id: Optional[torch.Tensor] = None
    sequence_number: Optional[torch.Tensor] = None
    action_probability: Optional[torch.Tensor] = None
    max_num_actions: Optional[int] = None
    metrics: Optional[torch.Tensor] = None

    @classmethod
    def from_dict(cls, d):
        return cls(**{f.name: d.get(f.name, None) for f in dataclasses.fields(cls)})


@dataclass
class BaseInput(TensorDataClass):
    state: FeatureData
    next_state: FeatureData
    reward: torch.Tensor
    time_diff: Optional[torch.Tensor]
    step: Optional[torch.Tensor]
    not_terminal: torch.Tensor

    def __len__(self):
        assert self.state.float_features.ndim == 2
        return self.state.float_features.size()[0]

    def batch_size(self):
        return len(self)

    def as_dict_shallow(self):
        return {
            "state": self.state,
            "next_state": self.next_state,
            "reward": self.reward,
            "time_diff": self.time_diff,
            "step": self.step,
            "not_terminal": self.not_terminal,
        }

    @staticmethod
    def from_dict(batch):
        return BaseInput(
            state=FeatureData(float_features=batch["state_features"]),
            next_state=FeatureData(float_features=batch["next_state_features"]),
            reward=batch["reward"],
            time_diff=batch["time_diff"],
            step=batch.get("step", None),
            not_terminal=batch["not_terminal"],
        )


@dataclass
class DiscreteDqnInput(BaseInput):
    action: torch.Tensor
    next_action: torch.Tensor
    possible_actions_mask: torch.Tensor
    possible_next_actions_mask: torch.Tensor
    extras: ExtraData

    @classmethod
    def input_prototype(cls, action_dim=2, batch_size=10, state_dim=3):
        return cls(
            state=FeatureData(float_features=torch.randn(batch_size, state_dim)),
            next_state=FeatureData(float_features=torch.randn(batch_size, state_dim)),
            reward=torch.rand(batch_size, 1),
            time_diff=torch.ones(batch_size, 1),
            step=torch.ones(batch_size, 1),
            not_terminal=torch.ones(batch_size, 1),
            action=F.one_hot(torch.randint(high=action_dim, size=(batch_size,)), num_classes=action_dim),
            next_action=F.one_hot(torch.randint(high=action_dim, size=(batch_size,)), num_classes=action_dim),
            possible_actions_mask=torch.ones(batch_size, action_dim),
            possible_next_actions_mask=torch.ones(batch_size, action_dim),
            extras=ExtraData(action_probability=torch.ones(batch_size, 1)),
        )

    @classmethod
    def from_dict(cls, batch):
        base = BaseInput.from_dict(batch)
        return cls(
            action=batch["action"],
            next_action=batch["next_action"],
            possible_actions_mask=batch["possible_actions_mask"],
            possible_next_actions_mask=batch["possible_next_actions_mask"],
            extras=ExtraData.from_dict(batch),
            **base.as_dict_shallow(),
        )


@dataclass
class SlateQInput(BaseInput):
    """reward, reward_mask: (batch_size, slate_size); reward_mask says whether the item's reward could be observed"""

    action: torch.Tensor
    next_action: torch.Tensor
    reward_mask: torch.Tensor
    extras: Optional[ExtraData] = None

    @classmethod
    def from_dict(cls, d):
        return cls(
            state=FeatureData(
                float_features=d["state_features"],
                candidate_docs=DocList(float_features=d["candidate_features"], mask=d["item_mask"], value=d["item_probability"]),
            ),
            next_state=FeatureData(
                float_features=d["next_state_features"],
                candidate_docs=DocList(float_features=d["next_candidate_features"], mask=d["next_item_mask"],
                                       value=d["next_item_probability"]),
            ),
            action=d["action"],
            next_action=d["next_action"],
            reward=d["position_reward"],
            reward_mask=d["reward_mask"],
            time_diff=d["time_diff"],
            not_terminal=d["not_terminal"],
            step=None,
            extras=ExtraData.from_dict(d),
        )


@dataclass
class ParametricDqnInput(BaseInput):
    action: FeatureData
    next_action: FeatureData
    possible_actions: FeatureData
    possible_actions_mask: torch.Tensor
    possible_next_actions: FeatureData
    possible_next_actions_mask: torch.Tensor
    extras: Optional[ExtraData] = None
    weight: Optional[torch.Tensor] = None

    @classmethod
    def from_dict(cls, batch):
        return cls(
            state=FeatureData(float_features=batch["state_features"]),
            action=FeatureData(float_features=batch["action"]),
            next_state=FeatureData(float_features=batch["next_state_features"]),
            next_action=FeatureData(float_features=batch["next_action"]),
            possible_actions=FeatureData(float_features=batch["possible_actions"]),
            possible_actions_mask=batch["possible_actions_mask"],
            possible_next_actions=FeatureData(float_features=batch["possible_next_actions"]),
            possible_next_actions_mask=batch["possible_next_actions_mask"],
            reward=batch["reward"],
            not_terminal=batch["not_terminal"],
            time_diff=batch["time_diff"],
            step=batch["step"],
            extras=batch["extras"],
            weight=batch.get("weight", None),
        )


@dataclass
class PolicyNetworkInput(BaseInput):
    action: FeatureData
    next_action: FeatureData
    extras: Optional[ExtraData] = None

    @classmethod
    def from_dict(cls, batch):
        base = BaseInput.from_dict(batch)
        return cls(
            action=FeatureData(float_features=batch["action"]),
            next_action=FeatureData(float_features=batch["next_action"]),
            extras=batch.get("extras", None),
            **base.as_dict_shallow(),
        )


@dataclass
class PolicyGradientInput(TensorDataClass):
    """One trajectory: state [T, S], action [T, A] one-hot, reward [T], log_prob [T] of the logged action under the
    acting policy, possible_actions_mask [T, A] (optional).  next_state / not_terminal bootstrap truncated
    trajectories (the TD-error advantage of the reference's PPO); leave None for complete episodes."""

    state: FeatureData
    action: torch.Tensor
    reward: torch.Tensor
    log_prob: torch.Tensor
    possible_actions_mask: Optional[torch.Tensor] = None
    next_state: Optional[FeatureData] = None
    not_terminal: Optional[torch.Tensor] = None

    @classmethod
    def input_prototype(cls, action_dim=2, batch_size=10, state_dim=3):
        return cls(
            state=FeatureData(float_features=torch.randn(batch_size, state_dim)),
            action=F.one_hot(torch.randint(high=action_dim, size=(batch_size,)), num_classes=action_dim),
            reward=torch.rand(batch_size),
            log_prob=torch.log(torch.rand(batch_size)),
            possible_actions_mask=torch.ones(batch_size, action_dim),
        )

    @classmethod
    def from_dict(cls, d):
        next_observation = d.get("next_observation", None)
        return cls(
            state=FeatureData(float_features=d["observation"]),
            action=d["action"],
            reward=d["reward"],
            log_prob=d["log_prob"],
            possible_actions_mask=d.get("possible_actions_mask", None),
            next_state=FeatureData(float_features=next_observation) if next_observation is not None else None,
            not_terminal=d.get("not_terminal", None),
        )

    def __len__(self):
        assert self.action.ndim == 2
        return len(self.action)

    def batch_size(self):
        return len(self)


@dataclass
class CBInput(TensorDataClass):
    """A contextual-bandit batch: context_arm_features [B, A, d] (the features of every arm), action [B, 1] int64 (the
    chosen arm), reward / label [B, 1] (label is what the model is trained on; it defaults to a copy of reward), weight and
    importance_weight [B, 1] (their product is the row's effective weight), arm_presence [B, A]."""

    context_arm_features: torch.Tensor
    features_of_chosen_arm: Optional[torch.Tensor] = None
    chosen_arm_id: Optional[torch.Tensor] = None
    arm_presence: Optional[torch.Tensor] = None
    action: Optional[torch.Tensor] = None
    reward: Optional[torch.Tensor] = None
    label: Optional[torch.Tensor] = None
    rewards_all_arms: Optional[torch.Tensor] = None
    action_log_probability: Optional[torch.Tensor] = None
    weight: Optional[torch.Tensor] = None
    importance_weight: Optional[torch.Tensor] = None
    arms: Optional[torch.Tensor] = None
    mdp_id: Optional[torch.Tensor] = None

    def __post_init__(self):
        if self.label is None and self.reward is not None:
            self.label = self.reward.clone()

    @classmethod
    def input_prototype(cls, context_dim: int = 2, batch_size: int = 10, arm_features_dim: int = 3, num_arms: int = 4):
        return cls(context_arm_features=torch.randn(batch_size, num_arms, arm_features_dim))

    @classmethod
    def from_dict(cls, d):
        # (rewards_all_arms is not read from the dict: the reference's from_dict leaves it out too)
        optional = ("features_of_chosen_arm", "chosen_arm_id", "arm_presence", "action", "reward", "label",
                    "action_log_probability", "weight", "importance_weight", "arms", "mdp_id")
        return cls(context_arm_features=d["context_arm_features"], **{k: d.get(k, None) for k in optional})

    def __len__(self):
        return self.context_arm_features.shape[0]

    @property
    def device(self):
        return self.context_arm_features.device

    @property
    def effective_weight(self):
        weight = self.weight
        if weight is None:
            weight = torch.ones(len(self), 1, device=self.device, dtype=torch.float)
        if self.importance_weight is not None:
            assert self.importance_weight.shape == weight.shape
            weight = weight * self.importance_weight
        return weight


@dataclass
class MemoryNetworkInput(BaseInput):
    """:1017-1046 — the world model's batch: every tensor sequence first, [seq_len, batch, ...]"""

    action: FeatureData
    valid_step: Optional[torch.Tensor] = None  # [B, 1] int64 in 1 .. seq_len: read by the Seq2Reward trainers alone
    extras: ExtraData = field(default_factory=ExtraData)

    @classmethod
    def from_dict(cls, d):
        return cls(
            state=FeatureData(float_features=d["state"]),
            next_state=FeatureData(float_features=d["next_state"]),
            action=FeatureData(float_features=d["action"]),
            reward=d["reward"],
            time_diff=d["time_diff"],
            not_terminal=d["not_terminal"],
            step=d["step"],
            extras=ExtraData.from_dict(d),
        )

    def __len__(self):
        n = self.state.float_features.ndim
        if n == 2:
            return self.state.float_features.size()[0]
        if n == 3:
            return self.state.float_features.size()[1]
        raise NotImplementedError()


@dataclass
class MemoryNetworkOutput(TensorDataClass):
    """:1057-1066"""

    mus: torch.Tensor
    sigmas: torch.Tensor
    logpi: torch.Tensor
    reward: torch.Tensor
    not_terminal: torch.Tensor
    last_step_lstm_hidden: torch.Tensor
    last_step_lstm_cell: torch.Tensor
    all_steps_lstm_hidden: torch.Tensor


@dataclass
class Seq2RewardOutput(TensorDataClass):
    """:1069-1071"""

    acc_reward: torch.Tensor


@dataclass
class SyntheticRewardNetworkOutput(TensorDataClass):
    """:1098-1102 — the synthetic-reward nets' output: predicted_reward [B, 1], mask [B, seq_len], output [B, seq_len]"""

    predicted_reward: torch.Tensor
    mask: torch.Tensor
    output: torch.Tensor


@dataclass
class BanditRewardModelInput(TensorDataClass):
    """:977-995 — logged bandit data: state, the logged action [B, A] (one-hot), reward [B, 1] and, for the inverse
    propensity weighting, the logging policy's probability of that action [B, 1]"""

    state: FeatureData
    action: torch.Tensor
    reward: torch.Tensor
    action_prob: Optional[torch.Tensor] = None

    @classmethod
    def from_dict(cls, batch):
        return cls(
            state=FeatureData(float_features=batch["state_features"]),
            action=batch["action"],
            reward=batch["reward"],
            action_prob=batch.get("action_probability", None),
        )

    def batch_size(self):
        assert self.state.float_features.ndim == 2
        return self.state.float_features.size()[0]


def _rows_at(data: torch.Tensor, index_2d: torch.Tensor) -> torch.Tensor:
    """out[b, j] = data[b, index_2d[b, j]] for data [B, N, D] and index_2d [B, M] (the reference's torch_utils.gather)"""
    return data.gather(1, index_2d.unsqueeze(2).expand(-1, -1, data.shape[2]))


@dataclass
class PreprocessedRankingInput(TensorDataClass):
    """:453-685 — a ranking batch: the state [B, state_dim], the candidates src_seq [B, S, candidate_dim], the logged slate as
    indices (offset by 2: 0 is the padding symbol and 1 the decoder's start symbol) and as gathered feature rows, its logged
    propensity tgt_out_probs [B, 1] and the slate's reward [B, 1].  The feature members are FeatureData: bare tensors go
    through from_tensors (or from_input, which derives the index and mask members)."""

    state: FeatureData
    src_seq: FeatureData
    src_src_mask: Optional[torch.Tensor] = None
    tgt_in_seq: Optional[FeatureData] = None
    tgt_out_seq: Optional[FeatureData] = None
    tgt_tgt_mask: Optional[torch.Tensor] = None
    slate_reward: Optional[torch.Tensor] = None
    position_reward: Optional[torch.Tensor] = None
    src_in_idx: Optional[torch.Tensor] = None
    tgt_in_idx: Optional[torch.Tensor] = None
    tgt_out_idx: Optional[torch.Tensor] = None
    tgt_out_probs: Optional[torch.Tensor] = None
    # the ground-truth slate, where there is one
    optim_tgt_in_idx: Optional[torch.Tensor] = None
    optim_tgt_out_idx: Optional[torch.Tensor] = None
    optim_tgt_in_seq: Optional[FeatureData] = None
    optim_tgt_out_seq: Optional[FeatureData] = None
    extras: Optional[ExtraData] = field(default_factory=ExtraData)

    _FEATURE_MEMBERS = ("state", "src_seq", "tgt_in_seq", "tgt_out_seq", "optim_tgt_in_seq", "optim_tgt_out_seq")

    def __post_init__(self):
        if any(isinstance(getattr(self, n), torch.Tensor) for n in self._FEATURE_MEMBERS):
            raise ValueError("Use from_tensors() " + " ".join(str(type(getattr(self, n))) for n in self._FEATURE_MEMBERS) + " ")

    def batch_size(self) -> int:
        return self.state.float_features.size()[0]

    def __len__(self) -> int:
        return self.batch_size()

    @classmethod
    def from_input(cls, state, candidates, device, action=None, optimal_action=None, logged_propensities=None, slate_reward=None,
                   position_reward=None, extras=None):
        """the derived members from raw input: action / optimal_action [B, T] index the candidates from 0"""
        assert len(state.shape) == 2 and len(candidates.shape) == 3
        state, candidates = state.to(device), candidates.to(device)
        B, S, D = candidates.shape
        if action is not None:
            assert len(action.shape) == 2
            action = action.to(device)
        if logged_propensities is not None:
            assert len(logged_propensities.shape) == 2 and logged_propensities.shape[1] == 1
            logged_propensities = logged_propensities.to(device)
        if slate_reward is not None:
            assert len(slate_reward.shape) == 2 and slate_reward.shape[1] == 1
            slate_reward = slate_reward.to(device)
        if position_reward is not None:
            assert position_reward.shape == action.shape
            position_reward = position_reward.to(device)

        def target_members(a):
            """(tgt_in_idx, tgt_out_idx, tgt_in_seq, tgt_out_seq, tgt_tgt_mask) of a slate: the decoder's input is its output
            shifted by one step behind the start symbol, whose features are zeros"""
            if a is None:
                return None, None, None, None, None
            T = a.shape[1]
            out_idx = a + 2
            in_idx = torch.full((B, T), 1, device=device)  # DECODER_START_SYMBOL
            in_idx[:, 1:] = out_idx[:, :-1]
            out_seq = _rows_at(torch.cat((torch.zeros(B, 2, D, device=device), candidates), dim=1), out_idx)
            in_seq = torch.zeros(B, T, D, device=device)
            in_seq[:, 1:] = out_seq[:, :-1]
            mask = ~torch.triu(torch.ones(1, T, T, device=device, dtype=torch.bool), diagonal=1)  # subsequent_mask
            return in_idx, out_idx, in_seq, out_seq, mask

        tgt_in_idx, tgt_out_idx, tgt_in_seq, tgt_out_seq, tgt_tgt_mask = target_members(action)
        optim_in_idx, optim_out_idx, optim_in_seq, optim_out_seq, _ = target_members(optimal_action)
        return cls.from_tensors(
            state=state, src_seq=candidates, src_src_mask=torch.ones(B, S, S, device=device).type(torch.int8),
            tgt_in_seq=tgt_in_seq, tgt_out_seq=tgt_out_seq, tgt_tgt_mask=tgt_tgt_mask, slate_reward=slate_reward,
            position_reward=position_reward, src_in_idx=torch.arange(S, device=device).repeat(B, 1) + 2, tgt_in_idx=tgt_in_idx,
            tgt_out_idx=tgt_out_idx, tgt_out_probs=logged_propensities, optim_tgt_in_idx=optim_in_idx,
            optim_tgt_out_idx=optim_out_idx, optim_tgt_in_seq=optim_in_seq, optim_tgt_out_seq=optim_out_seq, extras=extras)

    @classmethod
    def from_tensors(cls, state, src_seq, src_src_mask=None, tgt_in_seq=None, tgt_out_seq=None, tgt_tgt_mask=None,
                     slate_reward=None, position_reward=None, src_in_idx=None, tgt_in_idx=None, tgt_out_idx=None, tgt_out_probs=None,
                     optim_tgt_in_idx=None, optim_tgt_out_idx=None, optim_tgt_in_seq=None, optim_tgt_out_seq=None, extras=None,
                     **kwargs):
        given = dict(src_src_mask=src_src_mask, tgt_in_seq=tgt_in_seq, tgt_out_seq=tgt_out_seq, tgt_tgt_mask=tgt_tgt_mask,
                     slate_reward=slate_reward, position_reward=position_reward, src_in_idx=src_in_idx, tgt_in_idx=tgt_in_idx,
                     tgt_out_idx=tgt_out_idx, tgt_out_probs=tgt_out_probs, optim_tgt_in_idx=optim_tgt_in_idx,
                     optim_tgt_out_idx=optim_tgt_out_idx, optim_tgt_in_seq=optim_tgt_in_seq, optim_tgt_out_seq=optim_tgt_out_seq)
        assert isinstance(state, torch.Tensor) and isinstance(src_seq, torch.Tensor)
        for name, t in given.items():
            assert t is None or isinstance(t, torch.Tensor), name
        assert extras is None or isinstance(extras, ExtraData)
        wrap = lambda t: FeatureData(float_features=t) if t is not None else None  # noqa: E731
        for name in ("tgt_in_seq", "tgt_out_seq", "optim_tgt_in_seq", "optim_tgt_out_seq"):
            given[name] = wrap(given[name])
        return cls(state=FeatureData(float_features=state), src_seq=FeatureData(float_features=src_seq), extras=extras, **given)


@dataclass
class RankingOutput(TensorDataClass):
    """:1091-1124 — what a ranking net returns: the ranked slate's indices [B, T] (offset by 2), its per-step probabilities
    [B, T, S + 2] and per-sequence probability [B, 1] (rank mode); the logged slate's log-probability [B, 1]; the encoder's
    scores [B, T]"""

    ranked_tgt_out_idx: Optional[torch.Tensor] = None
    ranked_per_symbol_probs: Optional[torch.Tensor] = None
    ranked_per_seq_probs: Optional[torch.Tensor] = None
    log_probs: Optional[torch.Tensor] = None
    encoder_scores: Optional[torch.Tensor] = None


# ---- the reference's own classes, when it is importable (see the module docstring) ---------------------------
def _reference_types():
    import importlib.util
    import os

    if os.environ.get("REAGENT_AMD_OWN_TYPES") == "1":
        return None
    try:
        if importlib.util.find_spec("reagent") is None or importlib.util.find_spec("reagent.core.types") is None:
            return None
        import reagent.core.types as ref

        return ref
    except Exception:  # a partial installation (missing dependency of the reference): keep the restatements
        return None


USING_REFERENCE_TYPES = False
_ref = _reference_types()
if _ref is not None:
    for _name in ("TensorDataClass", "ActorOutput", "DocList", "FeatureData", "ExtraData", "BaseInput", "DiscreteDqnInput",
                  "SlateQInput", "ParametricDqnInput", "PolicyNetworkInput", "PolicyGradientInput", "CBInput", "MemoryNetworkInput",
                  "MemoryNetworkOutput", "Seq2RewardOutput", "SyntheticRewardNetworkOutput", "BanditRewardModelInput",
                  "PreprocessedRankingInput", "RankingOutput"):
        globals()[_name] = getattr(_ref, _name)
    USING_REFERENCE_TYPES = True
del _ref
