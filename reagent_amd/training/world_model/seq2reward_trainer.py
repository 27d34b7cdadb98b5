"""Seq2RewardTrainer, get_Q and get_step_prediction with the surface of reagent/training/world_model/seq2reward_trainer.py:20-271,
executed on the HIP kernels:

  mse segment   : Seq2RewardNetwork._run (rg_fc_forward, rg_lstm_forward per layer), rg_seq2reward_head (lstm_linear at each
                  row's valid step, the discounted reward target, the loss, d loss / d h_all and lstm_linear's gradients),
                  Seq2RewardNetwork.backward, rg_adam_step over the network's slab
  step segment  : the step predictor's FC stack in fp32, rg_step_ce_head (cross-entropy against valid_step - 1 and its
                  gradient), the stack's backward, rg_adam_step
  planning      : get_Q — the reference enumerates all A^multi_steps action sequences and runs the LSTM over B * A^multi_steps
                  rows for multi_steps steps; sequences in lexical order share prefixes, so here the rollout is a tree, a
                  level at a time (Seq2RewardNetwork.tree_rollout_max), and nothing of shape [multi_steps, B * P, .] exists

The generator path (training_step, backward, optimizer step, twice) and train_step_native run the same launches on the same
buffers: the same bits.  The reference moves every loss to the host on every step; here that happens only when a reporter is
set (the logged keys and values are the reference's).
"""
import logging
import types

import torch

from ... import _lib as L
from ... import ops
from ...core import types as rlt
from ...core.parameters import Seq2RewardTrainerParameters
from ...engine import ensure_slab
from ...models.fully_connected_network import FullyConnectedNetwork
from ...models.seq2reward_model import Seq2RewardNetwork
from ...optimizer import FusedAdam
from ..plumbing import NativeStepMixin, SegmentLoss, held_gradients, native_step, publish_gradients
from ..reagent_lightning_module import ReAgentLightningModule, _NoOpReporter
from ..utils import gen_permutations

logger = logging.getLogger(__name__)

MAX_ACTIONS = 32  # len(action_names)
MAX_SEQUENCES = 1 << 20  # len(action_names) ** multi_steps
# get_Q's workspace cap in bytes: the batch is planned in chunks of rows whose (h, c) levels, upper-layer input projections and
# embedding stay under it (rows are independent: the chunks give the same bits).  512 MiB keeps a chunk's two levels inside
# what the memory-side cache and L2 can hold a useful part of, and is far below what the device has.
GET_Q_WORKSPACE_BYTES = 512 << 20


def require_seq2reward_network(net, who: str):
    if not isinstance(net, Seq2RewardNetwork):
        raise NotImplementedError(f"{who}: seq2reward_network must be a reagent_amd Seq2RewardNetwork "
                                  f"(got {type(net).__name__}): planning and the step run on its kernels")


def check_planning_limits(num_action: int, multi_steps: int, who: str):
    if not 1 <= num_action <= MAX_ACTIONS:
        raise NotImplementedError(f"{who}: {num_action} actions are not supported (1 .. {MAX_ACTIONS})")
    if multi_steps < 1 or num_action ** multi_steps > MAX_SEQUENCES:
        raise NotImplementedError(f"{who}: {num_action} ** {multi_steps} action sequences are not supported "
                                  f"(multi_steps at least 1, at most 2^20 sequences)")
    if multi_steps > L.STEP_CE_MAX_CLASSES:
        raise NotImplementedError(f"{who}: multi_steps {multi_steps} is not supported (1 .. {L.STEP_CE_MAX_CLASSES})")


def _require_lexical(all_permut: torch.Tensor):
    """all_permut must be gen_permutations' enumeration: the tree rollout never reads it, it IS that order.  The shape is
    checked on every call, the content once per tensor object."""
    if all_permut.ndim != 3:
        raise NotImplementedError(f"get_Q: all_permut of shape {tuple(all_permut.shape)} is not gen_permutations' "
                                  "[seq_len, num_action ** seq_len, num_action]")
    steps, num_permut, num_action = all_permut.shape
    check_planning_limits(num_action, steps, "get_Q")
    if num_permut != num_action ** steps:
        raise NotImplementedError(f"get_Q: all_permut of shape {tuple(all_permut.shape)} is not gen_permutations' "
                                  "[seq_len, num_action ** seq_len, num_action]")
    if getattr(all_permut, "_rg_lexical", None) != all_permut._version:
        if not torch.equal(all_permut.detach().cpu().float(), gen_permutations(steps, num_action)):
            raise NotImplementedError("get_Q: all_permut is not gen_permutations' lexical one-hot enumeration; other "
                                      "sequence sets have no prefix tree to plan on")
        all_permut._rg_lexical = all_permut._version
    return steps, num_action


def best_action_shares(q_values: torch.Tensor, num_action: int):
    """the share of rows of q_values [B, A] whose arg-max is each action, as a list (validation_step's action distribution)"""
    counts = torch.bincount(torch.argmax(q_values, dim=1), minlength=num_action)
    return (counts.float() / counts.sum()).tolist()


@torch.no_grad()
def get_step_prediction(step_predict_network: FullyConnectedNetwork, training_batch: rlt.MemoryNetworkInput):
    """:20-27 — softmax of the step predictor on the first step's states [B, multi_steps] (rg_step_ce_head's softmax)"""
    first_step_state = training_batch.state.float_features[0]
    pred_step = step_predict_network(first_step_state)
    pred_step = pred_step if pred_step.is_contiguous() else pred_step.contiguous()
    step_probability = torch.empty_like(pred_step)
    ops.step_ce_head(pred_step, None, softmax=step_probability)
    return step_probability


@torch.no_grad()
def get_Q(seq2reward_network: Seq2RewardNetwork, cur_state: torch.Tensor, all_permut: torch.Tensor) -> torch.Tensor:
    """:30-64 — max over the action sequences that start with each action of the predicted accumulated reward, [B, A].
    cur_state: [B, state_dim]; all_permut: gen_permutations(multi_steps, A), [multi_steps, A ** multi_steps, A]."""
    require_seq2reward_network(seq2reward_network, "get_Q")
    steps, num_action = _require_lexical(all_permut)
    net = seq2reward_network
    assert cur_state.ndim == 2 and cur_state.shape[1] == net.state_dim and num_action == net.action_dim, \
        (cur_state.shape, all_permut.shape, net.state_dim, net.action_dim)
    cur_state = cur_state.to(net.lstm_linear.weight.device)
    L.require_cuda(cur_state, "cur_state")
    cur_state = NativeStepMixin._f32c(cur_state)
    batch_size = cur_state.shape[0]
    chunk = max(1, GET_Q_WORKSPACE_BYTES // (4 * net.tree_rollout_floats_per_row(steps, num_action)))
    chunk = min(chunk, ((1 << 29) - 1) // num_action ** steps)  # (a level's rows go through the kernels as an int)
    if chunk >= batch_size:
        return net.tree_rollout_max(cur_state, steps, num_action)
    return torch.cat([net.tree_rollout_max(cur_state[i:i + chunk], steps, num_action) for i in range(0, batch_size, chunk)])


class Seq2RewardTrainer(NativeStepMixin, ReAgentLightningModule):
    """Trainer for Seq2Reward"""

    _graph_capture_refusal = ("the world-model step is not captured into a HIP graph: its buffers are allocated per step; "
                              "run it eagerly")

    def __init__(self, seq2reward_network: Seq2RewardNetwork, params: Seq2RewardTrainerParameters):
        super().__init__()
        require_seq2reward_network(seq2reward_network, "Seq2RewardTrainer")
        check_planning_limits(len(params.action_names), params.multi_steps, "Seq2RewardTrainer")
        self.seq2reward_network = seq2reward_network
        self.params = params

        # Turning off Q value output during training:
        self.view_q_value = params.view_q_value
        # permutations used to do planning
        self.all_permut = gen_permutations(params.multi_steps, len(self.params.action_names))

        # Predict how many steps are remaining from the current step
        self.step_predict_network = FullyConnectedNetwork(
            [
                self.seq2reward_network.state_dim,
                self.params.step_predict_net_size,
                self.params.step_predict_net_size,
                self.params.multi_steps,
            ],
            ["relu", "relu", "linear"],
            use_layer_norm=False,
        )
        self.step_predict_network.precision = L.PREC_F32
        self._gamma_pows = {}

    def enable_data_parallel(self, process_group=None):
        raise NotImplementedError("Seq2RewardTrainer has no data-parallel path (world > 1 is not supported)")

    def configure_optimizers(self):
        return [
            {"optimizer": FusedAdam(self.seq2reward_network.parameters(), lr=self.params.learning_rate)},
            {"optimizer": FusedAdam(self.step_predict_network.parameters(), lr=self.params.learning_rate)},
        ]

    # ---- the mse segment ---------------------------------------------------------------------------------------------
    def _gamma_pow(self, seq_len, dev):
        """fp32(gamma ** i), i < seq_len, built on the host as the reference builds its mask (:226-233)"""
        key = (seq_len, str(dev))
        if key not in self._gamma_pows:
            gamma = self.params.gamma
            self._gamma_pows[key] = torch.Tensor([gamma**i for i in range(seq_len)]).to(dev)
        return self._gamma_pows[key]

    def _refuse_graph(self):
        if getattr(self, "_graph_mode", False):
            raise NotImplementedError(self._graph_capture_refusal)

    def _mse_forward(self, training_batch: rlt.MemoryNetworkInput, save: bool):
        """one pass and the head -> (loss [1] on the device, the tape, (d loss / d h_all, d lstm_linear.weight, d bias))"""
        assert isinstance(training_batch, rlt.MemoryNetworkInput)
        self._refuse_graph()
        net = self.seq2reward_network
        tape = net._run(training_batch.state.float_features, training_batch.action.float_features, save=save)
        T, B, H = tape["T"], tape["B"], net.num_hiddens
        dev = tape["emb"].device
        valid_step = net._steps(training_batch.valid_step, B, dev)
        reward = self._f32c(training_batch.reward.to(dev))
        assert reward.shape == (T, B), (reward.shape, T, B)
        f = dict(dtype=torch.float32, device=dev)
        acc, loss = torch.empty(B, **f), torch.empty(1, **f)
        dh_all, dw, db = torch.empty(T, B, H, **f), torch.empty(H, **f), torch.empty(1, **f)
        partials = torch.empty((H + 2) * ops.seq2reward_head_partials(B), dtype=torch.float64, device=dev)
        w, b = net._head_params()
        ops.seq2reward_head(tape["h"][-1], valid_step, reward, self._gamma_pow(T, dev), w, b, acc, dh_all, dw, db, partials, loss)
        return loss, tape, (dh_all, dw, db)

    def _mse_backward(self, tape, grads, grad_out=None):
        net = self.seq2reward_network
        params = list(net.parameters())
        slab = ensure_slab(params)
        held = held_gradients(slab, params)
        if grad_out is not None:
            grads = tuple(g * grad_out for g in grads)
        net.backward(tape, *grads)
        publish_gradients(slab, params, held)

    def get_mse_loss(self, training_batch: rlt.MemoryNetworkInput):
        """:201-245 — MSE(predicted accumulated reward at each row's valid step, the discounted sum of its rewards up to
        that step).  With autograd enabled, backward() of the loss runs the kernels' backward and publishes the network's
        gradients."""
        save = torch.is_grad_enabled()
        loss, tape, grads = self._mse_forward(training_batch, save)
        if not save:
            return loss.view(())
        return SegmentLoss.apply(lambda g: self._mse_backward(tape, grads, g), loss, *self.seq2reward_network.parameters())

    # ---- the step segment --------------------------------------------------------------------------------------------
    def _step_forward(self, training_batch: rlt.MemoryNetworkInput):
        """the step predictor's saving forward and the cross-entropy head -> (loss [1], the trainable net, backward)"""
        self._refuse_graph()
        net = self.step_predict_network
        e = self._trainable(types.SimpleNamespace(fc=net, parameters=net.parameters))
        dev = net.linears()[0].weight.device
        first_step_state = self._f32c(training_batch.state.float_features[0].to(dev))
        L.require_cuda(first_step_state, "training_batch.state")
        B, K = first_step_state.shape[0], self.params.multi_steps
        valid_step = Seq2RewardNetwork._steps(training_batch.valid_step, B, dev)
        f = dict(dtype=torch.float32, device=dev)
        logits, dlogits, loss = torch.empty(B, K, **f), torch.empty(B, K, **f), torch.empty(1, **f)
        e.stack.stage_weights(need_transposed=True)
        xc, xt = e.stack.stage_input(first_step_state, need_transposed=True)
        e.stack.forward(xc, logits, save=True)
        partials = torch.empty(ops.step_ce_head_partials(B), dtype=torch.float64, device=dev)
        # step loss's target is zero-based indexed: the head subtracts 1 from valid_step
        ops.step_ce_head(logits, valid_step, dlogits, None, partials, loss)
        return loss, e, lambda grad_out=None: e.backward(dlogits, xt, grad_out)

    def get_step_entropy_loss(self, training_batch: rlt.MemoryNetworkInput):
        """:247-267 — cross-entropy of the step predictor on the first step's states against valid_step - 1"""
        loss, e, backward = self._step_forward(training_batch)
        if not torch.is_grad_enabled():
            return loss.view(())
        return e.loss(backward, loss)

    # ---- the steps ---------------------------------------------------------------------------------------------------
    def _listening(self):
        return not isinstance(self.reporter, _NoOpReporter)

    def train_step_gen(self, training_batch: rlt.MemoryNetworkInput, batch_idx: int):
        mse_loss = self.get_mse_loss(training_batch)
        yield mse_loss

        step_entropy_loss = self.get_step_entropy_loss(training_batch)
        if self._listening():  # (nobody listens: no host synchronisation, no planning for the log)
            mse, step_entropy = mse_loss.item(), step_entropy_loss.item()
            q_values = [0] * len(self.params.action_names)
            if self.view_q_value:  # (planned at the network's weights after the mse segment's step, as in the reference)
                q_values = get_Q(self.seq2reward_network, training_batch.state.float_features[0], self.all_permut).mean(0).tolist()
            step_probability = get_step_prediction(self.step_predict_network, training_batch).mean(dim=0).tolist()
            logger.info(f"Seq2Reward trainer output: mse_loss={mse}, step_entropy_loss={step_entropy}, q_values={q_values}, "
                        f"step_probability={step_probability}")
            self.reporter.log(mse_loss=mse, step_entropy_loss=step_entropy, q_values=[q_values])

        yield step_entropy_loss

    @torch.no_grad()
    @native_step
    def train_step_native(self, training_batch: rlt.MemoryNetworkInput):
        """both segments with no autograd graph, generator or host synchronisation -> the two losses on the device"""
        opts = self.native_optimizers()
        mse_loss, tape, grads = self._mse_forward(training_batch, save=True)
        for p in self.seq2reward_network.parameters():
            p.grad = None
        self._mse_backward(tape, grads)
        opts[0].step()
        step_entropy_loss, e, backward = self._step_forward(training_batch)
        self._native_segment(e, backward, opts[1])
        self.all_batches_processed += 1
        return dict(mse_loss=mse_loss.view(()), step_entropy_loss=step_entropy_loss.view(()))

    @torch.no_grad()
    def validation_step(self, batch: rlt.MemoryNetworkInput, batch_idx: int):
        """:163-199 — (mse loss, step-entropy loss, mean planned Q per action, the share of rows whose best first action is
        each action), all on the host"""
        mse = self.get_mse_loss(batch).item()
        step_entropy = self.get_step_entropy_loss(batch).item()
        q = get_Q(self.seq2reward_network, batch.state.float_features[0], self.all_permut).cpu()  # [B, A]
        q_values, action_distribution = q.mean(0).tolist(), best_action_shares(q, len(self.params.action_names))
        self.reporter.log(eval_mse_loss=mse, eval_step_entropy_loss=step_entropy, eval_q_values=[q_values],
                          eval_action_distribution=[action_distribution])
        return (mse, step_entropy, q_values, action_distribution)

    def warm_start_components(self):
        components = ["seq2reward_network"]
        return components
