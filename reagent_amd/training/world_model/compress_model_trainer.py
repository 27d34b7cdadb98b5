"""CompressModelTrainer with the surface of reagent/training/world_model/compress_model_trainer.py:22-124: fits an MLP on the
first step's states to what Seq2Reward's planning gives (get_Q: the prefix-tree rollout of seq2reward_trainer.py), so that
acting needs one small forward and no planning.

  forward : the FloatFeatureFullyConnected's FC stack in fp32, saving
  target  : get_Q — rg_lstm_fanout_step per depth and layer, rg_seq2reward_plan_max
  loss    : F.mse_loss on [B, A] and the share of rows whose arg-max agrees with the target's, in torch (the shape is tiny)
  backward: the stack's backward from d loss / d output = 2 (output - target) / (B A), rg_adam_step

The generator path and train_step_native give the same bits.  Losses move to the host only when a reporter is set.
"""
import logging

import torch
import torch.nn.functional as F

from ... import _lib as L
from ...core import types as rlt
from ...core.parameters import Seq2RewardTrainerParameters
from ...core.types import FeatureData
from ...models.fully_connected_network import FloatFeatureFullyConnected
from ...models.seq2reward_model import Seq2RewardNetwork
from ...optimizer import FusedAdam
from ..plumbing import NativeStepMixin, native_step
from ..reagent_lightning_module import ReAgentLightningModule, _NoOpReporter
from ..utils import gen_permutations
from .seq2reward_trainer import best_action_shares, check_planning_limits, get_Q, require_seq2reward_network

logger = logging.getLogger(__name__)


class CompressModelTrainer(NativeStepMixin, ReAgentLightningModule):
    """Trainer for fitting Seq2Reward planning outcomes to a neural network-based policy"""

    _graph_capture_refusal = ("the world-model step is not captured into a HIP graph: its buffers are allocated per step; "
                              "run it eagerly")

    def __init__(
        self,
        compress_model_network: FloatFeatureFullyConnected,
        seq2reward_network: Seq2RewardNetwork,
        params: Seq2RewardTrainerParameters,
    ):
        super().__init__()
        require_seq2reward_network(seq2reward_network, "CompressModelTrainer")
        if not hasattr(compress_model_network, "fc") or not hasattr(compress_model_network.fc, "stack"):
            raise NotImplementedError("CompressModelTrainer: compress_model_network must be a reagent_amd "
                                      f"FloatFeatureFullyConnected (got {type(compress_model_network).__name__})")
        check_planning_limits(len(params.action_names), params.multi_steps, "CompressModelTrainer")
        self.compress_model_network = compress_model_network
        self.compress_model_network.fc.precision = L.PREC_F32
        self.seq2reward_network = seq2reward_network
        self.params = params

        # permutations used to do planning
        self.all_permut = gen_permutations(params.multi_steps, len(self.params.action_names))

    def enable_data_parallel(self, process_group=None):
        raise NotImplementedError("CompressModelTrainer has no data-parallel path (world > 1 is not supported)")

    def configure_optimizers(self):
        return [{"optimizer": FusedAdam(self.compress_model_network.parameters(),
                                        lr=self.params.compress_model_learning_rate)}]

    @staticmethod
    def extract_state_first_step(batch):
        return FeatureData(batch.state.float_features[0])

    def _forward(self, batch: rlt.MemoryNetworkInput):
        """-> (mse [1] and accuracy on the device, the trainable net, its backward)"""
        if getattr(self, "_graph_mode", False):
            raise NotImplementedError(self._graph_capture_refusal)
        e = self._trainable(self.compress_model_network)
        dev = e.params[0].device
        state = self._f32c(self.extract_state_first_step(batch).float_features.to(dev))
        L.require_cuda(state, "batch.state")
        B, A = state.shape[0], e.stack.dims[-1]
        out = torch.empty(B, A, dtype=torch.float32, device=dev)
        e.stack.stage_weights(need_transposed=True)
        xc, xt = e.stack.stage_input(state, need_transposed=True)
        e.stack.forward(xc, out, save=True)
        target = get_Q(self.seq2reward_network, state, self.all_permut)
        assert out.size() == target.size(), f"{out.size()}!={target.size()}"
        with torch.no_grad():
            mse = F.mse_loss(out, target)
            dout = (out - target) * (2.0 / (B * A))
            accuracy = torch.mean((torch.max(target, dim=1).indices == torch.max(out, dim=1).indices).float())
        return mse.view(1), accuracy, e, lambda grad_out=None: e.backward(dout, xt, grad_out)

    def get_loss(self, batch: rlt.MemoryNetworkInput):
        """:99-119 — (mse of the network's output against get_Q's, accuracy of its arg-max against get_Q's).  With autograd
        enabled, backward() of the mse runs the stack's backward and publishes the network's gradients."""
        mse, accuracy, e, backward = self._forward(batch)
        if not torch.is_grad_enabled():
            return mse.view(()), accuracy
        return e.loss(backward, mse), accuracy

    def train_step_gen(self, training_batch: rlt.MemoryNetworkInput, batch_idx: int):
        loss, accuracy = self.get_loss(training_batch)
        if not isinstance(self.reporter, _NoOpReporter):  # (nobody listens: no host synchronisation)
            mse, accuracy = loss.item(), accuracy.item()
            logger.info(f"Seq2Reward Compress trainer MSE/Accuracy: {mse}, {accuracy}")
            self.reporter.log(mse_loss=mse, accuracy=accuracy)
        yield loss

    @torch.no_grad()
    @native_step
    def train_step_native(self, training_batch: rlt.MemoryNetworkInput):
        """the step with no autograd graph, generator or host synchronisation -> mse and accuracy on the device"""
        mse, accuracy, e, backward = self._forward(training_batch)
        self._native_segment(e, backward, self.native_optimizers()[0])
        self.all_batches_processed += 1
        return dict(mse_loss=mse.view(()), accuracy=accuracy)

    @torch.no_grad()
    def validation_step(self, batch: rlt.MemoryNetworkInput, batch_idx: int):
        """:69-97 — (mse, the network's mean Q per action, the share of rows whose best action is each action, accuracy)"""
        mse, acc = self.get_loss(batch)
        mse, acc = mse.item(), acc.item()
        dev = next(self.compress_model_network.parameters()).device
        state = self.extract_state_first_step(batch).float_features.to(dev)
        q = self.compress_model_network(FeatureData(state)).cpu()  # [B, A]
        q_values, action_distribution = q.mean(0).tolist(), best_action_shares(q, len(self.params.action_names))
        self.reporter.log(eval_mse_loss=mse, eval_accuracy=acc, eval_q_values=[q_values],
                          eval_action_distribution=[action_distribution])
        return (mse, q_values, action_distribution, acc)

    def warm_start_components(self):
        return []  # (none yet, as in the reference)
