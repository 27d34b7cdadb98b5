"""MDNRNNTrainer with the constructor / generator surface of reagent/training/world_model/mdnrnn_trainer.py:20-177, executed
on the HIP kernels:

  forward : MDNRNN._run — per layer rg_fc_forward (x W_ih^T + b_ih, all steps) and rg_lstm_forward, then gmm_linear
  head    : rg_mdn_head — the three weighted losses, their sum and d loss / d gmm_linear's output in two launches
  backward: MDNRNN.backward — rg_fc_wgrad / rg_fc_dgrad for gmm_linear, per layer rg_lstm_backward and the weight gradients
  step    : rg_adam_step over the parameters' flat slab (optimizer.FusedAdam at params.learning_rate)

Torch contributes views and torch.cat.  The generator path (training_step, backward, optimizer step) and train_step_native
run the same launches on the same buffers: the same bits.
"""
from typing import Optional

import torch

from ... import ops
from ...core import types as rlt
from ...core.parameters import MDNRNNTrainerParameters
from ...engine import ensure_slab
from ...models.world_model import MemoryNetwork
from ...optimizer import FusedAdam
from ..plumbing import SegmentLoss, held_gradients, publish_gradients
from ..reagent_lightning_module import ReAgentLightningModule, _NoOpReporter

LOSS_NAMES = ("gmm", "bce", "mse", "loss")


class MDNRNNTrainer(ReAgentLightningModule):
    """Trainer for MDN-RNN"""

    _graph_capture_refusal = ("the world-model step is not captured into a HIP graph: its buffers are allocated per step; "
                              "run it eagerly")

    def __init__(self, memory_network: MemoryNetwork, params: MDNRNNTrainerParameters, cum_loss_hist: int = 100):
        super().__init__()
        if not hasattr(memory_network, "mdnrnn") or not hasattr(memory_network.mdnrnn, "_run"):
            raise NotImplementedError(f"MDNRNNTrainer: memory_network must be a reagent_amd MemoryNetwork "
                                      f"(got {type(memory_network).__name__}): the step runs on its MDNRNN's kernels")
        self.memory_network = memory_network
        self.params = params
        self._native_opt = None

    def enable_data_parallel(self, process_group=None):
        raise NotImplementedError("MDNRNNTrainer has no data-parallel path (world > 1 is not supported)")

    def configure_optimizers(self):
        return [FusedAdam(self.memory_network.mdnrnn.parameters(), lr=self.params.learning_rate)]

    # ---- the step's pieces -------------------------------------------------------------------------------------------
    def _forward(self, training_batch: rlt.MemoryNetworkInput, state_dim, save: bool):
        """one pass and the head -> (losses [4] = gmm, bce, mse, loss on the device, the tape, d loss / d gmm_outs)"""
        assert isinstance(training_batch, rlt.MemoryNetworkInput)
        if getattr(self, "_graph_mode", False):
            raise NotImplementedError(self._graph_capture_refusal)
        net = self.memory_network.mdnrnn
        tape = net._run(training_batch.action.float_features, training_batch.state.float_features, None, save=save)
        T, B, S, G = tape["T"], tape["B"], net.state_dim, net.num_gaussians
        if state_dim is not None and state_dim != S:
            raise NotImplementedError(f"MDNRNNTrainer.get_loss: state_dim={state_dim} is not the network's {S}; the gmm term "
                                      "is divided by the network's state_dim + 2 or not at all")
        z, N = tape["z"], T * B
        dev = z.device

        def rows(t, width=None):
            t = t.to(dev)
            t = t if t.dtype == torch.float32 else t.float()
            t = t if t.is_contiguous() else t.contiguous()
            return t.view(N) if width is None else t.view(N, width)

        p = self.params
        dz = torch.empty_like(z)
        losses = torch.empty(4, dtype=torch.float32, device=dev)
        partials = torch.empty(3 * ops.mdn_head_partials(N), dtype=torch.float64, device=dev)
        ops.mdn_head(z, rows(training_batch.next_state.float_features, S), rows(training_batch.reward),
                     rows(training_batch.not_terminal), G,
                     (p.next_state_loss_weight, p.not_terminal_loss_weight, p.reward_loss_weight), state_dim is not None,
                     (T - 1) * B if p.fit_only_one_next_step else 0, dz, partials, losses)
        return losses, tape, dz

    def _backward(self, tape, dz, grad_out=None):
        net = self.memory_network.mdnrnn
        params = list(net.parameters())
        slab = ensure_slab(params)
        held = held_gradients(slab, params)
        net.backward(tape, dz if grad_out is None else dz * grad_out)
        publish_gradients(slab, params, held)

    def get_loss(self, training_batch: rlt.MemoryNetworkInput, state_dim: Optional[int] = None):
        """:112-177 — {"gmm", "bce", "mse", "loss"}: GMMLoss(next_state) * weight (/ (state_dim + 2) inside "loss" when
        state_dim is given) + BCE(not_terminal) * weight + MSE(reward) * weight, each a mean over sequence and batch (over
        the last step with fit_only_one_next_step).  With autograd enabled, backward() of "loss" runs the kernels' backward
        and publishes the parameters' gradients."""
        save = torch.is_grad_enabled()
        losses, tape, dz = self._forward(training_batch, state_dim, save)
        out = {k: losses[i] for i, k in enumerate(LOSS_NAMES)}
        if save:
            out["loss"] = SegmentLoss.apply(lambda g: self._backward(tape, dz, g), losses[3:4],
                                            *self.memory_network.mdnrnn.parameters())
        return out

    def _report(self, losses, prefix=""):
        if isinstance(self.reporter, _NoOpReporter):  # (nobody listens: no host synchronisation)
            return
        detached = {k: v.detach().cpu().item() for k, v in losses.items()}
        self.reporter.log(**{prefix + k: detached[k] for k in ("loss", "gmm", "bce", "mse")})

    def train_step_gen(self, training_batch: rlt.MemoryNetworkInput, batch_idx: int):
        (seq_len, batch_size, state_dim) = training_batch.state.float_features.shape
        losses = self.get_loss(training_batch, state_dim)
        self._report(losses)
        yield losses["loss"]

    @torch.no_grad()
    def train_step_native(self, training_batch: rlt.MemoryNetworkInput):
        """the whole step with no autograd graph, generator or host synchronisation -> the four losses on the device"""
        if self._native_opt is None:
            self._native_opt = self.configure_optimizers()[0]
        (seq_len, batch_size, state_dim) = training_batch.state.float_features.shape
        losses, tape, dz = self._forward(training_batch, state_dim, save=True)
        for p in self.memory_network.mdnrnn.parameters():
            p.grad = None
        self._backward(tape, dz)
        self._native_opt.step()
        self.all_batches_processed += 1
        return {k: losses[i] for i, k in enumerate(LOSS_NAMES)}

    @torch.no_grad()
    def _eval_step(self, training_batch, prefix):
        (seq_len, batch_size, state_dim) = training_batch.state.float_features.shape
        losses = self.get_loss(training_batch, state_dim)  # (no autograd: nothing is saved)
        self._report(losses, prefix)
        loss = losses["loss"]
        self.log("td_loss", loss, prog_bar=True, batch_size=training_batch.batch_size())
        return loss

    def validation_step(self, training_batch: rlt.MemoryNetworkInput, batch_idx: int):
        return self._eval_step(training_batch, "eval_")

    def test_step(self, training_batch: rlt.MemoryNetworkInput, batch_idx: int):
        return self._eval_step(training_batch, "test_")
