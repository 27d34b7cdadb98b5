"""FeatureImportancePerturbation with the surface of
reagent/evaluation/feature_importance/feature_importance_perturbation.py (fields, compute_feature_importance, the result's two
columns), and a native sweep on reagent_amd/csrc/feature_importance.hip for the discrete DQN.

With a user ``pred_fn`` / ``perturb_fn`` the method runs through those two callables (``_generic``), with the reference's
behaviour: per feature a private copy of the batch, one disturbed column, the whole model again; the same order of random
draws and the same fp32 means.

The native sweep is taken when ``model`` is a ``DiscreteDqnWithPreprocessor`` over a plain ``FullyConnectedDQN`` (Linear ->
activation layers in PREC_F32: no batch norm, layer norm, dropout, atoms or dueling head; anything else is refused by name),
``pred_fn`` is one of the sentinels

    "max_q"          the row's largest Q-value
    "logged_action"  sum_a action[b, a] * q[b, a], the batch's "action" entry being the [B, A] one-hot of the logged action
    "per_action"     the A Q-values themselves (the result's importance is their mean; ``per_action_importance`` keeps [F, A])

and ``perturb_fn`` is None or ``create_default_perturb_fn``'s product.  A batch is a dict whose entry under the perturb
function's key (without one: "state_features", or the dict's only tensor pair) is the (values, presence) pair of the raw
features, column i being ``sorted_feature_ids[i]`` in the Preprocessor's input order.  Per batch and repeat: one Preprocessor
call, one layer-0 rg_fc_forward with RG_ACT_LINEAR (the shared pre-activation), the base forward, F ``torch.randperm(B)``
draws from torch's host generator in feature order (the stream the reference's loop consumes: ``torch.manual_seed``
reproduces it), rg_fi_sweep over the F variants, rg_fi_finish, and one host read.

Presence: the default perturbation permutes a feature's value AND its presence with the same permutation, and the
Preprocessor maps a row's (value, presence) of one feature to that feature's block of normalized columns and to nothing else.
Row b's block after the perturbation is therefore exactly row perm[b]'s block before it, which is why the sweep needs only
the normalized batch x and reads x[perm]: no raw batch is copied or normalized again.  The feature -> column-block table is
the Preprocessor's own (its ENUM expansion: ``Preprocessor.column_blocks``).
"""
import copy
import logging
from dataclasses import dataclass
from typing import Any, Callable, Optional, Union

import pandas as pd
import torch

from ... import _lib as L
from ... import ops
from ...models.dqn import FullyConnectedDQN
from ...prediction.predictor_wrapper import DiscreteDqnWithPreprocessor
from .feature_importance_base import FeatureImportanceBase

logger = logging.getLogger(__name__)
F32 = torch.float32
DEFAULT_KEY = "state_features"
WORKSPACE_CAP_BYTES = 64 << 20  # of partials per rg_fi_sweep launch: more variants than fit are swept in chunks


@dataclass
class FeatureImportancePerturbation(FeatureImportanceBase):
    # an iterable of batches; each one is scored `repeat` times
    data_loader: Any

    # (model, batch) -> [B, 1] predictions, called by the generic loop; or the name of a prediction the native sweep forms
    # itself: "max_q", "logged_action", "per_action"
    pred_fn: Union[str, Callable[[torch.nn.Module, Any], torch.Tensor]]

    # (batch, column) -> the batch with that raw column disturbed; it may work in place, the loop hands it a private copy.
    # None stands for create_default_perturb_fn(DEFAULT_KEY)
    perturb_fn: Optional[Callable[[Any, int], Any]] = None

    # independent disturbances drawn per batch and feature; their importances are averaged, so more of them is less noise
    repeat: int = 1

    def compute_feature_importance(self) -> pd.DataFrame:
        if isinstance(self.pred_fn, str):
            return self._native()
        return self._generic()

    def _generic(self) -> pd.DataFrame:
        """The method on any model through the two callables: a column's importance in one (batch, repeat) is the fp32
        mean of |prediction on the disturbed batch - prediction on the batch|, and its final value the fp32 mean of those.
        The features are visited in id order inside every repeat, which fixes the order of the perturb function's random
        draws (the default one draws a single torch.randperm per call)."""
        disturb = self.perturb_fn if self.perturb_fn is not None else create_default_perturb_fn(DEFAULT_KEY)
        scores = [[] for _ in self.sorted_feature_ids]
        for n_batch, batch in enumerate(self.data_loader):
            for _ in range(self.repeat):
                base = self.pred_fn(self.model, batch)
                for column, seen in enumerate(scores):
                    moved = self.pred_fn(self.model, disturb(copy.deepcopy(batch), column))
                    seen.append((moved - base).abs().mean().detach())
            logger.info("feature importance: batch %d scored %d time(s)", n_batch, self.repeat)
        return _ranked(self.sorted_feature_ids, [torch.stack(seen).mean().item() for seen in scores])

    # ---- the native sweep ---------------------------------------------------------------------------------------------
    def _checked(self):
        """-> (preprocessor, weights, biases, acts, blocks) of a model the sweep serves; refusals by name"""
        who, m = "FeatureImportancePerturbation", self.model
        if self.pred_fn not in L.FI_REDUCE:
            raise ValueError(f"{who}: pred_fn {self.pred_fn!r} is not a sentinel of the native sweep {sorted(L.FI_REDUCE)}")
        if self.perturb_fn is not None and not hasattr(self.perturb_fn, "fi_key"):
            raise NotImplementedError(f"{who}: the native sweep takes perturb_fn None or create_default_perturb_fn's product; "
                                      "pass a pred_fn callable to run the reference's loop with a perturb_fn of your own")
        if not isinstance(m, DiscreteDqnWithPreprocessor) or not isinstance(m.model, FullyConnectedDQN):
            inner = type(getattr(m, "model", m)).__name__
            what = "a dueling head" if "Dueling" in inner else f"a foreign model ({type(m).__name__} over {inner})"
            raise NotImplementedError(f"{who}: the native sweep serves a DiscreteDqnWithPreprocessor over a FullyConnectedDQN, "
                                      f"not {what}")
        fc = m.model.fc
        for what, on in (("batch norm", any(b is not None for b in fc.batch_norms())),
                         ("layer norm", any(n is not None for n in fc.layer_norms())),
                         ("dropout", any(p > 0.0 for p in fc.dropouts())), ("a residual wrapper", any(fc.residuals())),
                         ("atoms", m.model.num_atoms is not None), ("a precision other than PREC_F32", fc.precision != L.PREC_F32)):
            if on:
                raise NotImplementedError(f"{who}: the native sweep does not serve a network with {what}")
        lin = fc.linears()
        widest = max(l.out_features for l in lin)
        if widest > L.FI_MAX_WIDTH:
            raise NotImplementedError(f"{who}: a hidden width of {widest} is not supported by the native sweep (at most "
                                      f"{L.FI_MAX_WIDTH})")
        if len(lin) > L.FI_MAX_LAYERS or lin[-1].out_features > L.FI_MAX_ACTIONS:
            raise NotImplementedError(f"{who}: {len(lin)} layers / {lin[-1].out_features} actions are not supported by the native "
                                      f"sweep (at most {L.FI_MAX_LAYERS} / {L.FI_MAX_ACTIONS})")
        ids, known = list(self.sorted_feature_ids), list(m.state_preprocessor.sorted_features)
        if ids != known[:len(ids)]:  # id i labels raw column i: a reordered or foreign list would label the wrong feature
            raise ValueError(f"{who}: sorted_feature_ids {ids} are not the Preprocessor's leading input columns {known}")
        blocks = m.state_preprocessor.column_blocks()[:len(ids)]
        if max(e - s for s, e in blocks) > L.FI_MAX_WIDTH:
            raise NotImplementedError(f"{who}: a feature block wider than {L.FI_MAX_WIDTH} columns is not supported")
        weights = [l.weight.detach().float().contiguous() for l in lin]
        biases = [l.bias.detach().float().contiguous() for l in lin]
        return m.state_preprocessor, weights, biases, [L.ACT[a] for a in fc.activation_names], blocks

    def _pair(self, data):
        key = getattr(self.perturb_fn, "fi_key", None)
        if key is None and DEFAULT_KEY not in data:
            pairs = [k for k, v in data.items() if isinstance(v, (tuple, list)) and len(v) == 2]
            assert len(pairs) == 1, f"a batch without {DEFAULT_KEY!r} must hold exactly one (values, presence) pair"
            key = pairs[0]
        return data[key or DEFAULT_KEY]

    @torch.no_grad()
    def _native(self) -> pd.DataFrame:
        pre, weights, biases, acts, table = self._checked()
        dev, n, reduce = weights[0].device, len(self.sorted_feature_ids), L.FI_REDUCE[self.pred_fn]
        A, width = weights[-1].shape[0], max(e - s for s, e in table)
        C = A if self.pred_fn == "per_action" else 1
        blocks = torch.tensor(table, dtype=torch.int32).to(dev)
        total, rounds = torch.zeros(n, C, dtype=torch.float64), 0
        for batch_idx, data in enumerate(self.data_loader):
            values, presence = self._pair(data)
            mask = data["action"].to(dev).float().contiguous() if self.pred_fn == "logged_action" else None
            x = pre(values.to(dev), presence.to(dev))
            B = x.shape[0]
            z0 = torch.empty(B, weights[0].shape[0], dtype=F32, device=dev)
            ops.fc_forward(x, weights[0], biases[0], L.ACT["linear"], L.PREC_F32, y32=z0)
            q = x
            for w, b, act in zip(weights, biases, acts):  # the base forward: the per-layer launches the sweep's tail restates
                h = torch.empty(B, w.shape[0], dtype=F32, device=dev)
                ops.fc_forward(q, w, b, act, L.PREC_F32, y32=h)
                q = h
            per = max(1, ops.fi_partials(B, 1, A, reduce))
            chunk = max(1, min(65535, WORKSPACE_CAP_BYTES // (8 * per)))
            partials = torch.empty(min(n, chunk) * per, dtype=torch.float64, device=dev)
            for r in range(self.repeat):
                perm = torch.stack([torch.randperm(B) for _ in range(n)]).to(torch.int32).to(dev)
                importance = torch.empty(n, C, dtype=F32, device=dev)
                for v0 in range(0, n, chunk):
                    v1 = min(n, v0 + chunk)
                    ops.fi_sweep(x, z0, perm[v0:v1], blocks[v0:v1], weights, biases, acts, q, mask, reduce, width, partials)
                    ops.fi_finish(partials, B, importance[v0:v1])
                total += importance.cpu().double()  # the one host read
                rounds += 1
                logger.info(f"Processed {batch_idx} batches {r}-th time")
        mean = total / max(rounds, 1)
        self.per_action_importance = mean.float() if self.pred_fn == "per_action" else None
        return _ranked(self.sorted_feature_ids, mean.mean(dim=1).float().tolist())


def _ranked(feature_ids, importances) -> pd.DataFrame:
    """the result table: a row per feature, labelled by its id, the columns feature_id and feature_importance, the most
    important feature first"""
    ids = list(feature_ids)
    table = pd.DataFrame({"feature_id": ids, "feature_importance": [float(v) for v in importances]}, index=ids)
    return table.sort_values("feature_importance", ascending=False)


def create_default_perturb_fn(key: str):
    """-> a perturb function for batches that keep the raw (values, presence) pair under `key`: it re-deals one column of
    both tensors over the rows by ONE torch.randperm draw from the host generator, in place, and returns the batch"""

    def shuffle_column(batch, column):
        values, presence = batch[key]
        order = torch.randperm(values.shape[0])
        values[:, column] = values[order, column]
        presence[:, column] = presence[order, column]
        return batch

    shuffle_column.fi_key = key  # (where the native sweep finds the raw pair)
    return shuffle_column
