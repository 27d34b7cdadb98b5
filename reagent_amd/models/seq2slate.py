"""Seq2SlateTransformerNet and BaselineNet with the surface of reagent/models/seq2slate.py (:358-370, :382-843, :846-956), executed
on the HIP kernels, for the output architectures FRECHET_SORT (log-probabilities, training, greedy and sampled ranking) and
ENCODER_SCORE (forward only: ranking and ENCODER_SCORE_MODE).

What runs, rows ordered (s, b), N = S * B, E = dim_model:

  state_embed = Linear(state)  [B, Es],  cand_embed = Linear(src_seq)  [N, Ec]   rg_fc_forward
  x = (sqrt(Es) state_embed[b] | sqrt(Ec) cand_embed[(s, b)])                     rg_s2s_embed_join
  per nn.TransformerEncoderLayer (post-norm, relu, dropout 0, no mask), x -> y:
    q | k | v = x W^T + b (the packed in_proj)                                    rg_fc_forward
    ctx = softmax(q k^T / sqrt(hd)) v per (b, head)                               rg_attn_forward
    s1 = LayerNorm1(x + ctx Wo^T + bo)                                            rg_fc_forward, rg_residual_join, rg_layer_norm_forward
    y  = LayerNorm2(s1 + Linear(relu(Linear(s1))))                                FCStack, rg_residual_join, rg_layer_norm_forward
  behind the encoder: rg_frechet_head (the logged slate's log-probability, the trainer's loss and d loss / d (mem, scorer)) or
  rg_frechet_rank (ranking)

The backward walks the same list in reverse through models/encoder_ops.py, which TransformerSyntheticRewardNet shares.

torch's own modules are constructed as parameter holders in the reference's order (encoder, encoder_scorer, decoder,
positional_encoding_decoder, state_embedder, candidate_embedder) and the reference's xavier_uniform_ loop then runs over every
parameter with dim() > 1: the same seed gives the reference's initial weights bit for bit, and the state_dict keys are its keys
(seq2slate.encoder.transformer_encoder.layers.<i>.*, ...).  The decoder and its positional encoding are parameter holders under
these two architectures, as in the reference, which builds them and never runs them: they get no gradient.

Four parameter slices carry no information: each layer's key bias in_proj_bias[E:2E] and, in the first layer, the key weight on
the state columns in_proj_weight[E:2E, :state_embed_dim] (the state embedding is the same in every candidate's row) shift every
key of a batch row alike; the last layer's norm2.bias and encoder_scorer.bias shift every candidate's score alike; no soft-max
sees either.  Their gradients are computed like any other, with no special case, and are rounding noise, which Adam turns into
steps of full size: the reference's own float32 twins differ there by 1e-2 after four steps, by 7e-7 elsewhere.

Kept quirks: temperature is accepted and never read; Embedder multiplies by sqrt(dim_out) of its own half (state_embed_dim defaults
to dim_model // 2, the candidate half is the rest); the encoder sees no mask; the greedy and encoder rankings return one-hot
"probabilities" and ranked_per_seq_probs = 1; ENCODER_SCORE_MODE ends in .squeeze() with no dim, so its output is [T] at B = 1.
The sampled ranking draws with Philox keyed by a seed taken from torch's generator, not with torch.multinomial: the law is the
reference's, the stream is not.

Refused by name: output_arch=AUTOREGRESSIVE, PER_SYMBOL_LOG_PROB_DIST_MODE, DECODE_ONE_STEP_MODE, log-probabilities on an
ENCODER_SCORE net (the reference's decode raises there too), max_src_seq_len > 64, dim_model > 512, a head wider than 128,
num_heads not dividing dim_model, a batch whose src_seq_len exceeds max_src_seq_len or whose tgt_seq_len exceeds src_seq_len,
data parallel.  forward carries no autograd graph (training goes through Seq2SlateTrainer)."""
from typing import NamedTuple, Optional

import torch
import torch.nn as nn

from .. import _lib as L
from .. import ops
from ..core import types as rlt
from ..engine import FCStack, ensure_slab
from ..model_utils.seq2slate_utils import Seq2SlateMode, Seq2SlateOutputArch
from . import encoder_ops
from .base import ModelBase

F32 = torch.float32
WHO = "Seq2SlateTransformerNet"


class Seq2SlateTransformerOutput(NamedTuple):
    ranked_per_symbol_probs: Optional[torch.Tensor]
    ranked_per_seq_probs: Optional[torch.Tensor]
    ranked_tgt_out_idx: Optional[torch.Tensor]
    per_symbol_log_probs: Optional[torch.Tensor]
    per_seq_log_probs: Optional[torch.Tensor]
    encoder_scores: Optional[torch.Tensor]


class _Embedder(nn.Module):
    def __init__(self, dim_in, dim_out):
        super().__init__()
        self.dim_in, self.dim_out = dim_in, dim_out
        self.linear = nn.Linear(dim_in, dim_out)


class _EncoderHolder(nn.Module):
    def __init__(self, dim_model, num_heads, dim_feedforward, num_layers):
        super().__init__()
        layer = nn.TransformerEncoderLayer(d_model=dim_model, dim_feedforward=dim_feedforward, nhead=num_heads, dropout=0.0)
        self.transformer_encoder = nn.TransformerEncoder(layer, num_layers=num_layers)


class _DecoderHolder(nn.Module):
    def __init__(self, dim_model, num_heads, dim_feedforward, num_layers):
        super().__init__()
        assert num_layers >= 1
        self.layers = nn.ModuleList([nn.TransformerDecoderLayer(d_model=dim_model, nhead=num_heads, dim_feedforward=dim_feedforward,
                                                                dropout=0.0) for _ in range(num_layers)])


class _PositionalEncoding(nn.Module):
    def __init__(self, dim_model):
        super().__init__()
        self.pos_embed = nn.Linear(dim_model + 1, dim_model)


class _Seq2SlateHolder(nn.Module):
    """Seq2SlateTransformerModel's parameters under its names, constructed in its order and initialised by its loop"""

    def __init__(self, state_dim, candidate_dim, num_stacked_layers, num_heads, dim_model, dim_feedforward, state_embed_dim):
        super().__init__()
        self.encoder = _EncoderHolder(dim_model, num_heads, dim_feedforward, num_stacked_layers)
        self.encoder_scorer = nn.Linear(dim_model, 1)
        self.decoder = _DecoderHolder(dim_model, num_heads, dim_feedforward, num_stacked_layers)
        self.positional_encoding_decoder = _PositionalEncoding(dim_model)
        self.state_embedder = _Embedder(state_dim, state_embed_dim)
        self.candidate_embedder = _Embedder(candidate_dim, dim_model - state_embed_dim)
        for p in self.parameters():
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)


class BaselineNet(nn.Module):
    """:358-370 — an MLP on the state alone, one output: Linear, relu, (Linear, relu) x (num_stacked_layers - 1), Linear"""

    def __init__(self, state_dim, dim_feedforward, num_stacked_layers):
        super().__init__()
        nn_blocks = [nn.Linear(state_dim, dim_feedforward), nn.ReLU()]
        assert num_stacked_layers >= 1
        for _ in range(num_stacked_layers - 1):
            nn_blocks.extend([nn.Linear(dim_feedforward, dim_feedforward), nn.ReLU()])
        nn_blocks.append(nn.Linear(dim_feedforward, 1))
        self.mlp = nn.Sequential(*nn_blocks)
        self._stack = None

    def stack(self):
        if self._stack is None:
            lin = [m for m in self.mlp if isinstance(m, nn.Linear)]
            acts = [L.ACT["relu"]] * (len(lin) - 1) + [L.ACT["linear"]]
            self._stack = FCStack([m.weight for m in lin], [m.bias for m in lin], acts, L.PREC_F32)
        return self._stack

    def run(self, input, save=False):
        """-> (b [B, 1], the transposed staged input of a saving pass)"""
        dev = next(self.parameters()).device
        x = input.state.float_features.to(dev).float().contiguous()
        L.require_cuda(x, "state")
        return encoder_ops.stack_forward(self.stack(), x, save)

    def forward(self, input: rlt.PreprocessedRankingInput):
        return self.run(input)[0]


class Seq2SlateTransformerNet(ModelBase):
    def __init__(
        self,
        state_dim: int,
        candidate_dim: int,
        num_stacked_layers: int,
        dim_model: int,
        max_src_seq_len: int,
        max_tgt_seq_len: int,
        output_arch: Seq2SlateOutputArch,
        temperature: float,
        num_heads: int,
        dim_feedforward: int,
        state_embed_dim: Optional[int] = None,
    ):
        super().__init__()
        output_arch = Seq2SlateOutputArch(getattr(output_arch, "value", output_arch))
        if output_arch == Seq2SlateOutputArch.AUTOREGRESSIVE:
            raise NotImplementedError(f"{WHO}: output_arch AUTOREGRESSIVE is not supported (FRECHET_SORT, ENCODER_SCORE: the "
                                      "decoder needs masked and cross attention, which the attention kernels do not have)")
        if num_heads < 1 or dim_model % num_heads != 0:
            raise NotImplementedError(f"{WHO}: num_heads {num_heads} does not divide dim_model {dim_model}")
        if dim_model > min(L.ATTN_MAX_EMBED, L.S2S_MAX_EMBED):
            raise NotImplementedError(f"{WHO}: dim_model {dim_model} is not supported (up to {L.ATTN_MAX_EMBED})")
        if dim_model // num_heads > L.ATTN_MAX_HEAD_DIM:
            raise NotImplementedError(f"{WHO}: head width {dim_model // num_heads} is not supported (dim_model / num_heads up to "
                                      f"{L.ATTN_MAX_HEAD_DIM})")
        if not 1 <= max_src_seq_len <= L.S2S_MAX_SEQ_LEN:
            raise NotImplementedError(f"{WHO}: max_src_seq_len {max_src_seq_len} is not supported (1 .. {L.S2S_MAX_SEQ_LEN}: a lane "
                                      "per candidate)")
        if state_embed_dim is None:
            state_embed_dim = dim_model // 2
        if not 1 <= state_embed_dim < dim_model:
            raise NotImplementedError(f"{WHO}: state_embed_dim {state_embed_dim} is not supported (1 .. dim_model - 1)")
        self.state_dim, self.candidate_dim, self.num_stacked_layers, self.dim_model = state_dim, candidate_dim, num_stacked_layers, dim_model
        self.max_src_seq_len, self.max_tgt_seq_len, self.output_arch, self.temperature = max_src_seq_len, max_tgt_seq_len, output_arch, temperature
        self.num_heads, self.dim_feedforward, self.state_embed_dim = num_heads, dim_feedforward, state_embed_dim
        self.seq2slate = _Seq2SlateHolder(state_dim, candidate_dim, num_stacked_layers, num_heads, dim_model, dim_feedforward,
                                          state_embed_dim)
        self._transposed = encoder_ops.TransposedCache()
        self._stacks = None

    def get_distributed_data_parallel_model(self):
        raise NotImplementedError(f"{WHO} has no data-parallel path (get_distributed_data_parallel_model is not supported)")

    def input_prototype(self):
        return rlt.PreprocessedRankingInput.from_tensors(
            state=torch.randn(1, self.state_dim), src_seq=torch.randn(1, self.max_src_seq_len, self.candidate_dim),
            tgt_in_seq=torch.randn(1, self.max_tgt_seq_len, self.candidate_dim),
            tgt_out_seq=torch.randn(1, self.max_tgt_seq_len, self.candidate_dim), slate_reward=torch.randn(1))

    # ---- the encoder ---------------------------------------------------------------------------------------------------------
    def _layers(self):
        return list(self.seq2slate.encoder.transformer_encoder.layers)

    def trained_parameters(self):
        """the parameters the two architectures run (the decoder's and its positional encoding's are holders)"""
        m = self.seq2slate
        held = {id(p) for mod in (m.decoder, m.positional_encoding_decoder) for p in mod.parameters()}
        return [p for p in self.parameters() if id(p) not in held]

    def _ff_stacks(self):
        if self._stacks is None:
            self._stacks = [encoder_ops.block(m.linear1, m.linear2) for m in self._layers()]
        return self._stacks

    def _layer_forward(self, m, st, x, S, B, save):
        N, E = x.shape
        new = lambda *shape: torch.empty(*shape, dtype=F32, device=x.device)  # noqa: E731
        t = {}
        at = m.self_attn
        qkv = new(N, 3 * E)
        ops.fc_forward(x, at.in_proj_weight.detach(), at.in_proj_bias.detach(), L.ACT["linear"], L.PREC_F32, y32=qkv)
        ctx = new(N, E)
        p = new(B, self.num_heads, S, S) if save else None
        ops.attn_forward(qkv[:, :E], qkv[:, E:2 * E], qkv[:, 2 * E:], S, B, self.num_heads, ctx, p)
        o = new(N, E)
        ops.fc_forward(ctx, at.out_proj.weight.detach(), at.out_proj.bias.detach(), L.ACT["linear"], L.PREC_F32, y32=o)
        pre1, s1 = new(N, E), new(N, E)
        ops.residual_join(x, pre1, S, B, b=o)
        t["ln1"] = (new(N), new(N)) if save else (None, None)
        ops.layer_norm_forward(pre1, m.norm1.weight.detach(), m.norm1.bias.detach(), m.norm1.eps, L.ACT["linear"], y32=s1,
                               mean=t["ln1"][0], rstd=t["ln1"][1])
        f, t["xt_ff"] = encoder_ops.stack_forward(st, s1, save)
        pre2, y = new(N, E), new(N, E)
        ops.residual_join(s1, pre2, S, B, b=f)
        t["ln2"] = (new(N), new(N)) if save else (None, None)
        ops.layer_norm_forward(pre2, m.norm2.weight.detach(), m.norm2.bias.detach(), m.norm2.eps, L.ACT["linear"], y32=y,
                               mean=t["ln2"][0], rstd=t["ln2"][1])
        if save:
            t.update(x=x, qkv=qkv, p=p, ctx=ctx, pre1=pre1, pre2=pre2)
        return y, t

    def encode(self, input, save=False):
        """-> the tape of one pass: S, B, the last layer's output mem [S * B, E] and (save) what the backward reads"""
        dev = next(self.parameters()).device
        state = input.state.float_features.to(dev).float().contiguous()
        src = input.src_seq.float_features.to(dev).float()
        L.require_cuda(state, "state")
        assert state.ndim == 2 and src.ndim == 3 and src.shape[0] == state.shape[0], (state.shape, src.shape)
        assert state.shape[1] == self.state_dim and src.shape[2] == self.candidate_dim, (state.shape, src.shape)
        B, S, _ = src.shape
        if S > self.max_src_seq_len:
            raise NotImplementedError(f"{WHO}: src_seq_len {S} exceeds max_src_seq_len {self.max_src_seq_len}")
        m = self.seq2slate
        E, Es = self.dim_model, self.state_embed_dim
        cand = src.transpose(0, 1).contiguous().view(S * B, self.candidate_dim)  # rows (s, b)
        new = lambda *shape: torch.empty(*shape, dtype=F32, device=dev)  # noqa: E731
        se, ce, x = new(B, Es), new(S * B, E - Es), new(S * B, E)
        ops.fc_forward(state, m.state_embedder.linear.weight.detach(), m.state_embedder.linear.bias.detach(), L.ACT["linear"],
                       L.PREC_F32, y32=se)
        ops.fc_forward(cand, m.candidate_embedder.linear.weight.detach(), m.candidate_embedder.linear.bias.detach(),
                       L.ACT["linear"], L.PREC_F32, y32=ce)
        ops.s2s_embed_join(se, ce, S, B, x)
        tape = dict(S=S, B=B, state=state, cand=cand, layers=[])
        h = x
        for layer, st in zip(self._layers(), self._ff_stacks()):
            h, t = self._layer_forward(layer, st, h, S, B, save)
            tape["layers"].append(t)
        tape["mem"] = h
        return tape

    def scorer(self):
        sc = self.seq2slate.encoder_scorer
        return sc.weight.detach().view(-1), sc.bias.detach()

    # ---- backward ------------------------------------------------------------------------------------------------------------
    def grad_views(self):
        params = list(self.parameters())
        slab = ensure_slab(params)
        return slab, {id(p): slab.view(slab.grad, i) for i, p in enumerate(params)}

    def backward(self, tape, dmem, dw, db):
        """d loss / d every trained parameter from a saving pass and the head's outputs (dmem [S * B, E], dw [E] and db [1] =
        the scorer's gradients), written into the parameters' gradient slab (the caller publishes it)"""
        slab, grad = self.grad_views()
        G = lambda p: grad[id(p)]  # noqa: E731
        m = self.seq2slate
        S, B, E, Es = tape["S"], tape["B"], self.dim_model, self.state_embed_dim
        N = S * B
        new = lambda *shape: torch.empty(*shape, dtype=F32, device=dmem.device)  # noqa: E731
        G(m.encoder_scorer.weight).view(-1).copy_(dw)
        G(m.encoder_scorer.bias).copy_(db)
        d = dmem
        layers, stacks = self._layers(), self._ff_stacks()
        for i in range(len(layers) - 1, -1, -1):
            layer, st, t = layers[i], stacks[i], tape["layers"][i]
            at = layer.self_attn
            # y = LayerNorm2(s1 + ff(s1)), s1 = LayerNorm1(x + out_proj(ctx))
            dpre2 = encoder_ops.layer_norm_backward(layer.norm2, d, t["pre2"], t["ln2"], G(layer.norm2.weight), G(layer.norm2.bias))
            ds1_ff = new(N, E)
            st.backward(dpre2, t["xt_ff"], [G(layer.linear1.weight), G(layer.linear2.weight)],
                        [G(layer.linear1.bias), G(layer.linear2.bias)], dx32=ds1_ff)
            ds1 = new(N, E)
            ops.residual_join_backward([dpre2, ds1_ff], ds1)
            dpre1 = encoder_ops.layer_norm_backward(layer.norm1, ds1, t["pre1"], t["ln1"], G(layer.norm1.weight), G(layer.norm1.bias))
            dctx = encoder_ops.linear_backward(self._transposed, dpre1, t["ctx"], f"out_proj{i}", at.out_proj.weight,
                                               G(at.out_proj.weight), G(at.out_proj.bias))
            dqkv = new(N, 3 * E)
            qkv = t["qkv"]
            ops.attn_backward(dctx, qkv[:, :E], qkv[:, E:2 * E], qkv[:, 2 * E:], t["p"], S, B, self.num_heads, dqkv[:, :E],
                              dqkv[:, E:2 * E], dqkv[:, 2 * E:])
            dx_attn = encoder_ops.linear_backward(self._transposed, dqkv, t["x"], f"in_proj{i}", at.in_proj_weight,
                                                  G(at.in_proj_weight), G(at.in_proj_bias))
            d = new(N, E)
            ops.residual_join_backward([dpre1, dx_attn], d)
        dse, dce = new(B, Es), new(N, E - Es)
        ops.s2s_embed_join_backward(d, S, B, dse, dce)
        lin = m.state_embedder.linear
        encoder_ops.linear_backward(self._transposed, dse, tape["state"], "state_embedder", lin.weight, G(lin.weight), G(lin.bias),
                                    need_dx=False)
        lin = m.candidate_embedder.linear
        encoder_ops.linear_backward(self._transposed, dce, tape["cand"], "candidate_embedder", lin.weight, G(lin.weight),
                                    G(lin.bias), need_dx=False)
        return slab

    # ---- the head ------------------------------------------------------------------------------------------------------------
    def _tgt_out_idx(self, input, S):
        idx = input.tgt_out_idx
        assert idx is not None
        idx = idx.to(next(self.parameters()).device).long().contiguous()
        if idx.shape[1] > S:
            raise NotImplementedError(f"{WHO}: tgt_seq_len {idx.shape[1]} exceeds src_seq_len {S}")
        return idx

    def run_head(self, input, save=False, logged=None, reward=None, baseline=None, clamp_method=L.IPS_CLAMP_NONE, clamp_max=0.0):
        """PER_SEQ_LOG_PROB_MODE behind the encoder -> dict(tape, log_prob, p [B]; with logged and reward: impt, clamped [B],
        sums [3]; with save: dscore, dmem, dw, dbias)"""
        if self.output_arch != Seq2SlateOutputArch.FRECHET_SORT:
            raise NotImplementedError(f"{WHO}: log-probabilities and training need output_arch FRECHET_SORT (an ENCODER_SCORE net "
                                      "has no decoding distribution)")
        tape = self.encode(input, save=save)
        S, B, E = tape["S"], tape["B"], self.dim_model
        idx = self._tgt_out_idx(input, S)
        dev = tape["mem"].device
        new = lambda *shape: torch.empty(*shape, dtype=F32, device=dev)  # noqa: E731
        r = dict(tape=tape, log_prob=new(B), p=new(B))
        kw = {}
        if logged is not None:
            r.update(impt=new(B), clamped=new(B), sums=new(3))
            kw = dict(logged=logged, reward=reward, baseline=baseline, clamp_method=clamp_method, clamp_max=clamp_max,
                      impt=r["impt"], clamped=r["clamped"], sums=r["sums"])
            if save:
                r.update(dscore=new(B, S), dmem=new(S * B, E), dw=new(E), dbias=new(1))
                kw.update(dscore=r["dscore"], dmem=r["dmem"], dw=r["dw"], dbias=r["dbias"])
        w, b = self.scorer()
        ws = torch.empty(ops.frechet_head_workspace(B, E), dtype=torch.float64, device=dev)
        ops.frechet_head(tape["mem"], w, b, idx, S, B, r["log_prob"], r["p"], ws, **kw)
        return r

    def _rank(self, input, tgt_seq_len, greedy):
        tape = self.encode(input)
        S, B = tape["S"], tape["B"]
        T = self.max_tgt_seq_len if tgt_seq_len is None else tgt_seq_len
        if T > S:
            raise NotImplementedError(f"{WHO}: tgt_seq_len {T} exceeds src_seq_len {S}")
        assert greedy is not None
        dev = tape["mem"].device
        idx = torch.empty(B, T, dtype=torch.int64, device=dev)
        probs, per_seq = torch.empty(B, T, S + 2, dtype=F32, device=dev), torch.empty(B, dtype=F32, device=dev)
        if self.output_arch == Seq2SlateOutputArch.ENCODER_SCORE:
            mode, seed = L.FRECHET_RANK_ENCODER, 0
        elif greedy:
            mode, seed = L.FRECHET_RANK_GREEDY, 0
        else:  # a fresh Philox key per call, taken from torch's generator (so torch.manual_seed makes the draws repeatable)
            mode, seed = L.FRECHET_RANK_SAMPLED, int(torch.randint(0, 2 ** 62, (1,)).item())
        w, b = self.scorer()
        ops.frechet_rank(mode, S, B, idx, probs, per_seq, mem=tape["mem"], w=w, bias=b, seed=seed)
        return rlt.RankingOutput(ranked_per_symbol_probs=probs, ranked_per_seq_probs=per_seq.view(B, 1), ranked_tgt_out_idx=idx)

    def _encoder_scores(self, input):
        if self.output_arch != Seq2SlateOutputArch.ENCODER_SCORE:
            raise NotImplementedError(f"{WHO}: ENCODER_SCORE_MODE needs output_arch ENCODER_SCORE (the reference asserts it)")
        tape = self.encode(input)
        S, B, E = tape["S"], tape["B"], self.dim_model
        idx = self._tgt_out_idx(input, S)
        T = idx.shape[1]
        # encoder_scorer on the rows of mem that tgt_out_idx names: rows (b, t) gathered, then the [E] -> 1 linear
        rows = ((idx - 2) * B + torch.arange(B, device=idx.device).view(B, 1)).view(-1)
        picked = tape["mem"].index_select(0, rows)
        sc = self.seq2slate.encoder_scorer
        out = torch.empty(B * T, 1, dtype=F32, device=picked.device)
        ops.fc_forward(picked, sc.weight.detach(), sc.bias.detach(), L.ACT["linear"], L.PREC_F32, y32=out)
        return rlt.RankingOutput(encoder_scores=out.view(B, T, 1).squeeze())

    @torch.no_grad()
    def forward(self, input: rlt.PreprocessedRankingInput, mode: Seq2SlateMode, tgt_seq_len: Optional[int] = None,
                greedy: Optional[bool] = None):
        mode = Seq2SlateMode(getattr(mode, "value", mode))
        if mode == Seq2SlateMode.RANK_MODE:
            return self._rank(input, tgt_seq_len, greedy)
        if mode == Seq2SlateMode.PER_SEQ_LOG_PROB_MODE:
            assert input.tgt_in_idx is not None and input.tgt_out_idx is not None
            r = self.run_head(input)
            return rlt.RankingOutput(log_probs=r["log_prob"].view(-1, 1))
        if mode == Seq2SlateMode.ENCODER_SCORE_MODE:
            return self._encoder_scores(input)
        raise NotImplementedError(f"{WHO}: mode {mode.name} is not supported (RANK_MODE, PER_SEQ_LOG_PROB_MODE, ENCODER_SCORE_MODE)")
