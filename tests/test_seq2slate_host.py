"""The host pieces that go with the Seq2Slate kernels: reagent_amd.model_utils.seq2slate_utils, the parameter classes of
reagent_amd.core.parameters_seq2slate and reagent_amd.training.ranking.helper.ips_clamp — against statements written out as
loops, and the helper against what rg_frechet_head computes on the device for the same importance weights."""
import dataclasses

import pytest
import torch

import reagent_amd._lib as L
from reagent_amd import ops
from reagent_amd.core.parameters_seq2slate import (IPSClamp, IPSClampMethod, LearningMethod, Seq2SlateParameters,
                                                   ips_clamp_code)
from reagent_amd.model_utils import seq2slate_utils as U
from reagent_amd.training.ranking import ips_clamp
from test_lstm_kernels import _bits

F32, F64 = torch.float32, torch.float64


def test_symbols_modes_and_architectures():
    assert (U.PADDING_SYMBOL, U.DECODER_START_SYMBOL) == (0, 1)
    assert {m.name: m.value for m in U.Seq2SlateMode} == dict(
        RANK_MODE="rank", PER_SEQ_LOG_PROB_MODE="per_sequence_log_prob", PER_SYMBOL_LOG_PROB_DIST_MODE="per_symbol_log_prob_dist",
        DECODE_ONE_STEP_MODE="decode_one_step", ENCODER_SCORE_MODE="encoder_score_mode")
    assert {a.name: a.value for a in U.Seq2SlateOutputArch} == dict(
        ENCODER_SCORE="encoder_score", AUTOREGRESSIVE="autoregressive", FRECHET_SORT="frechet_sort")


def test_mask_logits_by_idx_hides_the_reserved_and_the_fed_symbols():
    B, T, S = 3, 4, 6
    gen = torch.Generator().manual_seed(0)
    logits = torch.randn(B, T, S + 2, generator=gen, dtype=F64)
    fed = torch.stack([torch.randperm(S, generator=gen)[:T - 1] + 2 for _ in range(B)])
    tgt_in_idx = torch.cat((torch.full((B, 1), U.DECODER_START_SYMBOL), fed), dim=1)
    want = logits.clone()
    for b in range(B):
        for t in range(T):
            want[b, t, :2] = float("-inf")
            for u in range(1, t + 1):
                want[b, t, tgt_in_idx[b, u]] = float("-inf")
    got = U.mask_logits_by_idx(logits, tgt_in_idx)
    assert torch.equal(got, want)
    assert (logits[:, :, :2] == float("-inf")).all()  # the reserved columns are written in place, as the reference does


def test_per_symbol_reductions():
    B, T, C = 3, 4, 7
    gen = torch.Generator().manual_seed(1)
    probs = torch.softmax(torch.randn(B, T, C, generator=gen, dtype=F64), dim=2)
    idx = torch.randint(2, C, (B, T), generator=gen)
    want = torch.stack([torch.stack([probs[b, t, idx[b, t]] for t in range(T)]).prod() for b in range(B)]).view(B, 1)
    assert torch.equal(U.per_symbol_to_per_seq_probs(probs, idx), want)
    logs = torch.log(probs)
    want_log = torch.stack([torch.stack([logs[b, t, idx[b, t]] for t in range(T)]).sum() for b in range(B)]).view(B, 1)
    assert torch.allclose(U.per_symbol_to_per_seq_log_probs(logs, idx), want_log, rtol=0, atol=1e-15)
    # a product under 1e-40 is held there (in float32 a subnormal)
    tiny = torch.full((1, 2, 3), 1e-30)
    assert torch.equal(U.per_symbol_to_per_seq_probs(tiny, torch.full((1, 2), 2)), torch.full((1, 1), 1e-40))


def test_parameter_classes():
    p = Seq2SlateParameters()
    assert (p.on_policy, p.learning_method, p.ips_clamp, p.simulation) == (True, LearningMethod.REINFORCEMENT_LEARNING, None, None)
    assert [f.name for f in dataclasses.fields(Seq2SlateParameters)] == ["on_policy", "learning_method", "ips_clamp", "simulation"]
    assert [f.name for f in dataclasses.fields(IPSClamp)] == ["clamp_method", "clamp_max"]
    assert LearningMethod.SIMULATION.expect_slate_wise_reward and not LearningMethod.TEACHER_FORCING.expect_slate_wise_reward
    assert {m.name: m.value for m in IPSClampMethod} == dict(UNIVERSAL="universal", AGGRESSIVE="aggressive")
    with pytest.raises(NotImplementedError, match="simulation"):
        Seq2SlateParameters(simulation=object())
    with pytest.raises(dataclasses.FrozenInstanceError):
        p.on_policy = False
    assert ips_clamp_code(None) == (L.IPS_CLAMP_NONE, 0.0)
    assert ips_clamp_code(IPSClamp(IPSClampMethod.UNIVERSAL, 3)) == (L.IPS_CLAMP_UNIVERSAL, 3.0)
    assert ips_clamp_code(IPSClamp(IPSClampMethod.AGGRESSIVE, 0.5)) == (L.IPS_CLAMP_AGGRESSIVE, 0.5)


@pytest.mark.parametrize("clamp", [None, IPSClamp(IPSClampMethod.UNIVERSAL, 2.0), IPSClamp(IPSClampMethod.AGGRESSIVE, 2.0)])
def test_ips_clamp_is_the_clamp_of_the_head(backend, clamp):
    """one candidate and one step: p = 1, so the head's importance weight is 1 / logged exactly, and its clamped weight has the
    bits of the host helper's on that weight"""
    B, dev = 5, backend.device
    logged = torch.tensor([0.25, 0.5, 1.0, 0.125, 0.75])
    impt = (1.0 / logged.double())
    want = ips_clamp(impt, clamp)
    assert want is not impt
    if clamp is not None:
        hit = impt > clamp.clamp_max
        assert 1 <= int(hit.sum()) <= B - 1
        assert torch.equal(want[hit], torch.full_like(want[hit], 2.0 if clamp.clamp_method == IPSClampMethod.UNIVERSAL else 0.0))
        assert torch.equal(want[~hit], impt[~hit])
    z = lambda *s: torch.zeros(*s, dtype=F32, device=dev)  # noqa: E731
    out = dict(impt=z(B), clamped=z(B), sums=z(3))
    method, cmax = ips_clamp_code(clamp)
    ops.frechet_head(z(B, 4), z(4), z(1), torch.full((B, 1), 2, dtype=torch.int64, device=dev), 1, B, z(B), z(B),
                     torch.zeros(ops.frechet_head_workspace(B, 4), dtype=F64, device=dev), logged=logged.to(dev),
                     reward=torch.ones(B, device=dev), clamp_method=method, clamp_max=cmax, **out)
    assert torch.equal(_bits(out["impt"]), _bits(impt.float()))
    assert torch.equal(_bits(out["clamped"]), _bits(want.float()))
    sums = torch.stack((-want.mean(), -impt.mean(), -want.mean()))  # reward 1, no baseline
    assert torch.equal(_bits(out["sums"]), _bits(sums.float()))


def test_ranking_input_from_input_derives_indices_sequences_and_masks():
    import reagent_amd.core.types as rlt

    B, S, T, D = 3, 5, 3, 2
    gen = torch.Generator().manual_seed(2)
    state, cand = torch.randn(B, 4, generator=gen), torch.randn(B, S, D, generator=gen)
    action = torch.stack([torch.randperm(S, generator=gen)[:T] for _ in range(B)])
    logged, reward = torch.rand(B, 1, generator=gen) + 0.1, torch.randn(B, 1, generator=gen)
    b = rlt.PreprocessedRankingInput.from_input(state, cand, "cpu", action=action, logged_propensities=logged, slate_reward=reward,
                                                optimal_action=action.flip(1))
    assert [f.name for f in dataclasses.fields(b)] == [
        "state", "src_seq", "src_src_mask", "tgt_in_seq", "tgt_out_seq", "tgt_tgt_mask", "slate_reward", "position_reward",
        "src_in_idx", "tgt_in_idx", "tgt_out_idx", "tgt_out_probs", "optim_tgt_in_idx", "optim_tgt_out_idx", "optim_tgt_in_seq",
        "optim_tgt_out_seq", "extras"]
    assert len(b) == b.batch_size() == B
    assert torch.equal(b.state.float_features, state) and torch.equal(b.src_seq.float_features, cand)
    assert torch.equal(b.src_in_idx, torch.arange(2, S + 2).expand(B, S)) and b.src_in_idx.dtype == torch.int64
    assert b.src_src_mask.dtype == torch.int8 and torch.equal(b.src_src_mask, torch.ones(B, S, S, dtype=torch.int8))
    assert torch.equal(b.tgt_out_idx, action + 2) and b.tgt_in_idx.dtype == torch.int64
    assert torch.equal(b.tgt_out_probs, logged) and torch.equal(b.slate_reward, reward) and b.position_reward is None
    assert torch.equal(b.tgt_tgt_mask, torch.tril(torch.ones(T, T, dtype=torch.bool)).view(1, T, T))
    for i in range(B):
        assert b.tgt_in_idx[i].tolist() == [U.DECODER_START_SYMBOL] + (action[i, :-1] + 2).tolist()
        for t in range(T):
            assert torch.equal(b.tgt_out_seq.float_features[i, t], cand[i, action[i, t]])
            want_in = torch.zeros(D) if t == 0 else cand[i, action[i, t - 1]]
            assert torch.equal(b.tgt_in_seq.float_features[i, t], want_in)
    assert torch.equal(b.optim_tgt_out_idx, action.flip(1) + 2)
    assert torch.equal(b.optim_tgt_out_seq.float_features[:, 0], cand[torch.arange(B), action[:, -1]])
    # no slate: the target members stay None
    bare = rlt.PreprocessedRankingInput.from_input(state, cand, "cpu")
    assert bare.tgt_out_idx is None and bare.tgt_in_seq is None and bare.tgt_tgt_mask is None and bare.extras is None
    # bare tensors are refused by the constructor, by the reference's message
    with pytest.raises(ValueError, match=r"Use from_tensors\(\)"):
        rlt.PreprocessedRankingInput(state=state, src_seq=rlt.FeatureData(cand))
    moved = b.float()  # TensorDataClass's forwarding reaches the nested members
    assert moved.tgt_out_idx.dtype == torch.float32 and moved.state.float_features.dtype == torch.float32
    out = rlt.RankingOutput(log_probs=torch.zeros(B, 1))
    assert [f.name for f in dataclasses.fields(out)] == ["ranked_tgt_out_idx", "ranked_per_symbol_probs", "ranked_per_seq_probs",
                                                          "log_probs", "encoder_scores"]
    assert out.ranked_tgt_out_idx is None and out.encoder_scores is None


def test_ranking_batch_is_seeded_distinct_and_positive(backend):
    """synthetic.ranking_batch: built through from_input; its slate goes straight into rg_frechet_head"""
    import reagent_amd.core.types as rlt
    from reagent_amd import synthetic

    B, S, T, SD, CD = 12, 5, 3, 4, 3
    a, b, c = (synthetic.ranking_batch(B, S, T, SD, CD, seed=s) for s in (7, 7, 8))
    assert isinstance(a, rlt.PreprocessedRankingInput)
    assert torch.equal(a.tgt_out_idx, b.tgt_out_idx) and torch.equal(a.slate_reward, b.slate_reward)
    assert not torch.equal(a.src_seq.float_features, c.src_seq.float_features)
    assert a.state.float_features.shape == (B, SD) and a.src_seq.float_features.shape == (B, S, CD)
    assert a.tgt_out_idx.shape == (B, T) and a.tgt_out_probs.shape == (B, 1) and a.slate_reward.shape == (B, 1)
    assert all(len(set(r)) == T for r in a.tgt_out_idx.tolist()) and ((a.tgt_out_idx >= 2) & (a.tgt_out_idx < S + 2)).all()
    assert (a.tgt_out_probs > 0).all() and (a.tgt_out_probs < 1).all()
    dev, E = backend.device, 8
    z = lambda *s: torch.zeros(*s, dtype=F32, device=dev)  # noqa: E731
    log_prob, p = z(B), z(B)
    ops.frechet_head(z(S * B, E), z(E), z(1), a.tgt_out_idx.to(dev), S, B, log_prob, p,
                     torch.zeros(ops.frechet_head_workspace(B, E), dtype=F64, device=dev))
    want = torch.tensor(1.0 / (S * (S - 1) * (S - 2)), dtype=F64)  # equal scores: a uniform Plackett-Luce law
    assert torch.equal(_bits(p), _bits(want.float().expand(B)))
