"""The CEM planner's kernels (reagent_amd/csrc/cem.hip) against float64 statements: the rollout step by step on its own traced
entry states (teacher-forced, so errors do not compound), the placement invariance of a trajectory's bits, the noise recipe
against its numpy restatement, rg_cem_refit and rg_cem_tally against numpy, and the ensemble mean (a departure)."""
import numpy as np
import pytest
import torch

import cem_statement as CS
from reagent_amd import ops
from reagent_amd.core import types as rlt
from reagent_amd.models.cem_planner import CEMPlannerNetwork
from reagent_amd.models.world_model import MemoryNetwork

F32, F64, I32 = torch.float32, torch.float64, torch.int32


def _ulp(x):
    return float(np.spacing(np.float32(abs(float(x)))))


def _bound(ref64, torch32):
    """tests/test_lstm_kernels.py's self-calibrating bound: four times torch's own fp32 error, at least 4 ulp of the largest"""
    own = (torch32.double() - ref64).abs().max().item()
    return max(4.0 * own, 4.0 * _ulp(ref64.abs().max().item()))


def _close(got, ref64, torch32, what):
    bound = _bound(ref64, torch32)
    err = (got.double() - ref64).abs().max().item()
    print(f"{what}: kernel error {err:.3e}, bound {bound:.3e}, ratio {err / bound:.3f}")
    assert err <= bound, (what, err, bound)
    return bound


def _planner(dev, *, H, L, S, A, G, P, T, M=1, E=1, te=True, seed=0, nt_bias=None, w_hh_scale=None, discrete=False, gamma=0.9):
    torch.manual_seed(seed)
    nets = [MemoryNetwork(S, A, H, L, G) for _ in range(M)]
    for net in nets:
        with torch.no_grad():
            if nt_bias is not None:
                net.mdnrnn.gmm_linear.bias[-1] = nt_bias
            if w_hh_scale is not None:
                for k in range(L):
                    getattr(net.mdnrnn.rnn, f"weight_hh_l{k}").mul_(w_hh_scale)
        net.to(dev)
    kw = {} if discrete else dict(action_upper_bounds=np.ones(A), action_lower_bounds=-np.ones(A))
    return CEMPlannerNetwork(nets, 2, P, E, 1, T, S, A, discrete, te, gamma, **kw)


def _run(pl, dev, seed, iteration=0, noise=None, sol=None, trace=True, grouping=None):
    P, T, A, S = pl.cem_pop_size, pl.plan_horizon_length, pl.action_dim, pl.state_dim
    g = torch.Generator().manual_seed(seed)
    init = torch.randn(S, generator=g)
    if sol is None:
        sol = torch.rand(P, T, A, generator=g) * 2 - 1
    out = torch.full((P,), -7.0, dtype=F64, device=dev)
    tr = pl._rollout(init.to(dev), sol.to(dev).contiguous(), None, out, seed=seed, iteration=iteration, noise=noise, trace=trace,
                     grouping=grouping)
    return init, sol, out.cpu(), None if tr is None else tr.cpu()


SHAPES = {
    "h1_one_row": dict(H=1, L=2, S=1, A=1, G=1, P=1, T=1, te=False),
    "h31_n31": dict(H=31, L=2, S=4, A=3, G=3, P=31, T=5, te=True, nt_bias=1.5),
    "h33_n33_g32_s33": dict(H=33, L=2, S=33, A=1, G=32, P=33, T=5, te=True, nt_bias=1.5),
    "h100_l4_two_models": dict(H=100, L=4, S=4, A=3, G=3, P=33, T=2, M=2, te=True, nt_bias=1.5),
    "h256_l1": dict(H=256, L=1, S=4, A=1, G=1, P=33, T=1, te=False),
    "h8_n65": dict(H=8, L=2, S=4, A=3, G=3, P=65, T=5, te=True, nt_bias=1.5),
}
SEED = 11


def _check_rollout(pl, dev, cfg, seed):
    S, A, G, T, P = cfg["S"], cfg["A"], cfg["G"], cfg["T"], cfg["P"]
    M, te = cfg.get("M", 1), cfg["te"]
    N, W = P, (2 * S + 1) * G + 2
    noise = CS.rollout_noise(seed, 0, N, T, S)
    init, sol, out, tr = _run(pl, dev, seed)
    model = np.floor(noise["u_model"].astype(np.float64) * M).astype(np.int64)
    st64 = [CS.Statement.of(m, F64) for m in pl.mem_net_list]
    st32 = [CS.Statement.of(m, F32) for m in pl.mem_net_list]
    pick = torch.from_numpy(model)
    assert torch.equal(tr[0, :, :S], init.expand(N, S))
    left_out = decisions = 0
    acc = np.zeros(N)
    alive = np.ones(N, dtype=bool)
    stop_step = np.full(N, T)
    gamma_pow = np.array([pl.gamma ** j for j in range(T)], dtype=np.float32)
    for j in range(T):
        entry, z = tr[j, :, :S], tr[j, :, S:S + W]
        idx, nt = tr[j, :, -2].long().numpy(), tr[j, :, -1].long().numpy()
        action = sol[:, j]
        z64 = torch.stack([s.z(entry, action)[0] for s in st64])[pick, torch.arange(N)]
        z32 = torch.stack([s.z(entry, action)[0] for s in st32])[pick, torch.arange(N)]
        bound = _close(z, z64, z32, f"step {j} z")
        # this package's MemoryNetwork.forward on the materialised rows: the zero-hidden quirk
        for mi, net in enumerate(pl.mem_net_list):
            rows = pick == mi
            if not rows.any():
                continue
            o = net(rlt.FeatureData(entry[None].to(dev)), rlt.FeatureData(action[None].to(dev)))
            names = ("mus", "sigmas", "logpi", "reward", "not_terminal")
            for name, ref64, t32 in zip(names, st64[mi].split(z64), st32[mi].split(z32)):
                got = getattr(o, name)[0].cpu().double()
                assert (got[rows] - ref64[rows]).abs().max().item() <= _bound(ref64[rows], t32[rows]), (name, j)
        k_ref, mk, nt_ref, mnt = CS.decide(z64.numpy(), noise["u_mix"][j], noise["u_term"][j], S, G, te)
        sure_k, sure_nt = mk > bound, mnt > bound
        assert np.array_equal(idx[sure_k], k_ref[sure_k]) and np.array_equal(nt[sure_nt], nt_ref[sure_nt]), j
        left_out += int((~sure_k).sum()) + (int((~sure_nt).sum()) if te else 0)
        decisions += N * (2 if te else 1)
        if j + 1 < T:  # next_state = fp32(mu_k + sigma_k * eps) of the traced z, within 1 ulp
            zz = z.double().numpy()
            cols = idx[:, None] * S + np.arange(S)[None, :]
            mu, ls = np.take_along_axis(zz, cols, 1), np.take_along_axis(zz, G * S + cols, 1)
            want = (mu + np.exp(ls) * noise["eps"][j].astype(np.float64)).astype(np.float32)
            got = tr[j + 1, :, :S].numpy()
            assert np.all(np.abs(got.astype(np.float64) - want) <= np.spacing(np.abs(want))), j
        term = (z[:, -2].numpy() * gamma_pow[j]).astype(np.float32)  # the fp32 product
        acc = np.where(alive, acc + term.astype(np.float64), acc)
        stop_step = np.where(alive & (nt == 0), j, stop_step)
        alive &= nt != 0
    assert np.array_equal(out.numpy(), acc), "the accumulated reward is the double sum of the traced fp32 terms"
    assert left_out <= 0.01 * decisions, (left_out, decisions)
    return stop_step


@pytest.mark.parametrize("name", list(SHAPES))
def test_rollout_against_the_float64_statement(backend, name):
    cfg = SHAPES[name]
    pl = _planner(backend.device, **cfg)
    stop = _check_rollout(pl, backend.device, cfg, SEED)
    if cfg.get("nt_bias") is not None and cfg["T"] >= 4 and cfg["P"] >= 31:  # (a midway stop needs steps to be midway of)
        T = cfg["T"]
        assert (stop == 0).any() and ((stop > 0) & (stop < T - 1)).any() and (stop == T).any(), np.bincount(stop, minlength=T + 1)


def test_a_rollout_that_carried_the_hidden_state_would_not_pass(backend):
    """two layers, W_hh scaled up: the float64 statement WITH the hidden state carried from step to step leaves the bound from
    the second step on, the zero-state statement stays inside it"""
    cfg = dict(H=8, L=2, S=4, A=3, G=3, P=33, T=3, te=False, w_hh_scale=4.0)
    pl = _planner(backend.device, **cfg)
    init, sol, out, tr = _run(pl, backend.device, SEED)
    S, W = cfg["S"], (2 * cfg["S"] + 1) * cfg["G"] + 2
    s64, s32 = CS.Statement.of(pl.mem_net_list[0], F64), CS.Statement.of(pl.mem_net_list[0], F32)
    hidden = None
    worst = 0.0
    for j in range(cfg["T"]):
        entry, z = tr[j, :, :S], tr[j, :, S:S + W]
        z64, _ = s64.z(entry, sol[:, j])
        bound = _close(z, z64, s32.z(entry, sol[:, j])[0], f"zero state, step {j}")
        carried, hidden = s64.z(entry, sol[:, j], hidden)
        if j > 0:
            worst = max(worst, (z.double() - carried).abs().max().item() / bound)
    assert worst > 100.0, worst


def test_nan_weight_reaches_its_own_trajectories_only(backend):
    cfg = dict(H=8, L=2, S=4, A=3, G=3, P=40, T=3, M=2, te=True)
    pl = _planner(backend.device, **cfg)
    with torch.no_grad():
        pl.mem_net_list[1].mdnrnn.gmm_linear.bias[-2] = float("nan")
    _, _, out, _ = _run(pl, backend.device, SEED, trace=False)
    model = np.floor(CS.rollout_noise(SEED, 0, cfg["P"], cfg["T"], cfg["S"])["u_model"].astype(np.float64) * 2).astype(int)
    assert 0 < model.sum() < cfg["P"]
    assert np.array_equal(np.isnan(out.numpy()), model == 1)


def test_placement_invariance_and_the_two_noise_sources(backend):
    """M = 3 models of which one draws no trajectory; permuted solutions and a permuted grouping keep every solution's bits;
    in-kernel noise, rg_cem_fill_noise's buffers and the numpy restatement give the same bits; so do two runs"""
    dev = backend.device
    cfg = dict(H=8, L=2, S=4, A=3, G=3, P=70, T=4, M=3, te=True, nt_bias=1.5)
    pl = _planner(dev, **cfg)
    P, T, S, N = cfg["P"], cfg["T"], cfg["S"], cfg["P"]
    ref = CS.rollout_noise(SEED, 0, N, T, S)
    ref["u_model"] = (ref["u_model"] * (2.0 / 3.0)).astype(np.float32)  # nobody draws model 2
    filled = dict(u_model=torch.empty(N, dtype=F32, device=dev), u_mix=torch.empty(T, N, dtype=F32, device=dev),
                  eps=torch.empty(T, N, S, dtype=F32, device=dev), u_term=torch.empty(T, N, dtype=F32, device=dev))
    ops.cem_fill_noise(SEED, 0, filled["u_model"], filled["u_mix"], filled["eps"], filled["u_term"])
    for k in ("u_mix", "u_term"):
        assert np.array_equal(filled[k].cpu().numpy(), ref[k]), k
    init, sol, base, _ = _run(pl, dev, SEED, trace=False)
    _, _, again, _ = _run(pl, dev, SEED, trace=False)
    assert torch.equal(base.view(torch.int64), again.view(torch.int64))
    _, _, buffered, _ = _run(pl, dev, SEED, trace=False, noise=filled)
    assert torch.equal(base.view(torch.int64), buffered.view(torch.int64))
    # explicit noise with an idle model, then the same under a permutation of the solutions and of the tiles' rows
    noise = dict(filled, u_model=torch.from_numpy(ref["u_model"]).to(dev))
    _, _, plain, _ = _run(pl, dev, SEED, trace=False, noise=noise)
    tiles = ops.cem_rollout_tiles(N, 3)
    rowmap, tile_model = torch.empty(tiles * 32, dtype=I32, device=dev), torch.empty(tiles, dtype=I32, device=dev)
    ops.cem_group(noise["u_model"], SEED, 0, N, 3, None, rowmap, tile_model)
    tm = tile_model.cpu().numpy()
    assert 2 not in tm and (tm == -1).any() and {0, 1} <= set(tm.tolist())
    g = np.random.default_rng(5)
    perm = g.permutation(P)
    inv = np.argsort(perm)
    noise_p = {k: v.index_select(v.dim() - 1 if k != "eps" else 1, torch.from_numpy(perm).to(dev)).contiguous() for k, v in noise.items()}
    _, _, permuted, _ = _run(pl, dev, SEED, trace=False, noise=noise_p, sol=sol[perm])
    assert torch.equal(permuted[inv].view(torch.int64), plain.view(torch.int64))
    rm = rowmap.cpu().numpy().reshape(tiles, 32)
    order = g.permutation(tiles)
    rm2 = np.stack([g.permutation(rm[t]) for t in order])
    _, _, regrouped, _ = _run(pl, dev, SEED, trace=False, noise=noise,
                              grouping=(torch.from_numpy(np.ascontiguousarray(rm2.reshape(-1))).to(dev),
                                        torch.from_numpy(np.ascontiguousarray(tm[order])).to(dev)))
    assert torch.equal(regrouped.view(torch.int64), plain.view(torch.int64))


def test_noise_recipe(backend):
    dev = backend.device
    N, T, S = 37, 3, 5
    ref = CS.rollout_noise(9, 2, N, T, S)
    got = dict(u_model=torch.empty(N, dtype=F32, device=dev), u_mix=torch.empty(T, N, dtype=F32, device=dev),
               eps=torch.empty(T, N, S, dtype=F32, device=dev), u_term=torch.empty(T, N, dtype=F32, device=dev))
    ops.cem_fill_noise(9, 2, got["u_model"], got["u_mix"], got["eps"], got["u_term"])
    for k in ("u_model", "u_mix", "u_term"):
        assert np.array_equal(got[k].cpu().numpy(), ref[k]), k
    e = got["eps"].cpu().numpy()
    assert np.all(np.abs(e.astype(np.float64) - ref["eps"]) <= 4 * np.spacing(np.abs(ref["eps"])))
    P, Tn, A = 300, 4, 3
    acts = torch.empty(P, Tn, dtype=I32, device=dev)
    ops.cem_sample_discrete(9, 0, A, acts)
    assert np.array_equal(acts.cpu().numpy(), CS.discrete_actions(9, 0, P, Tn, A))
    assert set(acts.cpu().numpy().ravel().tolist()) == set(range(A))


def _sample(dev, P, D, seed, iteration=0):
    ps = torch.tensor([0.0] * D + [1.0] * D + [0.0, 0.0], dtype=F64, device=dev)  # mean 0, var 1, bounds +-4: cv = 1
    lo, hi = torch.full((D,), -4.0, dtype=F64, device=dev), torch.full((D,), 4.0, dtype=F64, device=dev)
    sol, sol32 = torch.empty(P, D, dtype=F64, device=dev), torch.empty(P, D, dtype=F32, device=dev)
    ops.cem_sample(ps, lo, hi, seed, iteration, sol, sol32)
    return sol.cpu().numpy(), sol32.cpu().numpy()


def test_truncated_normal_draws(backend):
    P, D = 256, 256  # 2^16 draws
    tn, tn32 = _sample(backend.device, P, D, 21)
    ref = CS.truncated_normal(21, 0, P, D)
    assert np.all(np.abs(tn - ref) <= 4 * np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64))
    assert np.array_equal(tn32, tn.astype(np.float32))
    assert tn.min() >= -2.0 and tn.max() <= 2.0
    # the standard normal truncated to [-2, 2]: mean 0, variance 1 - 4 phi(2) / (2 Phi(2) - 1), fourth moment by quadrature
    x = np.linspace(-2, 2, 400001)
    w = np.exp(-x * x / 2)
    trapezoid = getattr(np, "trapezoid", None) or np.trapz
    w /= trapezoid(w, x)
    var, m4 = trapezoid(w * x ** 2, x), trapezoid(w * x ** 4, x)
    assert abs(var - 0.774) < 1e-3
    n = tn.size
    assert abs(tn.mean()) <= 4 * np.sqrt(var / n)
    assert abs(tn.var() - var) <= 4 * np.sqrt((m4 - var ** 2) / n)


def test_sample_applies_the_constrained_variance(backend):
    dev = backend.device
    P, D = 5, 6
    mean = np.array([0.0, 0.9, -0.5, 0.0, 1.0, 0.3])
    var = np.array([0.25, 0.25, 1e-4, 4.0, 0.25, np.nan])
    lo, hi = -np.ones(D), np.ones(D)
    tn = np.random.default_rng(0).uniform(-2, 2, size=(P, D))
    ps = torch.from_numpy(np.concatenate([mean, var, [0, 0]])).to(dev)
    sol, sol32 = torch.empty(P, D, dtype=F64, device=dev), torch.empty(P, D, dtype=F32, device=dev)
    ops.cem_sample(ps, torch.from_numpy(lo).to(dev), torch.from_numpy(hi).to(dev), 0, 0, sol, sol32, tn=torch.from_numpy(tn).to(dev))
    cv = np.minimum(np.minimum(((mean - lo) / 2) ** 2, ((hi - mean) / 2) ** 2), var)
    want = tn * np.sqrt(cv) + mean
    assert np.array_equal(sol.cpu().numpy(), want, equal_nan=True)
    assert np.array_equal(sol32.cpu().numpy(), want.astype(np.float32), equal_nan=True)


# ---- refit and tally ----------------------------------------------------------------------------------------------------
def _refit_numpy(rewards, sol, ne, alpha, eps, mean, var):
    elites_idx = np.sort(np.argsort(rewards, kind="stable")[-ne:])  # numpy's elites, summed in solution-index order
    el = sol[elites_idx]
    new_mean = np.add.reduce(el, axis=0) / ne
    new_var = np.add.reduce((el - new_mean) ** 2, axis=0) / ne
    mean = alpha * mean + (1 - alpha) * new_mean
    var = alpha * var + (1 - alpha) * new_var
    return elites_idx, mean, var, bool(np.max(var) <= eps)


def _refit(dev, rewards, sol, ne, alpha, eps, mean, var, state=(0.0, 0.0)):
    P, D = sol.shape
    ps = torch.from_numpy(np.concatenate([mean, var, state])).to(dev)
    flags = torch.zeros(P, dtype=I32, device=dev)
    ops.cem_refit(torch.from_numpy(rewards).to(dev), torch.from_numpy(sol).to(dev), ne, alpha, eps, ps, flags)
    return ps.cpu().numpy(), flags.cpu().numpy()


@pytest.mark.parametrize("P,ne", [(1, 1), (33, 1), (33, 33), (33, 8), (1025, 100)])
@pytest.mark.parametrize("integers", [True, False])
def test_refit_against_numpy(backend, P, ne, integers):
    g = np.random.default_rng(P * 7 + ne)
    D = 7
    sol = g.integers(-8, 9, size=(P, D)).astype(np.float64) if integers else g.normal(size=(P, D))
    rewards = np.round(g.normal(size=P), 1)  # rounded: ties, also at the elite boundary
    if P > 2:
        rewards[g.integers(P)] = np.nan  # ranks above every number: an elite
        rewards[[0, P - 1]] = np.sort(rewards[~np.isnan(rewards)])[-min(ne, P - 2)]  # a tie exactly at the boundary
    mean, var = g.normal(size=D), g.uniform(0.5, 1.5, size=D)
    alpha = 0.25 if not integers else 0.5
    idx, m, v, done = _refit_numpy(rewards, sol, ne, alpha, 1e-3, mean, var)
    ps, flags = _refit(backend.device, rewards, sol, ne, alpha, 1e-3, mean, var)
    assert np.array_equal(np.flatnonzero(flags), idx)
    if P > 2:
        assert flags[np.flatnonzero(np.isnan(rewards))[0]] == 1
    tol = 0.0 if integers else 4 * np.spacing(np.maximum(np.abs(m), np.abs(v)))  # small integers: the arithmetic is exact
    assert np.all(np.abs(ps[:D] - m) <= tol) and np.all(np.abs(ps[D:2 * D] - v) <= tol)
    assert ps[2 * D] == float(done) == 0.0 and ps[2 * D + 1] == 1.0


def test_refit_is_exact_on_small_integers_and_ties_go_to_the_higher_index(backend):
    sol = np.array([[1.0, -2.0], [3.0, 4.0], [5.0, 0.0], [7.0, 2.0], [-1.0, 6.0]])
    rewards = np.array([1.0, 2.0, 2.0, 0.5, 2.0])  # two elites: indices 2 and 4 (of the equal rewards the higher indices)
    mean, var = np.array([1.0, 2.0]), np.array([4.0, 8.0])
    idx, m, v, _ = _refit_numpy(rewards, sol, 2, 0.5, 1e-3, mean, var)
    assert idx.tolist() == [2, 4]
    ps, flags = _refit(backend.device, rewards, sol, 2, 0.5, 1e-3, mean, var)
    assert flags.tolist() == [0, 0, 1, 0, 1]
    assert np.array_equal(ps[:4], np.concatenate([m, v]))


def test_refit_done_flag_at_equality_and_later_calls_do_nothing(backend):
    dev = backend.device
    sol = np.array([[1.0, 1.0], [3.0, 1.0], [9.0, 9.0]])
    rewards = np.array([2.0, 3.0, -1.0])  # elites 0 and 1: new_var = [1, 0]
    mean, var = np.zeros(2), np.array([1.0, 0.0])
    # alpha = 0.5: var = [1, 0]; epsilon = 1.0 = max(var) exactly
    ps, _ = _refit(dev, rewards, sol, 2, 0.5, 1.0, mean, var)
    assert ps[2:4].tolist() == [1.0, 0.0] and ps[4] == 1.0 and ps[5] == 1.0
    just_below = np.nextafter(1.0, 0.0)
    ps2, _ = _refit(dev, rewards, sol, 2, 0.5, just_below, mean, var)
    assert ps2[4] == 0.0 and ps2[5] == 1.0
    # with done set nothing moves: refit, sample, group and rollout all return at once
    ps3, flags = _refit(dev, rewards, sol, 2, 0.5, 1.0, ps[:2], ps[2:4], state=(1.0, 1.0))
    assert np.array_equal(ps3, ps) and not flags.any()
    pst = torch.from_numpy(ps).to(dev)
    s64, s32 = torch.full((3, 2), -5.0, dtype=F64, device=dev), torch.full((3, 2), -5.0, dtype=F32, device=dev)
    ops.cem_sample(pst, torch.zeros(2, dtype=F64, device=dev), torch.ones(2, dtype=F64, device=dev), 1, 1, s64, s32)
    assert (s64 == -5.0).all() and (s32 == -5.0).all()
    pl = _planner(dev, H=8, L=1, S=2, A=2, G=2, P=3, T=1)
    out = torch.full((3,), -7.0, dtype=F64, device=dev)
    pl._rollout(torch.zeros(2, device=dev), s32.view(3, 1, 2), None, out, seed=1, done=pst[4:])
    assert (out == -7.0).all()


def test_tally_against_numpy(backend):
    dev = backend.device
    g = np.random.default_rng(3)
    P, T, A = 200, 3, 5
    actions = g.integers(0, A - 1, size=(P, T)).astype(np.int32)  # the last first action is never drawn
    rewards = g.normal(size=P)
    out = torch.empty(3 * A + 1, dtype=F64, device=dev)
    ops.cem_tally(torch.from_numpy(actions).to(dev), torch.from_numpy(rewards).to(dev), A, out)
    out = out.cpu().numpy()
    count, total = np.zeros(A), np.zeros(A)
    for a, r in zip(actions[:, 0], rewards):
        count[a] += 1
        total[a] += r
    with np.errstate(invalid="ignore"):
        q = total / count
    assert np.array_equal(out[:A], count) and np.array_equal(out[A:2 * A], total) and np.array_equal(out[2 * A:3 * A], q, equal_nan=True)
    assert np.isnan(out[3 * A - 1]) and out[3 * A] == np.nanargmax(q)
    all_nan = torch.empty(3 * A + 1, dtype=F64, device=dev)
    ops.cem_tally(torch.from_numpy(actions).to(dev), torch.full((P,), float("nan"), dtype=F64, device=dev), A, all_nan)
    assert all_nan.cpu().numpy()[3 * A] == -1


def test_ensemble_mean_is_the_index_order_double_mean(backend):
    """DEPARTURE from the reference, which raises for ensemble_population_size > 1"""
    dev = backend.device
    cfg = dict(H=8, L=2, S=4, A=3, G=3, P=21, T=4, E=3, te=True, nt_bias=1.5)
    pl = _planner(dev, **cfg)
    P, E, T, S = 21, 3, 4, 4
    init, sol, out, tr = _run(pl, dev, SEED)
    assert tr.shape[1] == P * E
    gamma_pow = np.array([pl.gamma ** j for j in range(T)], dtype=np.float32)
    acc, alive = np.zeros(P * E), np.ones(P * E, dtype=bool)
    for j in range(T):
        term = (tr[j, :, -4].numpy() * gamma_pow[j]).astype(np.float32)
        acc = np.where(alive, acc + term.astype(np.float64), acc)
        alive &= tr[j, :, -1].numpy() != 0
    want = np.array([(acc[p * E] + acc[p * E + 1] + acc[p * E + 2]) / 3.0 for p in range(P)])
    assert np.array_equal(out.numpy(), want)
    # a solution's E trajectories share its actions: the entry state of step 0 and the solution index n // E
    single = _planner(dev, **dict(cfg, E=1, P=P * E))
    _, _, flat, _ = _run(single, dev, SEED, sol=sol.repeat_interleave(E, dim=0))
    assert np.array_equal(flat.numpy(), acc)
