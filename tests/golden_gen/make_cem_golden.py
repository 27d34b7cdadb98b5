"""TEST INFRASTRUCTURE.  Generates tests/golden/cem/*.npz and tests/golden/reference_records/cem_signatures.json by running the
UNMODIFIED reference CEMPlannerNetwork (through oracle/stubs.py) on seeded reference MemoryNetworks.  Run where the reference
tree and scipy are present:

    python tests/golden_gen/make_cem_golden.py            (writes the fixtures and the signature record)
    python tests/golden_gen/make_cem_golden.py --check    (regenerates them and compares with the committed files)

For the duration of the planner's call the library's draw functions are replaced by recording stand-ins (no line of the
reference is copied or changed): np.random.randint, scipy.stats.truncnorm(...).rvs, random.choices and the sample() of
Categorical, Normal and Bernoulli as cem_planner.py names them.  A stand-in draws uniforms or standard normals from one
seeded numpy generator, applies the rule include/reagent_hip.h states (floor(u * count); the count of cumulative
probabilities <= u; loc + scale * eps; u < p; rejection into [-2, 2]) and stores the draw, laid out as the kernels' explicit
noise: u_model [N], u_mix / u_term [T, N], eps [T, N, S], tn [P, D], action indices [P, T].  Steps a stopped trajectory never
reached hold 0.5 and zeros.  What a planner's locals hold is recorded where it passes through a method: the solutions and
their accumulated rewards of every iteration (acc_rewards_of_all_solutions, wrapped, not changed) and the mean and var every
iteration starts from (constrained_variance).  Data only.

Layout: config_json; param_<m>_<i> (member m's parameters in state_dict order) and names_json; state; per iteration k
it<k>_tn, it<k>_u_model, it<k>_u_mix, it<k>_u_term, it<k>_eps, it<k>_solutions, it<k>_rewards, it<k>_mean, it<k>_var (the two the
iteration starts from); discrete: actions; result (and result_idx), with the dtype the reference returned.

The generator ASSERTS what makes a replay decidable and refuses to write otherwise: every recorded sampling decision has a
float64 margin above MARGIN, the reward gap at the elite boundary of every iteration and the gap between the best and the
second-best first-action mean are above 10 * ROLLOUT_BOUND."""
import json
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden")
OUT = os.path.join(GOLDEN, "cem")
SIGNATURES = os.path.join(GOLDEN, "reference_records", "cem_signatures.json")
ROLLOUT_BOUND = 1e-4  # the suite's replay tolerance, relative to the largest accumulated reward
MARGIN = 1e-4  # of a sampling decision, in probability

CASES = {
    # discrete: A = 2, two layers, terminals effective, gamma 0.9
    "cem_discrete": dict(discrete=True, M=1, S=3, A=2, H=8, L=2, G=2, P=40, E=1, T=4, iters=1, elites=1, te=True, gamma=0.9,
                         alpha=0.25, epsilon=0.001, seed=5, nt_bias=1.5),
    # continuous: two world models, G = 3, terminals not effective, 4 iterations, 8 elites
    "cem_continuous_two_models": dict(discrete=False, M=2, S=3, A=2, H=8, L=1, G=3, P=32, E=1, T=3, iters=4, elites=8, te=False,
                                      gamma=0.95, alpha=0.25, epsilon=1e-9, seed=7, nt_bias=None),
    # continuous: terminals effective, an epsilon that stops it after the second iteration
    "cem_continuous_early_stop": dict(discrete=False, M=1, S=3, A=2, H=8, L=2, G=2, P=32, E=1, T=4, iters=5, elites=8, te=True,
                                      gamma=0.9, alpha=0.25, epsilon=0.22, seed=18, nt_bias=2.0),
}


class Recorder:
    def __init__(self, c):
        self.c = c
        self.g = np.random.default_rng(c["seed"] + 1000)
        self.iterations = []
        self.cur = None
        self.n = -1
        self.j = 0
        self.min_margin = np.inf
        self.actions = None

    def begin_iteration(self):
        c = self.c
        N, T, S = c["P"] * c["E"], c["T"], c["S"]
        self.cur = dict(u_model=np.full(N, 0.5, np.float32), u_mix=np.full((T, N), 0.5, np.float32),
                        u_term=np.full((T, N), 0.5, np.float32), eps=np.zeros((T, N, S), np.float32))
        self.iterations.append(self.cur)
        self.n = -1

    def uniform(self):
        return np.float32(self.g.integers(0, 1 << 24) * 2.0 ** -24)

    # ---- the stand-ins -------------------------------------------------------------------------------------------------
    def randint(self, low, high=None, *a, **k):
        assert low == 0 and high == self.c["M"] and not a and not k
        u = self.uniform()
        self.n += 1
        self.j = 0
        self.cur["u_model"][self.n] = u
        return int(np.floor(np.float64(u) * high))

    def truncnorm(self, lo, hi, loc, scale):
        rec = self
        assert (lo, hi) == (-2, 2) and not np.any(loc) and np.all(scale == 1)

        class Sampler:
            def rvs(self, size):
                out = np.empty(size)
                for i in np.ndindex(*size):
                    z = rec.g.standard_normal()
                    while abs(z) > 2.0:
                        z = rec.g.standard_normal()
                    out[i] = z
                rec.begin_iteration()
                rec.cur["tn"] = out.copy()
                return out

        return Sampler()

    def choices(self, population, k):
        c = self.c
        u = np.array([[self.uniform() for _ in range(c["T"])] for _ in range(k)])
        self.actions = np.floor(u.astype(np.float64) * c["A"]).astype(np.int32)
        self.begin_iteration()
        lookup = {tuple(s): s for s in population}
        return [lookup[tuple(int(a) for a in row)] for row in self.actions]

    def categorical(self):
        rec = self

        class Categorical:
            def __init__(self, probs):
                self.probs = probs

            def sample(self):
                p = self.probs.double().numpy()
                cdf = np.cumsum(p / p.sum())
                u = rec.uniform()
                rec.cur["u_mix"][rec.j, rec.n] = u
                if len(cdf) > 1:
                    rec.min_margin = min(rec.min_margin, float(np.abs(cdf[:-1] - np.float64(u)).min()))
                return torch.tensor(min(int((cdf <= np.float64(u)).sum()), len(cdf) - 1))

        return Categorical

    def normal(self):
        rec = self

        class Normal:
            def __init__(self, loc, scale):
                self.loc, self.scale = loc, scale

            def sample(self):
                eps = rec.g.standard_normal(self.loc.shape[0]).astype(np.float32)
                rec.cur["eps"][rec.j, rec.n] = eps
                if not rec.c["te"]:
                    rec.j += 1  # (no Bernoulli draw closes the step)
                return self.loc + self.scale * torch.from_numpy(eps)

        return Normal

    def bernoulli(self):
        rec = self

        class Bernoulli:
            def __init__(self, probs):
                self.probs = probs

            def sample(self):
                u = rec.uniform()
                rec.cur["u_term"][rec.j, rec.n] = u
                rec.min_margin = min(rec.min_margin, abs(float(u) - float(self.probs.double())))
                rec.j += 1
                return (torch.tensor(float(u)) < self.probs).float()

        return Bernoulli


def generate(name):
    c = CASES[name]
    from oracle import stubs

    stubs.install()
    import reagent.models.cem_planner as ref
    import scipy.stats
    from reagent.core import types as rlt
    from reagent.models.world_model import MemoryNetwork

    torch.manual_seed(c["seed"])
    nets = [MemoryNetwork(state_dim=c["S"], action_dim=c["A"], num_hiddens=c["H"], num_hidden_layers=c["L"],
                          num_gaussians=c["G"]) for _ in range(c["M"])]
    with torch.no_grad():
        for net in nets:
            net.mdnrnn.gmm_linear.weight[-2] *= 4.0  # rewards spread out: the elite boundary has a gap
            if c["nt_bias"] is not None:
                net.mdnrnn.gmm_linear.bias[-1] = c["nt_bias"]
    bounds = {} if c["discrete"] else dict(action_upper_bounds=np.array([1.0, 2.0]), action_lower_bounds=np.array([-1.0, -0.5]))
    planner = ref.CEMPlannerNetwork(mem_net_list=nets, cem_num_iterations=c["iters"], cem_population_size=c["P"],
                                    ensemble_population_size=c["E"], num_elites=c["elites"], plan_horizon_length=c["T"],
                                    state_dim=c["S"], action_dim=c["A"], discrete_action=c["discrete"], terminal_effective=c["te"],
                                    gamma=c["gamma"], alpha=c["alpha"], epsilon=c["epsilon"], **bounds)
    state = torch.randn(1, c["S"])
    rec = Recorder(c)
    inner_rewards, inner_cv = planner.acc_rewards_of_all_solutions, planner.constrained_variance
    starts = []

    def rewards(st, solutions):
        out = inner_rewards(st, solutions)
        rec.cur["solutions"], rec.cur["rewards"] = solutions.numpy().copy(), np.asarray(out, dtype=np.float64).copy()
        return out

    def cv(mean, var):
        starts.append((np.array(mean, dtype=np.float64), np.array(var, dtype=np.float64)))
        return inner_cv(mean, var)

    planner.acc_rewards_of_all_solutions, planner.constrained_variance = rewards, cv
    saved = (np.random.randint, scipy.stats.truncnorm, random.choices, ref.Categorical, ref.Normal, ref.Bernoulli)
    np.random.randint, scipy.stats.truncnorm, random.choices = rec.randint, rec.truncnorm, rec.choices
    ref.Categorical, ref.Normal, ref.Bernoulli = rec.categorical(), rec.normal(), rec.bernoulli()
    try:
        import warnings

        with warnings.catch_warnings():
            warnings.simplefilter("ignore", DeprecationWarning)  # numpy's, for the length-1 array in a scalar slot (:186)
            result = planner(rlt.FeatureData(state))
    finally:
        np.random.randint, scipy.stats.truncnorm, random.choices, ref.Categorical, ref.Normal, ref.Bernoulli = saved

    arrays = {"config_json": np.array(json.dumps(c)), "state": state.numpy()}
    names = [k for k, _ in nets[0].state_dict().items()]
    arrays["names_json"] = np.array(json.dumps(names))
    for m, net in enumerate(nets):
        for i, (_, v) in enumerate(net.state_dict().items()):
            arrays[f"param_{m}_{i}"] = v.detach().numpy().copy()
    assert rec.min_margin > MARGIN, (name, "a sampling decision is too close to call", rec.min_margin)
    for k, it in enumerate(rec.iterations):
        r = it["rewards"]
        scale = np.abs(r).max()
        if c["discrete"]:
            first = rec.actions[:, 0]
            means = np.sort([r[first == a].mean() for a in range(c["A"])])
            assert means[-1] - means[-2] > 10 * ROLLOUT_BOUND * scale, (name, means)
        else:
            s = np.sort(r)
            assert s[-c["elites"]] - s[-c["elites"] - 1] > 10 * ROLLOUT_BOUND * scale, (name, k, "the elite boundary is too close")
            it["mean"], it["var"] = starts[k]
            it["solutions"] = it["solutions"].reshape(c["P"], -1)
        for key, v in it.items():
            arrays[f"it{k}_{key}"] = v
    arrays["iterations"] = np.array(len(rec.iterations))
    if c["discrete"]:
        arrays["actions"] = rec.actions
        arrays["result_idx"] = np.asarray(result[0])
        arrays["result"] = result[1].numpy()
    else:
        arrays["result"] = result.numpy()
    return arrays


def signatures():
    """the reference's signatures as tests/test_reference_signatures.py reduces them (name, kind, default).  CEMPolicy is not
    among them: its module (model_managers/model_based/cross_entropy_method.py) imports the model managers, which need
    packages that are not here; tests/test_cem_trainer.py states its two signatures itself."""
    from oracle import stubs

    stubs.install()
    ns = {}
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_reference_signatures import _PARAMS

    exec(_PARAMS, ns)
    return ns["surface"]([
        ("reagent.core.parameters.CEMTrainerParameters", ["__init__"]),
        ("reagent.models.cem_planner.CEMPlannerNetwork",
         ["__init__", "forward", "acc_rewards_of_one_solution", "acc_rewards_of_all_solutions", "sample_reward_next_state_terminal",
          "constrained_variance", "continuous_planning", "discrete_planning"]),
        ("reagent.training.cem_trainer.CEMTrainer", ["__init__", "configure_optimizers", "train_step_gen"]),
    ])


def main():
    check = "--check" in sys.argv[1:]
    os.makedirs(OUT, exist_ok=True)
    failed = []
    for name in CASES:
        arrays = generate(name)
        path = os.path.join(OUT, name + ".npz")
        if check:
            with np.load(path) as old:
                same = sorted(old.files) == sorted(arrays) and all(
                    old[k].dtype == arrays[k].dtype and np.array_equal(old[k], arrays[k]) for k in arrays)
            print(name, "identical" if same else "DIFFERS")
            if not same:
                failed.append(name)
        else:
            np.savez_compressed(path, **arrays)
            print("wrote", name, os.path.getsize(path) // 1024, "KiB", "iterations", int(arrays["iterations"]))
    rec = signatures()
    if check:
        same = json.load(open(SIGNATURES)) == json.loads(json.dumps(rec))
        print("cem_signatures.json", "identical" if same else "DIFFERS")
        if not same:
            failed.append("cem_signatures.json")
        sys.exit(1 if failed else 0)
    with open(SIGNATURES, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
    print("wrote cem_signatures.json")


if __name__ == "__main__":
    main()
