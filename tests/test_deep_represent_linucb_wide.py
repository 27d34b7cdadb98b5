"""DeepRepresentLinUCBTrainer where the last MLP layer is 128 or 256 wide (d = 129, 257): the ridge solve of every training
step is rg_linucb_solve_blocked on the device-resident buffers, never the parent's host path.  On the interpreter and, under
`-m gpu`, on the MI355X.  u = 2^-24.

The inverse after two steps and an epoch end is held, relative to the largest entry, to 4 e_ref + d 2 u of the float64
inverse of the folded averages, e_ref being torch's own fp32 inverse's distance from it (the rule
tests/test_deep_represent_linucb_trainer.py applies at d = 129).
"""
import pytest
import torch

U = 2.0 ** -24
MARGIN = 4.0
CONFIG = dict(F=9, activations=["relu", "linear"], lr=1e-3, weight_decay=0.0, loss_type="mse", l2_reg_lambda=1.0, gamma=0.9,
              model=dict(output_activation="linear", ucb_alpha=1.0, use_batch_norm=False, normalize_output=False,
                         use_layer_norm=False, use_skip_connections=False, nn_e2e=False))
B, ARMS = 600, 3


def _trainer(width, dev, seed=5, **over):
    from reagent_amd.gym.policies import Policy
    from reagent_amd.models import DeepRepresentLinearRegressionUCB
    from reagent_amd.training import DeepRepresentLinUCBTrainer

    torch.manual_seed(seed)
    c = CONFIG
    kw = dict(dict(c["model"], l2_reg_lambda=c["l2_reg_lambda"], gamma=c["gamma"]), **over)
    scorer = DeepRepresentLinearRegressionUCB(c["F"], [8, width], list(c["activations"]), **kw).to(dev)
    tr = DeepRepresentLinUCBTrainer(Policy(scorer=scorer, sampler=None), lr=c["lr"], weight_decay=c["weight_decay"],
                                    loss_type=c["loss_type"])
    return tr, scorer


def _batches(dev, n=2, seed=6):
    from reagent_amd.core.types import CBInput

    gen = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        x = torch.randn(B, ARMS, CONFIG["F"], generator=gen).to(dev)
        out.append(CBInput(context_arm_features=x, action=torch.randint(0, ARMS, (B, 1), generator=gen).to(dev),
                           reward=torch.randn(B, 1, generator=gen).to(dev)))
    return out


def _rel(got, ref):
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item()


def _forbid_the_host_path(monkeypatch):
    from reagent_amd.models.linear_regression import LinearRegressionUCB

    def host(self):
        pytest.fail(f"the parent's host path was taken at d = {self.input_dim}")

    monkeypatch.setattr(LinearRegressionUCB, "_calculate_coefs", host)


@pytest.mark.parametrize("width", [128, 256])
def test_every_step_solves_on_the_device_and_matches_the_float64_inverse(backend, monkeypatch, width):
    from reagent_amd import ops

    dev, d = backend.device, width + 1
    tr, scorer = _trainer(width, dev)
    assert scorer.input_dim == d and scorer._solve_workspace.numel() == 0
    _forbid_the_host_path(monkeypatch)
    monkeypatch.setattr(ops, "linucb_solve", lambda *a, **k: pytest.fail(f"rg_linucb_solve was called at d = {d}"))
    calls = []
    blocked = ops.linucb_solve_blocked
    monkeypatch.setattr(ops, "linucb_solve_blocked", lambda *a: (calls.append(a[-1].data_ptr()), blocked(*a))[1])
    for batch in _batches(dev):
        tr.train_step_native(batch)
        assert scorer._solve_unchecked  # the step itself reads nothing back
    tr.on_train_epoch_end()
    assert len(calls) == 3 and len(set(calls)) == 1  # one solve a step and one at the epoch's end, one workspace
    assert int(scorer._solve_status.item()) == 0 and not scorer._solve_unchecked and not scorer._coefs_dirty
    c = CONFIG
    eye = torch.eye(d, dtype=torch.float64)
    A, b, sw = scorer.avg_A.cpu().double(), scorer.avg_b.cpu().double(), scorer.sum_weight.cpu().double() / c["gamma"]
    inv = torch.linalg.inv(A + c["l2_reg_lambda"] * eye / sw)
    e_ref = _rel(torch.linalg.inv((A + c["l2_reg_lambda"] * eye / sw).float()), inv)
    err = _rel(scorer.inv_avg_A, inv)
    print(f"d = {d}: inverse {err:.3e} of {MARGIN * e_ref + d * 2 * U:.3e} (torch fp32 {e_ref:.3e})")
    assert err <= MARGIN * e_ref + d * 2 * U
    assert torch.equal(scorer.inv_avg_A, scorer.inv_avg_A.t())
    assert scorer.num_obs.item() == 2 * B and scorer.cur_num_obs.item() == 0
    assert not scorer.cur_avg_A.any() and not scorer.cur_avg_b.any() and scorer.cur_sum_weight.item() == 0.0
    assert torch.equal(scorer.coefs_valid_for_avg_A, scorer.avg_A)


def test_the_lightning_loop_and_the_native_step_give_the_same_bits(backend, monkeypatch):
    dev = backend.device
    _forbid_the_host_path(monkeypatch)
    states = []
    for native in (False, True):
        tr, scorer = _trainer(128, dev)
        opt = tr.native_optimizers()[0] if native else tr.configure_optimizers()
        losses = []
        for i, batch in enumerate(_batches(dev)):
            if native:
                loss = tr.train_step_native(batch)
            else:
                opt.zero_grad()
                loss = tr.training_step(batch, i)
                loss.backward()
                opt.step()
            losses.append(loss.detach().cpu().reshape(1).clone())
        tr.on_train_epoch_end()
        states.append((losses, {k: v.detach().cpu().clone() for k, v in scorer.state_dict().items()}))
    (la, sa), (lb, sb) = states
    assert all(torch.equal(x, y) for x, y in zip(la, lb))
    assert set(sa) == set(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    assert sa["inv_avg_A"].abs().max() > 0 and sa["num_obs"].item() == 2 * B


def test_the_workspace_follows_the_module_and_stays_out_of_the_state_dict(backend):
    dev = backend.device
    narrow = _trainer(5, dev)[1]
    tr, scorer = _trainer(128, dev)
    keys = set(scorer.state_dict())
    # the reference's keys: what a narrow model has, nothing for the workspace or the status flag
    assert keys == set(narrow.state_dict()) and not any("workspace" in k or "status" in k for k in keys)
    tr.train_step_native(_batches(dev, n=1)[0])
    need = 3 * 160 * 160 * 4
    assert scorer._solve_workspace.numel() == need and scorer._solve_workspace.device.type == torch.device(dev).type
    assert set(scorer.state_dict()) == keys
    scorer.cpu()
    assert scorer._solve_workspace.device.type == "cpu" and scorer._solve_workspace.numel() == need
    scorer.to(dev)
    assert scorer._solve_workspace.device.type == torch.device(dev).type and scorer._solve_status.device == scorer.avg_A.device
    kept = scorer._solve_workspace.data_ptr()
    tr.train_step_native(_batches(dev, n=1, seed=7)[0])
    tr.on_train_epoch_end()
    assert scorer._solve_workspace.data_ptr() == kept and scorer.num_obs.item() == 2 * B
    assert int(scorer._solve_status.item()) == 0 and torch.isfinite(scorer.inv_avg_A).all()
    fresh = _trainer(128, dev)[1]
    fresh.load_state_dict(scorer.state_dict(), strict=True)  # and back in: nothing missing, nothing unexpected


def test_a_failed_pivot_at_129_is_recomputed_on_the_host_once(backend):
    """the assertions of tests/test_deep_represent_linucb_trainer.py::test_a_failed_pivot_is_recomputed_on_the_host_once"""
    from reagent_amd.models.linear_regression import matrix_inv_fallback_pinv

    _, scorer = _trainer(128, backend.device, l2_reg_lambda=0.0)
    d = scorer.input_dim
    assert d == 129
    v = torch.randn(d, generator=torch.Generator().manual_seed(1))
    scorer.cur_avg_A.copy_(torch.outer(v, v))  # rank one, no regularisation: a zero pivot
    scorer.cur_sum_weight.fill_(10.0)
    scorer.mark_dirty()
    scorer._calculate_coefs()
    assert int(scorer._solve_status.item()) == 1
    scorer.check_solve_status()  # the parent's inv / pinv on the host, from the folded avg_A
    assert int(scorer._solve_status.item()) == 0 and not scorer._solve_unchecked
    assert torch.equal(scorer.avg_A.cpu(), (torch.outer(v, v) * 10.0) / (torch.tensor(10.0) + torch.tensor(1e-5)))
    want = matrix_inv_fallback_pinv(scorer.avg_A.cpu() + 0.0 * torch.eye(d) / scorer.sum_weight.cpu())
    assert torch.allclose(scorer.inv_avg_A.cpu(), want, rtol=0, atol=0, equal_nan=True)
    assert not scorer.cur_avg_A.any() and scorer.cur_sum_weight.item() == 0.0
