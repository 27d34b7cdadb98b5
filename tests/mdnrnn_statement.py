"""TEST INFRASTRUCTURE.  The world model's lines restated with torch's own operations, for any dtype: gmm_loss
(reagent/models/mdn_rnn.py:215-233), the split of gmm_linear's output (:75-92), MDNRNNTrainer.get_loss
(reagent/training/world_model/mdnrnn_trainer.py:143-177) and the model itself (nn.LSTM + nn.Linear under the reference's
parameter names).  The float64 evaluation is the yardstick of tests/test_mdn_head.py and tests/test_mdnrnn_trainer.py, the
fp32 evaluation calibrates their bounds."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F


def ulp(x):
    return float(np.spacing(np.float32(abs(float(x)))))


def close(got, ref64, torch32, what, ratios=None):
    """the self-calibrating bound of tests/test_pg_kernels.py: 4 x the fp32 torch statement's own largest error against
    float64, floored at 4 ulp (fp32) of the largest magnitude; prints the three numbers.  Where the fp32 statement itself
    overflows (log sigma = -30: its gradient is inf * 0 = NaN) it calibrates nothing and the floor alone is the bound"""
    ref64 = torch.as_tensor(ref64).detach().cpu().double()
    own = (torch.as_tensor(torch32).detach().cpu().double() - ref64).abs().max().item()
    floor = 4.0 * ulp(ref64.abs().max().item())
    bound = max(4.0 * own, floor) if np.isfinite(own) else floor
    err = (torch.as_tensor(got).detach().cpu().double() - ref64).abs().max().item()
    print(f"{what}: kernel error {err:.3e}, torch fp32 error {own:.3e}, bound {bound:.3e}, ratio {err / bound:.3f}")
    if ratios is not None:
        ratios.append(err / bound)
    assert err <= bound, (what, err, bound, own)
    return bound, own


def gmm_lines(batch, mus, sigmas, logpi, reduce=True):
    lp = logpi + torch.distributions.Normal(mus, sigmas).log_prob(batch.unsqueeze(-2)).sum(-1)
    m = lp.max(dim=-1, keepdim=True)[0]
    log_prob = m.squeeze(-1) + torch.log(torch.exp(lp - m).sum(-1))
    return -log_prob.mean() if reduce else -log_prob


def split_lines(z, G, S):
    """z [..., (2S + 1) G + 2] -> mus, sigmas, logpi, reward, not_terminal"""
    lead, st = z.shape[:-1], G * S
    return (z[..., :st].reshape(*lead, G, S), torch.exp(z[..., st:2 * st].reshape(*lead, G, S)),
            F.log_softmax(z[..., 2 * st:2 * st + G], dim=-1), z[..., -2], z[..., -1])


def head_lines(z, next_state, reward, not_terminal, G, dtype, weights=(1.0, 1.0, 1.0), divide=True, first_row=0):
    """z [N, .] fp32 -> (losses [4] = gmm, bce, mse, loss; d loss / d z; sigmas; logpi) of the reference's lines in dtype;
    weights = (next_state, not_terminal, reward)"""
    z = z.to(dtype).requires_grad_(True)
    S = next_state.shape[-1]
    mus, sigmas, logpi, rs, nts = split_lines(z, G, S)
    k = slice(first_row, None)
    gmm = gmm_lines(next_state.to(dtype)[k], mus[k], sigmas[k], logpi[k]) * weights[0]
    bce = F.binary_cross_entropy_with_logits(nts[k], not_terminal.to(dtype)[k]) * weights[1]
    mse = F.mse_loss(rs[k], reward.to(dtype)[k]) * weights[2]
    loss = gmm / (S + 2) + bce + mse if divide else gmm + bce + mse
    loss.backward()
    return torch.stack([gmm, bce, mse, loss]).detach(), z.grad, sigmas.detach(), logpi.detach()


class Statement(nn.Module):
    """the reference's MDNRNN as torch modules (its parameter names), for a state_dict of either side"""

    def __init__(self, S, A, H, L, G):
        super().__init__()
        self.S, self.G = S, G
        self.rnn = nn.LSTM(input_size=S + A, hidden_size=H, num_layers=L)
        self.gmm_linear = nn.Linear(H, (2 * S + 1) * G + 2)

    def forward(self, actions, states, hidden=None):
        all_h, last = self.rnn(torch.cat([actions, states], dim=-1), hidden)
        return (*split_lines(self.gmm_linear(all_h), self.G, self.S), all_h, last)

    def losses(self, b, weights, divide=True, last_step_only=False):
        """get_loss on a batch dict of this module's dtype -> gmm, bce, mse, loss (with graph)"""
        mus, sigmas, logpi, rs, nts, _, _ = self(b["action"], b["state"])
        ns, nt, r = b["next_state"], b["not_terminal"], b["reward"]
        if last_step_only:
            ns, nt, r, mus, sigmas, logpi, nts, rs = (x[-1:] for x in (ns, nt, r, mus, sigmas, logpi, nts, rs))
        gmm = gmm_lines(ns, mus, sigmas, logpi) * weights[0]
        bce = F.binary_cross_entropy_with_logits(nts, nt) * weights[1]
        mse = F.mse_loss(rs, r) * weights[2]
        return gmm, bce, mse, (gmm / (self.S + 2) + bce + mse if divide else gmm + bce + mse)
