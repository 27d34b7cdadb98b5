"""TEST INFRASTRUCTURE: float64 statements of the loss heads of reagent_amd/csrc/heads.hip, one plain function per head.

Tensors in, tensors out; float64 arithmetic, torch autograd for the gradients.  Nothing here calls a project kernel or
anything from `reagent_amd.ops`: tests/test_head_kernels.py and tests/fuzz/fuzz_heads.py both hold the kernels to these.

  qr_head_ref      qrdqn_trainer.py:108-160, :210-218   the (N, B, N) quantile-Huber pair loss and the masked next action
  c51_head_ref     c51_trainer.py:98-187                softmax over atoms, categorical projection with the l == b == u fix-ups
  cpe_head_ref     dqn_trainer_base.py:338-452          reward / CPE q-net losses of the logged action, masked-softmax propensities
  bcq_filter_ref   imitator_training.py:12-25           mask *= (softmax / rowmax >= threshold)
"""
import torch
import torch.nn.functional as F

F64 = torch.float64
NOT_POSSIBLE = -1e9  # ACTION_NOT_POSSIBLE_VAL


def _reward_and_discount(action, reward, reward_boosts, not_terminal, gamma, gamma_exponent):
    """-> (boosted reward [B, 1], discount * not_terminal [B, 1]), float64"""
    B = action.shape[0]
    r = reward.to(F64).reshape(-1, 1)
    if reward_boosts is not None:
        r = r + (action.to(F64) * reward_boosts.to(F64).reshape(1, -1)).sum(1, keepdim=True)
    if gamma_exponent is None:
        disc = torch.full((B, 1), gamma, dtype=F64)
    else:
        disc = torch.pow(torch.tensor(gamma, dtype=F64), gamma_exponent.to(F64).reshape(-1, 1))
    return r, disc * not_terminal.to(F64).reshape(-1, 1)


def _masked_argmax(values, next_mask, fp32_rows):
    """argmax_a (values + NOT_POSSIBLE * (1 - mask)), first maximal index.  Rows listed in `fp32_rows` are decided in the
    reference's own fp32 arithmetic instead: there the penalty absorbs every value of a fully masked row (all keys are
    exactly -1e9), so action 0 wins, while float64 would still rank the masked actions by value."""
    idx = (values + NOT_POSSIBLE * (1 - next_mask.to(F64))).argmax(1)
    if fp32_rows is not None and len(fp32_rows):
        rows = torch.as_tensor(fp32_rows, dtype=torch.int64)
        key32 = values[rows].float() + torch.tensor(NOT_POSSIBLE, dtype=torch.float32) * (1 - next_mask[rows].float())
        idx[rows] = key32.argmax(1)
    return idx


def qr_head_ref(q, qn_online, qn_target, action, next_mask, reward, reward_boosts, not_terminal, gamma, gamma_exponent,
                quantiles, num_atoms, maxq, fp32_rows=None):
    """q, qn_online (None: select with the target net), qn_target: [B, A * N].  maxq: the next atoms are the target net's
    at argmax_a mean_atoms(selection net) under the mask; otherwise next_mask is the logged next action (one-hot).
    -> dict(loss, dq [B, A * N], all_q [B, A], select [B, A] or None (the unpenalised selection values), next_idx or None)"""
    B, A = action.shape
    N = num_atoms
    qd = q.to(F64).clone().requires_grad_()
    cur3, tg3 = qd.view(B, A, N), qn_target.to(F64).view(B, A, N)
    select = next_idx = None
    if maxq:
        select = (qn_online.to(F64).view(B, A, N) if qn_online is not None else tg3).mean(2)
        next_idx = _masked_argmax(select, next_mask, fp32_rows)
        nxt = tg3[torch.arange(B), next_idx]
    else:
        nxt = (tg3 * next_mask.to(F64).unsqueeze(-1)).sum(1)
    r, dn = _reward_and_discount(action, reward, reward_boosts, not_terminal, gamma, gamma_exponent)
    target = (r + dn * nxt).detach()                        # [B, N]
    cur = (cur3 * action.to(F64).unsqueeze(-1)).sum(1)      # [B, N]
    td = target.t().unsqueeze(-1) - cur                     # [N, B, N]: target atom i, row b, current atom j
    hub = torch.where(td.abs() < 1, 0.5 * td.pow(2), td.abs() - 0.5)
    loss = (hub * (quantiles.to(F64) - (td.detach() < 0).to(F64)).abs()).mean()
    loss.backward()
    return dict(loss=loss.detach(), dq=qd.grad, all_q=cur3.detach().mean(2), select=select, next_idx=next_idx)


def c51_head_ref(q, qn_online, qn_target, action, next_mask, reward, reward_boosts, not_terminal, gamma, gamma_exponent,
                 support, qmin, qmax, num_atoms, maxq, fp32_rows=None):
    """logits [B, A * N]; maxq: the next distribution is the target net's at argmax_a E[support] of the selection net
    (qn_online, None: the target net) under the mask; otherwise next_mask is the logged next action (one-hot).
    -> dict(loss, dq [B, A * N], all_q [B, A], select [B, A] or None, next_idx or None)"""
    B, A = action.shape
    N = num_atoms
    sd = support.to(F64)
    qd = q.to(F64).clone().requires_grad_()
    logd = F.log_softmax(qd.view(B, A, N), dim=2)
    next_dist = F.softmax(qn_target.to(F64).view(B, A, N), dim=2)
    select = next_idx = None
    if maxq:
        select = ((F.softmax(qn_online.to(F64).view(B, A, N), dim=2) if qn_online is not None else next_dist) * sd).sum(2)
        next_idx = _masked_argmax(select, next_mask, fp32_rows)
        nd = next_dist[torch.arange(B), next_idx]
    else:
        nd = (next_dist * next_mask.to(F64).unsqueeze(-1)).sum(1)
    r, dn = _reward_and_discount(action, reward, reward_boosts, not_terminal, gamma, gamma_exponent)
    tq = (r + dn * sd).clamp(qmin, qmax)
    b = (tq - qmin) / ((qmax - qmin) / (N - 1.0))
    lo, up = b.floor().to(torch.int64), b.ceil().to(torch.int64)
    lo[(up > 0) * (lo == up)] -= 1
    up[(lo < (N - 1)) * (lo == up)] += 1
    m = torch.zeros_like(nd)
    m.scatter_add_(1, lo, nd * (up.to(F64) - b))
    m.scatter_add_(1, up, nd * (b - lo.to(F64)))
    loss = -(m.detach() * (logd * action.to(F64).unsqueeze(-1)).sum(1)).sum(1).mean()
    loss.backward()
    return dict(loss=loss.detach(), dq=qd.grad, all_q=(logd.detach().exp() * sd).sum(2), select=select, next_idx=next_idx)


def masked_softmax_ref(scores, mask, temperature):
    """softmax of scores / T over the kept entries only; a row that keeps nothing is a zero row"""
    keep = mask > 0
    x = (scores.to(F64) / temperature).masked_fill(~keep, float("-inf"))
    p = torch.softmax(x, dim=1)
    return torch.where(keep.any(1, keepdim=True), p, torch.zeros_like(p)).masked_fill(~keep, 0.0)


def cpe_head_ref(reward_est, q_cpe, q_cpe_tgt_next, next_scores, next_mask, action, reward, extra_metrics, not_terminal,
                 gamma, gamma_exponent, temperature, num_metrics, loss):
    """reward_est, q_cpe, q_cpe_tgt_next: [B, M * A] viewed (B, M, A); loss: "mse" or "huber" (smooth L1, beta 1) for the
    CPE q-net, the reward net is always mse; both means run over B * M elements.
    -> dict(propensities [B, A], reward_loss, cpe_loss, d_reward_est [B, M * A], d_q_cpe [B, M * A])"""
    B, A = action.shape
    M = num_metrics
    p = masked_softmax_ref(next_scores, next_mask, temperature)
    a_log = action.argmax(1)
    real = reward.to(F64).reshape(B, 1)
    if M > 1:
        real = torch.cat([real, extra_metrics.to(F64).reshape(B, M - 1)], dim=1)
    rows = torch.arange(B)
    re = reward_est.to(F64).clone().requires_grad_()
    qc = q_cpe.to(F64).clone().requires_grad_()
    reward_loss = F.mse_loss(re.view(B, M, A)[rows, :, a_log], real)
    _, dn = _reward_and_discount(action, reward, None, not_terminal, gamma, gamma_exponent)
    target = real + dn * (q_cpe_tgt_next.to(F64).view(B, M, A) * p.unsqueeze(1)).sum(2)
    logged = qc.view(B, M, A)[rows, :, a_log]
    cpe_loss = F.mse_loss(logged, target) if loss == "mse" else F.smooth_l1_loss(logged, target)
    reward_loss.backward()
    cpe_loss.backward()
    return dict(propensities=p, reward_loss=reward_loss.detach(), cpe_loss=cpe_loss.detach(), d_reward_est=re.grad,
                d_q_cpe=qc.grad)


def bcq_filter_ref(logits, threshold, mask):
    """-> (mask * keep, ratio) with ratio = softmax / rowmax(softmax) in float64 and keep = ratio >= float32(threshold)
    (the threshold reaches the kernel as an fp32 number)"""
    p = torch.softmax(logits.to(F64), dim=1)
    ratio = p / p.max(dim=1, keepdim=True).values
    thr = torch.tensor(threshold, dtype=torch.float32).to(F64)
    return mask.to(F64) * (ratio >= thr).to(F64), ratio
