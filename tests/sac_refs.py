"""TEST INFRASTRUCTURE: statements of the continuous-control kernels of reagent_amd/csrc/sac.hip, one plain function each.

Tensors in, tensors out; torch arithmetic in the dtype asked for (float64 is the statement, float32 is "torch fp32 on the
same formula", the calibration of every bound), torch autograd for the gradients.  Nothing here calls a project kernel or
anything from `reagent_amd.ops`: tests/test_sac_head_statements.py and tests/fuzz/fuzz_sac_heads.py hold the kernels to these.

  gaussian_forward_ref    actor.py:199-231        clamp of scale_log, reparameterised sample, tanh squash and its clamp
  gaussian_log_prob_ref   actor.py:166-188, 233-261  get_log_prob of a GIVEN squashed action
  gaussian_backward_ref   actor.py:215-261        autograd through forward + get_log_prob sharing (loc, scale_log)
  critic_head_ref         sac_trainer.py:205-248  target value, the two mse losses and their gradients
  actor_head_ref          sac_trainer.py:23-47, 254-280, 311-320  actor loss (plain / CRR weighted) and the entropy terms
  kld_ref                 sac_trainer.py:282-306  action-embedding KLD term
  td3_target_action_ref   td3_trainer.py:141-146  target-policy smoothing
"""
import math

import numpy as np
import torch

F64 = torch.float64
F32 = torch.float32
LOG_PROB_MIN, LOG_PROB_MAX = -2.0, 2.0                # actor.py:18-19
EPS = 1e-6                                            # actor.py:161 self.eps
CONST = math.log(math.sqrt(2 * math.pi))              # actor.py:160 self.const
A_MAX = float(np.float32(1.0) - np.float32(1e-6))     # the clamp bound the fp32 reference applies: 0.9999989867210388
assert A_MAX == 0.9999989867210388


# ---- the Gaussian head --------------------------------------------------------------------------------------------------
def split(loc_scale, dtype=F64):
    """_get_loc_and_scale_log (actor.py:190-200) without layer norm -> loc, clamped scale_log"""
    A = loc_scale.shape[1] // 2
    ls = loc_scale.to(dtype)
    return ls[:, :A], ls[:, A:].clamp(LOG_PROB_MIN, LOG_PROB_MAX)


def squash(raw):
    """_squash_raw_action (actor.py:202-213) without l2 normalisation"""
    return torch.clamp(torch.tanh(raw), -A_MAX, A_MAX)


def lp_terms(loc, scale_log, action):
    """per element: _normal_log_prob - _squash_correction (actor.py:166-188, 244-247, 261 before the sum)"""
    r = (torch.atanh(action) - loc) / scale_log.exp()
    return (-(r**2) / 2 - scale_log - CONST) - (1 - action**2 + EPS).log()


def gaussian_forward_ref(loc_scale, noise, dtype=F64):
    """stage A: -> (action, squashed_mean) (actor.py:216-220)"""
    loc, sl = split(loc_scale, dtype)
    return squash(loc + noise.to(dtype) * sl.exp()), squash(loc)


def gaussian_log_prob_ref(loc_scale, action, dtype=F64):
    """stage B: get_log_prob at the action given -> (log_prob [B], terms [B, A])"""
    loc, sl = split(loc_scale, dtype)
    t = lp_terms(loc, sl, action.to(dtype))
    return t.sum(1), t


def gaussian_backward_ref(loc_scale, noise, g_action, g_log_prob, kld_coef=None, kld_on_mean=False, dtype=F64):
    """d (sum(a * G_a) + sum(lp * g_lp) + K) / d loc_scale through forward() and get_log_prob() on the same (loc, scale_log).
    K is the KLD term linearised at its coefficients: d K / d x = c0 + c1 x, x the action or the squashed mean.
    -> (d_loc_scale [B, 2A], action, log_prob)"""
    ls = loc_scale.to(dtype).clone().requires_grad_(True)
    a, sm = gaussian_forward_ref(ls, noise, dtype)
    lp, _ = gaussian_log_prob_ref(ls, a, dtype)
    loss = torch.zeros((), dtype=dtype)
    if g_action is not None:
        loss = loss + (a * g_action.to(dtype)).sum()
    if g_log_prob is not None:
        loss = loss + (lp * g_log_prob.to(dtype)).sum()
    if kld_coef is not None:
        A = a.shape[1]
        c0, c1 = kld_coef.to(dtype)[:A], kld_coef.to(dtype)[A:]
        x = sm if kld_on_mean else a
        loss = loss + (c0 * x + 0.5 * c1 * x * x).sum()
    if loss.requires_grad:
        loss.backward()
        grad = ls.grad
    else:
        grad = torch.zeros_like(ls)
    return grad, a.detach(), lp.detach()


# ---- the loss heads -----------------------------------------------------------------------------------------------------
def clamp_lp(lp):
    return lp.clamp(LOG_PROB_MIN, LOG_PROB_MAX)


def critic_head_ref(q1t, q2t, lp_next, reward, not_terminal, gamma, alpha):
    """sac_trainer.py:222-239.  next_state_value is an fp32 tensor that `-= entropy_temperature * log_prob_a` updates in
    place with a float64 temperature: the difference is formed in float64 and rounded to fp32 once.  `discount` is an fp32
    tensor filled with gamma.  -> (y in float64 from that fp32 value, v32, the magnitudes |reward| + |discount v nt|)"""
    v = q1t.to(F64)
    if q2t is not None:
        v = torch.min(v, q2t.to(F64))
    v32 = (v - alpha.to(F64) * clamp_lp(lp_next).to(F64)).to(F32)
    r = reward.to(F64)
    if gamma > 0.0:
        g32 = torch.tensor(gamma, dtype=F32).to(F64)
        nxt = g32 * v32.to(F64) * not_terminal.to(F64)
        return r + nxt, v32, r.abs() + nxt.abs()
    return r.clone(), v32, r.abs()


def crr_weight(advantage, crr_mode, crr_p0, crr_clamp):
    """CRRWeightFn.get_weight_from_advantage (sac_trainer.py:39-47): 1 = indicator, 2 = exponent"""
    if crr_mode == 1:
        return (advantage >= crr_p0).to(advantage.dtype)
    w = torch.exp(advantage / crr_p0)
    return torch.clamp(w, 0.0, crr_clamp) if crr_clamp else w


def actor_head_ref(lp, q1a, q2a, alpha, target_entropy, v_cur=None, crr_mode=0, crr_p0=0.0, crr_clamp=0.0,
                   backprop_log_prob=True, dtype=F64):
    """sac_trainer.py:257-280 and the temperature segment's operand (:316-317).
    -> dict(terms [B] (the loss is their mean), ent [B], g_lp, dq1a, dq2a (None without q2a))"""
    lpd = lp.to(dtype).clone().requires_grad_(True)
    q1d = q1a.to(dtype).clone().requires_grad_(True)
    q2d = q2a.to(dtype).clone().requires_grad_(True) if q2a is not None else None
    mq = q1d if q2d is None else torch.min(q1d, q2d)
    c = clamp_lp(lpd)
    if not backprop_log_prob:
        c = c.detach()
    if crr_mode:
        adv = (mq - v_cur.to(dtype)).detach()
        terms = -(c * crr_weight(adv, crr_mode, crr_p0, crr_clamp).detach())
    else:
        terms = alpha.to(dtype) * c - mq
    loss = terms.mean()
    if loss.requires_grad:
        loss.backward()
    z = lambda t: t.grad if t.grad is not None else torch.zeros_like(t)  # noqa: E731
    return dict(terms=terms.detach(), ent=clamp_lp(lp.to(dtype)) + target_entropy, g_lp=z(lpd), dq1a=z(q1d),
                dq2a=z(q2d) if q2d is not None else None)


def kld_value(x, emb_mean, emb_var):
    """sac_trainer.py:285-304 on the batch x [B, A] -> (kld, per-dimension terms)"""
    m, v = x.mean(0), x.var(0)
    t = 0.5 * ((v + (m - emb_mean) ** 2) / emb_var - 1 + emb_var.log() - v.log())
    return t.sum(), t


def kld_ref(x, squashed, emb_mean, emb_var, weight):
    """-> dict(kld, terms [A], grad [B, A] = d (weight * kld) / d x by autograd, x (the batch the statistic saw), m, v)"""
    xd = x.to(F64)
    if squashed:
        xd = squash(xd)
    xd = xd.clone().requires_grad_(True)
    kld, t = kld_value(xd, emb_mean.to(F64), emb_var.to(F64))
    (weight * kld).backward()
    return dict(kld=kld.detach(), terms=t.detach(), grad=xd.grad, x=xd.detach(), m=xd.detach().mean(0), v=xd.detach().var(0))


# ---- exact kernels ------------------------------------------------------------------------------------------------------
def td3_target_action_ref(next_actor, noise, noise_variance, clip_lo, clip_hi, lo, hi):
    """td3_trainer.py:141-146 in fp32, every operation rounded once in this order"""
    n = (noise * torch.tensor(noise_variance, dtype=F32)).clamp(float(np.float32(clip_lo)), float(np.float32(clip_hi)))
    return (next_actor + n).clamp(float(np.float32(lo)), float(np.float32(hi)))
