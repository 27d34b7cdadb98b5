"""TEST INFRASTRUCTURE.  The CEM planner's lines restated for any dtype, and the noise recipe of include/reagent_hip.h restated
in numpy.

One planning step of one world model (reagent/models/cem_planner.py:192-215 through reagent/models/mdn_rnn.py:47-102):
cat([action, state]), nn.LSTM from a ZERO hidden state (or a given one, for the test that shows the difference), gmm_linear,
the split into mus / sigmas / logpi / reward / not_terminal; then the sampling rules: the mixture index by inverse CDF over
exp(logpi) against a uniform, next_state = mu_k + sigma_k * eps, not_terminal = (u < sigmoid(logit)).  The float64 evaluation
is the yardstick of tests/test_cem_kernels.py, the fp32 evaluation calibrates its bounds."""
import numpy as np
import torch
import torch.nn as nn

DRAW_MODEL, DRAW_MIX, DRAW_TERM, DRAW_EPS, DRAW_TN, DRAW_ACTION = range(6)
M32 = np.uint64(0xFFFFFFFF)


class Statement(nn.Module):
    """a MemoryNetwork's MDNRNN as torch's own modules under its parameter names"""

    def __init__(self, S, A, H, L, G):
        super().__init__()
        self.S, self.G = S, G
        self.rnn = nn.LSTM(input_size=S + A, hidden_size=H, num_layers=L)
        self.gmm_linear = nn.Linear(H, (2 * S + 1) * G + 2)

    @classmethod
    def of(cls, memory_network, dtype):
        m = memory_network
        s = cls(m.state_dim, m.action_dim, m.num_hiddens, m.num_hidden_layers, m.num_gaussians)
        s.load_state_dict({k[len("mdnrnn."):]: v.detach().cpu() for k, v in m.state_dict().items()}, strict=True)
        return s.to(dtype)

    @torch.no_grad()
    def z(self, state, action, hidden=None):
        """gmm_linear's output [N, W] for one step of N rows, and the hidden state after it"""
        dtype = self.gmm_linear.weight.dtype
        x = torch.cat([action.to(dtype), state.to(dtype)], dim=-1).unsqueeze(0)
        y, hidden = self.rnn(x) if hidden is None else self.rnn(x, hidden)
        return self.gmm_linear(y)[0], hidden

    def split(self, z):
        """mdn_rnn.py:80-101 — mus [N, G, S], sigmas, logpi [N, G], reward [N], not_terminal [N]"""
        S, G = self.S, self.G
        n = z.shape[0]
        mus = z[:, :G * S].reshape(n, G, S)
        sigmas = torch.exp(z[:, G * S:2 * G * S].reshape(n, G, S))
        logpi = torch.log_softmax(z[:, 2 * G * S:2 * G * S + G], dim=-1)
        return mus, sigmas, logpi, z[:, -2], z[:, -1]


def decide(z64, u_mix, u_term, S, G, terminal_effective):
    """the float64 sampling decisions of rows z64 [N, W] -> (index, its margin, not_terminal, its margin): the margins are the
    distance of the uniform from the nearest CDF edge and from the probability"""
    z64 = np.asarray(z64, dtype=np.float64)
    logits = z64[:, 2 * G * S:2 * G * S + G]
    m = logits.max(axis=1, keepdims=True)
    logpi = logits - m - np.log(np.exp(logits - m).sum(axis=1, keepdims=True))
    cdf = np.cumsum(np.exp(logpi), axis=1)
    u = np.asarray(u_mix, dtype=np.float64)[:, None]
    k = np.minimum((cdf <= u).sum(axis=1), G - 1)
    edges = cdf[:, :G - 1] if G > 1 else np.full((z64.shape[0], 1), np.inf)
    margin_k = np.abs(edges - u).min(axis=1) if G > 1 else np.full(z64.shape[0], np.inf)
    if not terminal_effective:
        return k, margin_k, np.ones(z64.shape[0], dtype=np.int64), np.full(z64.shape[0], np.inf)
    p = 1.0 / (1.0 + np.exp(-z64[:, -1]))
    ut = np.asarray(u_term, dtype=np.float64)
    return k, margin_k, (ut < p).astype(np.int64), np.abs(ut - p)


# ---- the noise recipe ---------------------------------------------------------------------------------------------------
def philox4x32_10(seed, group, offset):
    """Philox4x32-10 with key = seed and counter (group lo, group hi, offset lo, offset hi), vectorised over group / offset:
    -> uint64 array [..., 4] of the four 32-bit outputs"""
    group, offset = np.broadcast_arrays(np.asarray(group, dtype=np.uint64), np.asarray(offset, dtype=np.uint64))
    c = [group & M32, group >> np.uint64(32), offset & M32, offset >> np.uint64(32)]
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & M32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return np.stack(c, axis=-1)


def draw(seed, kind, iteration, n, hi, lo):
    n, hi, lo = (np.asarray(v, dtype=np.uint64) for v in (n, hi, lo))
    group = n | (np.uint64(iteration) << np.uint64(20)) | (np.uint64(kind) << np.uint64(52))
    return philox4x32_10(seed, group, (hi << np.uint64(32)) | lo)


def uniform(x):
    return ((x[..., 0] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24).astype(np.float32)


def normal64(x):
    u1 = (x[..., 0].astype(np.float64) + 1.0) * 2.0 ** -32
    u2 = x[..., 1].astype(np.float64) * 2.0 ** -32
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def rollout_noise(seed, iteration, N, T, S):
    """what rg_cem_fill_noise writes: u_model [N], u_mix [T, N], eps [T, N, S], u_term [T, N]"""
    n = np.arange(N)
    j = np.arange(T)[:, None]
    return dict(
        u_model=uniform(draw(seed, DRAW_MODEL, iteration, n, 0, 0)),
        u_mix=uniform(draw(seed, DRAW_MIX, iteration, n[None, :], j, 0)),
        u_term=uniform(draw(seed, DRAW_TERM, iteration, n[None, :], j, 0)),
        eps=normal64(draw(seed, DRAW_EPS, iteration, n[None, :, None], j[:, :, None], np.arange(S)[None, None, :])).astype(np.float32),
    )


def truncated_normal(seed, iteration, P, D, attempts=32):
    """tn [P, D]: the first of `attempts` standard normals inside [-2, 2], else the last one clamped"""
    p, d = np.arange(P)[:, None], np.arange(D)[None, :]
    out = np.zeros((P, D))
    got = np.zeros((P, D), dtype=bool)
    z = out
    for t in range(attempts):
        z = normal64(draw(seed, DRAW_TN, iteration, p, d, t))
        take = ~got & (np.abs(z) <= 2.0)
        out[take] = z[take]
        got |= take
    out[~got] = np.clip(z[~got], -2.0, 2.0)
    return out


def discrete_actions(seed, iteration, P, T, A):
    u = uniform(draw(seed, DRAW_ACTION, iteration, np.arange(P)[:, None], np.arange(T)[None, :], 0))
    return np.floor(u.astype(np.float64) * A).astype(np.int32)
