"""TEST INFRASTRUCTURE.  Seq2Reward's lines restated with torch's own operations, for any dtype: the network
(reagent/models/seq2reward_model.py:22-95: nn.LSTM over the actions, every layer's h0 = map_linear(state[0]), lstm_linear at
each row's valid step), the mse loss against the discounted reward sum (reagent/training/world_model/seq2reward_trainer.py:
216-245) and the step predictor's cross-entropy (:261-267).  The float64 evaluation is the yardstick of
tests/test_seq2reward_trainer.py, the fp32 evaluation calibrates its bounds."""
import torch
import torch.nn as nn
import torch.nn.functional as F


class Statement(nn.Module):
    """the reference's Seq2RewardNetwork as torch modules (its parameter names), for a state_dict of either side"""

    def __init__(self, S, A, H, L):
        super().__init__()
        self.L = L
        self.rnn = nn.LSTM(input_size=A, hidden_size=H, num_layers=L)
        self.lstm_linear = nn.Linear(H, 1)
        self.map_linear = nn.Linear(S, H)

    def forward(self, state, action, valid_step=None):
        B = state.shape[1]
        h0 = self.map_linear(state[0][None, :, :].repeat(self.L, 1, 1))
        all_h, _ = self.rnn(action, (h0, torch.zeros_like(h0)))
        last = all_h[-1] if valid_step is None else all_h[valid_step - 1, torch.arange(B)]
        return self.lstm_linear(last)

    def mse_loss(self, b, gamma):
        """get_mse_loss on a batch dict of this module's dtype (valid_step int64 [B, 1])"""
        v = b["valid_step"].flatten()
        pred = self(b["state"], b["action"], v)
        T, B = b["reward"].shape
        mask = torch.Tensor([[gamma ** i for i in range(T)] for _ in range(B)]).transpose(0, 1).to(b["reward"].dtype)
        target = torch.cumsum(b["reward"] * mask, dim=0)[v - 1, torch.arange(B)].unsqueeze(1)
        return F.mse_loss(pred, target)


def step_entropy_loss(params, b):
    """get_step_entropy_loss with the step predictor's parameters (W0, b0, W1, b1, W2, b2, of the batch's dtype)"""
    x = b["state"][0]
    for i in range(0, len(params), 2):
        x = F.linear(x, params[i], params[i + 1])
        if i + 2 < len(params):
            x = F.relu(x)
    return F.cross_entropy(x, b["valid_step"].flatten() - 1)


def mlp(params, x):
    for i in range(0, len(params), 2):
        x = F.linear(x, params[i], params[i + 1])
        if i + 2 < len(params):
            x = F.relu(x)
    return x


def flat_q(m, cur_state, all_permut):
    """get_Q's statement (:43-62) on the Statement module"""
    B = cur_state.shape[0]
    _, P, A = all_permut.shape
    state = cur_state.unsqueeze(0).repeat_interleave(P, dim=1)
    acc = m(state, all_permut.to(cur_state.dtype).repeat(1, B, 1)).reshape(B, A, P // A)
    return torch.max(acc, dim=2).values
