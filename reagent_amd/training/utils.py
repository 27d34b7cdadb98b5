"""The helpers of reagent/training/utils.py that the world-model trainers use (host-side tensor construction: no kernel)."""
import torch


def gen_permutations(seq_len: int, num_action: int) -> torch.Tensor:
    """utils.py:57-66 — every action sequence of length seq_len over num_action actions as one-hot floats, in lexical order:
    [seq_len, num_action ** seq_len, num_action].  Sequence p's action at step t is digit t of p written in base num_action,
    most significant digit first (seq_len == 1, which the reference treats apart, is the same statement: p itself)."""
    assert seq_len >= 1 and num_action >= 1, (seq_len, num_action)
    p = torch.arange(num_action ** seq_len)
    weights = num_action ** torch.arange(seq_len - 1, -1, -1)
    digits = (p.unsqueeze(0) // weights.unsqueeze(1)) % num_action  # [seq_len, P]
    return (digits.unsqueeze(-1) == torch.arange(num_action)).float()
