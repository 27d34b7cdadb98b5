"""The world-model evaluators' kernels (reagent_amd/csrc/wm_eval.hip): rg_lstm_forward_ablate, rg_wm_mdn_losses,
rg_wm_feature_fill, rg_wm_mus_sensitivity.  Exact where the issue of bits is the statement (a zero-delta variant is
rg_lstm_forward; a variant's losses are rg_mdn_head's on its gathered rows), otherwise a plain float64 torch statement under
the self-calibrating bound of tests/test_lstm_kernels.py (_close).  NaN fills every padding and every output before a run."""
import numpy as np
import pytest
import torch

import reagent_amd._lib as L
from reagent_amd import ops
from test_lstm_kernels import _bits, _close

NAN = float("nan")


def _padded(t, pad=3):
    """t's values in a row-padded buffer whose padding is NaN"""
    big = torch.full((t.shape[0], t.shape[1] + pad), NAN, dtype=t.dtype, device=t.device)
    big[:, :t.shape[1]] = t
    return big[:, :t.shape[1]]


def _layer(H, B, T, In, seed):
    g = torch.Generator().manual_seed(seed)
    k = 1.0 / H ** 0.5
    p = {n: (torch.rand(*s, generator=g) * 2 - 1) * k for n, s in
         (("w_ih", (4 * H, In)), ("w_hh", (4 * H, H)), ("b_ih", (4 * H,)), ("b_hh", (4 * H,)))}
    p["x"] = torch.randn(T * B, In, generator=g)
    p["fill"] = torch.randn(In, generator=g)
    return p


def _ablate(dev, p, T, B, H, table, fill, fill_stride=0):
    """-> h_all, c_all [T, V, B, H] of the kernel; the shared projection is torch's fp32 x W_ih^T + b_ih"""
    V = len(table)
    d = {k: v.to(dev) for k, v in p.items()}
    xproj = (p["x"] @ p["w_ih"].T + p["b_ih"]).view(T, B, 4 * H).to(dev)
    h_all, c_all = (torch.full((T, V * B, H), NAN, device=dev) for _ in range(2))
    ops.lstm_forward_ablate(xproj, _padded(d["x"]), d["w_ih"], d["w_hh"], d["b_hh"],
                            torch.tensor(table, dtype=torch.int32).to(dev), fill.to(dev).contiguous(), fill_stride,
                            max(e - s for s, e in table), h_all, c_all)
    return h_all.view(T, V, B, H).cpu(), c_all.view(T, V, B, H).cpu(), xproj, d


@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("B", [1, 33])
@pytest.mark.parametrize("H", [1, 33, 256])
def test_a_zero_delta_variant_is_rg_lstm_forward(backend, H, B, T):
    dev, In = backend.device, 5
    p = _layer(H, B, T, In, 7 * H + B + T)
    p["x"][:, 2] = 0.75  # a constant column with its own value as the fill: all deltas are zero
    p["fill"][2] = 0.75
    table = [(0, 2), (3, 3), (1, 4), (2, 3), (4, 5)]  # real, empty, real, constant, real
    h_all, c_all, xproj, d = _ablate(dev, p, T, B, H, table, p["fill"])
    h, c = (torch.full((T, B, H), NAN, device=dev) for _ in range(2))
    ops.lstm_forward(xproj, d["w_hh"], d["b_hh"], None, None, h, c)
    for v in (1, 3):
        assert torch.equal(_bits(h_all[:, v]), _bits(h)) and torch.equal(_bits(c_all[:, v]), _bits(c)), v
    for v in (0, 2, 4):
        assert not torch.isnan(h_all[:, v]).any() and not torch.equal(_bits(h_all[:, v]), _bits(h)), v


# block widths 1, 2 and the cap; blocks at column 0 and at the last column; a fill row per variant (stride 3 with the identity:
# the discrete sweep, whose variant i sets every action to e_i)
@pytest.mark.parametrize("H,B,T,In,table,stride", [(33, 33, 3, 5, [(0, 1), (3, 5), (4, 5), (0, 2)], 0),
                                                   (33, 2, 2, L.WM_MAX_BLOCK, [(0, L.WM_MAX_BLOCK)], 0),
                                                   (33, 2, 2, 5, [(0, 3)] * 3, 3)])
def test_variants_against_float64_on_the_materialised_input(backend, H, B, T, In, table, stride):
    p = _layer(H, B, T, In, 11 * In + stride)
    fill = torch.eye(stride).flatten() if stride else p["fill"]
    h_all = _ablate(backend.device, p, T, B, H, table, fill, stride)[0]
    for v, (s, e) in enumerate(table):
        x = p["x"].clone()
        x[:, s:e] = fill[v * stride + s:v * stride + e]
        out = {}
        for dtype in (torch.float64, torch.float32):
            m = torch.nn.LSTM(input_size=In, hidden_size=H)
            with torch.no_grad():
                for name in ("w_ih", "w_hh", "b_ih", "b_hh"):
                    getattr(m, name.replace("w_", "weight_").replace("b_", "bias_") + "_l0").copy_(p[name])
                out[dtype] = m.to(dtype)(x.view(T, B, In).to(dtype))[0]
        _close(h_all[:, v], out[torch.float64], out[torch.float32], f"h_all of variant {v}, block {s}:{e} of {In}")


def test_a_block_wider_than_the_cap_is_refused_by_name(backend):
    z = torch.zeros(1, 4, device=backend.device)
    with pytest.raises(NotImplementedError, match=f"a block {L.WM_MAX_BLOCK + 1} columns wide"):
        ops.lstm_forward_ablate(z.view(1, 1, 4), z, z.view(4, 1), z.view(4, 1), None, torch.zeros(1, 2, dtype=torch.int32,
                                device=backend.device), z.view(4), 0, L.WM_MAX_BLOCK + 1, z.view(1, 1, 4), z.view(1, 1, 4))


@pytest.mark.parametrize("last_step", [False, True])
@pytest.mark.parametrize("T,B", [(1, 1), (1, 5), (3, 3)])
@pytest.mark.parametrize("V", [1, 3])
def test_a_variants_losses_are_rg_mdn_heads_on_its_rows(backend, V, T, B, last_step):
    dev, G, S, N = backend.device, 2, 3, T * B
    g = torch.Generator().manual_seed(100 * V + N)
    W = (2 * S + 1) * G + 2
    z = _padded(torch.randn(T * V * B, W, generator=g).to(dev))
    ns, r = torch.randn(N, S, generator=g).to(dev), torch.randn(N, generator=g).to(dev)
    nt = (torch.rand(N, generator=g) > 0.3).float().to(dev)
    weights, first = (0.7, 1.3, 2.0), (T - 1) * B if last_step else 0
    losses = torch.full((V, 4), NAN, device=dev)
    ops.wm_mdn_losses(z, ns, r, nt, T, B, V, G, weights, True, first, losses)
    for v in range(V):
        zv = z.view(T, V, B, W)[:, v].reshape(N, W)
        one, dz = torch.full((4,), NAN, device=dev), torch.empty(N, W, device=dev)
        ops.mdn_head(zv, ns, r, nt, G, weights, True, first, dz, torch.empty(3 * ops.mdn_head_partials(N), dtype=torch.float64,
                                                                              device=dev), one)
        assert torch.equal(_bits(losses[v]), _bits(one)), (v, losses[v], one)


def test_feature_fill(backend):
    dev, N = backend.device, 300
    g = torch.Generator().manual_seed(3)
    x = torch.randn(N, 12, generator=g)
    x[:, 1] = torch.randint(-9, 9, (N,), generator=g).float()  # integer-valued: the mean's double sum is exact
    x[:, 2] = (torch.arange(N) % 3 == 0).float()  # a single-column enum takes the mean
    counts = {3: 10, 4: 40, 5: 20, 6: 30, 7: 5, 8: 7, 9: 5, 10: 9, 11: 9}
    for c, n in counts.items():
        x[:, c] = (torch.arange(N) < n).float()
    table = [(0, 1), (1, 2), (2, 3), (3, 7), (7, 10), (10, 12)]  # 3:7 even (lower median 20 -> column 5), 7:10 and 10:12 ties
    fill = torch.full((12,), NAN, device=dev)
    ops.wm_feature_fill(_padded(x.to(dev)), torch.tensor(table, dtype=torch.int32).to(dev), fill)
    fill = fill.cpu()
    for c in (0, 1, 2):
        mean = x[:, c].double().mean().item()
        assert abs(fill[c].item() - mean) <= np.spacing(np.float32(abs(mean))), c
    assert fill[1].item() == np.float32(x[:, 1].double().mean().item())
    for s, e in table[3:]:
        sums = x[:, s:e].double().sum(0)
        first = int((sums == torch.median(sums)).nonzero()[0])
        assert fill[s:e].tolist() == [float(i == first) for i in range(e - s)], (s, e, fill[s:e])
    assert fill[3:7].tolist() == [0, 0, 1, 0] and fill[7:10].tolist() == [1, 0, 0] and fill[10:12].tolist() == [1, 0]


def test_mus_sensitivity_against_float64(backend):
    dev, N, G, S = backend.device, 300, 2, 5
    g = torch.Generator().manual_seed(9)
    z0, z1 = (torch.randn(N, (2 * S + 1) * G + 2, generator=g) for _ in range(2))
    table = [(0, 1), (1, 4), (4, 5)]
    got = torch.full((3,), NAN, device=dev)
    ops.wm_mus_sensitivity(_padded(z0.to(dev)), _padded(z1.to(dev)), G, S, torch.tensor(table, dtype=torch.int32).to(dev), got)

    def statement(dtype):
        m0, m1 = (z[:, :G * S].view(N, G, S).to(dtype) for z in (z0, z1))
        return torch.stack([torch.mean(torch.sum(torch.abs(m1[:, :, s:e] - m0[:, :, s:e]), dim=2)) for s, e in table])

    _close(got, statement(torch.float64), statement(torch.float32), "sensitivity")
