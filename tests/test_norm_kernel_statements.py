"""The layer-norm, batch-norm and dropout kernels (reagent_amd/csrc/layernorm.hip, fcopts.hip) held to the float64 statements
of tests/norm_refs.py at every shape where their index arithmetic takes another path.

Bounds.  Nothing here is a literal tolerance and nothing grows with the batch.  For a quantity and a STRATUM (a row class
for layer norm, a column class for batch norm; dgamma / dbeta of layer norm sum over all rows and form the stratum "all")
the bound is the largest of
  4 x the largest error of the float32 statement against the float64 one over a torch-only pool of POOL seeds of that
      shape and input law (the case under test is drawn from another seed),
  4 x the spread of the float64 answer over twins of the operands, and
  4 ulp (fp32) of the quantity's largest magnitude in the stratum.
A twin moves every fp32 operand of the entry point by the unit roundoff 2^-24 (half an ulp at the foot of its binade), each
operand as a whole in one direction, the directions of the operands against each other taken from the columns of an 8 x 8
Hadamard matrix, so any two operands move apart in four of the eight twins.  That is what a correctly rounding producer of
an operand may have handed over: mean and rstd of the backward are such products, and at n = 2 with a row mean of 1000 a
half ulp of `mean` is all of dz.  (Moving the ELEMENTS of one operand against each other would measure the textbook
condition number of a variance instead, under which any one-pass variance of given inputs counts as accurate; the inputs
of these kernels are given exactly.)  For the backward entry points the spread is taken on the closed forms of
norm_refs.*_backward_form, which a test below ties to the autograd statement.
bf16 outputs are not bounded: they equal the fp32 output rounded to nearest even, bit for bit.

Every line "RATIO ..." printed is kernel error / bound of one quantity and stratum (profiles/NOTES_r30.md holds the worst)."""
import math

import numpy as np
import pytest
import torch

import norm_refs as R
import reagent_amd._lib as L
from reagent_amd import ops

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
U = 2.0 ** -24
POOL = 8
EINVAL, EWORKSPACE = -1, -4
NAN = float("nan")
BIG = float(np.float32(1e18))
ACT_NAMES = sorted(L.ACT, key=L.ACT.get)


# ---- shared machinery -------------------------------------------------------------------------------------------------
@pytest.fixture(autouse=True)
def _one_torch_thread():
    """The statements and pools are thousands of small torch operations.  Intra-op threads gain them nothing, and when the
    suite's worker processes share the cores their spin-waits cost this file a factor of 30 (and the other workers their
    cores).  One thread while a test of this file runs; the setting found is put back."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def _ulp(x):
    return float(np.spacing(np.float32(abs(float(x)))))


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16) if t.dtype == BF16 else t.view(torch.int32) if t.dtype == F32 else t


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _sgn(j, k):
    """entry (k, j) of the 8 x 8 Hadamard matrix: the direction operand j moves in twin k"""
    return -1.0 if bin(j & k).count("1") & 1 else 1.0


def _twin(t, j, k):
    return None if t is None else t.double() * (1.0 + _sgn(j, k) * U)


def _sel(t, idx, axis):
    return t if idx is None else t.index_select(axis, idx)


def _maxabs(t):
    return float(t.abs().nan_to_num(nan=math.inf).max()) if t.numel() else 0.0


class Bounds:
    """(quantity, stratum) -> the three terms"""

    def __init__(self):
        self.own, self.spread, self.mag = {}, {}, {}

    @staticmethod
    def _up(d, key, v):
        d[key] = max(d.get(key, 0.0), v)

    def learn(self, q, strata, axis, r64, r32=None, twin=None, base=None):
        for s, idx in strata.items():
            self._up(self.mag, (q, s), _maxabs(_sel(r64, idx, axis)))
            if r32 is not None:
                self._up(self.own, (q, s), _maxabs(_sel(r32.double() - r64, idx, axis)))
            if twin is not None:
                self._up(self.spread, (q, s), _maxabs(_sel(twin - (r64 if base is None else base), idx, axis)))

    def bound(self, q, s):
        return max(4.0 * self.own.get((q, s), 0.0), 4.0 * self.spread.get((q, s), 0.0), 4.0 * _ulp(self.mag[(q, s)]))


def _hold(what, q, got, r64, bd, strata, axis, shrink=1.0):
    """assert |got - statement| <= bound in every stratum; -> the worst ratio"""
    worst = 0.0
    for s, idx in strata.items():
        if idx is not None and idx.numel() == 0:
            continue
        err, b = _maxabs(_sel(got.detach().cpu().double() - r64, idx, axis)), bd.bound(q, s) / shrink
        print(f"RATIO {what} {q} {s} err {err:.3e} bound {b:.3e} ratio {err / b:.3f}")
        assert err <= b, (what, q, s, err, b, bd.own.get((q, s)), bd.spread.get((q, s)), bd.mag.get((q, s)))
        worst = max(worst, err / b)
    return worst


class Padded:
    """an operand as a view of a wider NaN-filled buffer: [rows, cols] inside [rows, cols + pad] (its own leading dimension),
    [len] inside [pad + len + pad]"""

    def __init__(self, dev, shape=None, pad=0, src=None, dtype=F32):
        shape = tuple(src.shape) if src is not None else tuple(shape)
        if len(shape) == 2:
            self.buf = torch.full((shape[0], shape[1] + pad), NAN, dtype=dtype, device=dev)
            self.v = self.buf[:, :shape[1]]
        else:
            self.buf = torch.full((shape[0] + 2 * pad,), NAN, dtype=dtype, device=dev)
            self.v = self.buf[pad:pad + shape[0]]
        if src is not None:
            self.v.copy_(src)

    def intact(self):
        """the padding is still NaN"""
        return int(self.buf.isnan().sum().item()) - int(self.v.isnan().sum().item()) == self.buf.numel() - self.v.numel()

    def cpu(self):
        return self.v.detach().cpu().contiguous()


def _workspace(dev, nbytes, dtype):
    """-> (buffer with a NaN tail of 16 elements, the view of exactly nbytes handed to the kernel)"""
    k = nbytes // torch.empty((), dtype=dtype).element_size()
    buf = torch.full((k + 16,), NAN, dtype=dtype, device=dev)
    return buf, buf[:k]


# ---- layer norm: cases ------------------------------------------------------------------------------------------------
LN_NS = [1, 2, 63, 64, 65, 127, 128, 129, 1000, 2047, 2048]
LN_BS = [1, 3, 4, 5, 9, 13, 17, 29, 33]  # n_wg 1, 1, 1, 2, 3, 4, 5, 8, 9: both loops of ln_param_grad_kernel, 0..3 idle waves
LN_SHAPES = sorted({(B, n) for n in LN_NS for B in (1, 5)} | {(B, n) for B in LN_BS for n in (65, 2048)}
                   | {(2, 65), (6, 65)})  # (the last two: a workgroup with two idle waves)
ROW_CLASSES = ["ordinary", "large_mean", "constant", "tiny_spread", "large"]
LN_ROW_Q, LN_PAR_Q = ("y", "mean", "rstd", "dz"), ("dgamma", "dbeta")
LN_MAX_PER_LANE = 32


def _ln_emu_cost(B, n):
    """lane-iterations the interpreter runs per pass over the rows: every wave of every workgroup walks all
    LN_MAX_PER_LANE register slots of its 64 lanes whatever n is, so the cost goes with the workgroups, not with n"""
    return (B + 3) // 4 * 4 * 64 * LN_MAX_PER_LANE


LN_EMU_BUDGET = 1 << 20  # lane-iterations the interpreter runs in about a second: 128 workgroups
LN_SMALL = [s for s in LN_SHAPES if _ln_emu_cost(*s) <= LN_EMU_BUDGET]
assert LN_SMALL == LN_SHAPES  # nine workgroups at the most: no layer-norm shape is left to the GPU alone


def ln_rows(B, n):
    """row r is of class (r + n) mod 5 -> {class: rows}"""
    return {c: torch.tensor([r for r in range(B) if (r + n) % 5 == k], dtype=torch.long) for k, c in enumerate(ROW_CLASSES)}


def ln_inputs(B, n, seed):
    gen = torch.Generator().manual_seed(1_000_003 * seed + 4099 * B + n)
    z = torch.randn(B, n, generator=gen) * 2 + 0.5
    rows = ln_rows(B, n)
    z[rows["large_mean"]] += 999.5
    z[rows["constant"]] = 0.75
    z[rows["tiny_spread"]] = 1.0 + 1e-4 * torch.randn(len(rows["tiny_spread"]), n, generator=gen)
    # +-1e18 at no more than 128 columns of the row: the sum of their squares, at most 1.28e38, stays inside fp32, so neither
    # torch's fp32 nor a kernel that sums squared deviations in fp32 may overflow; anything cubed or summed unshifted would
    step = (n + 127) // 128
    cols = torch.arange(0, n, step)
    for r in rows["large"]:  # (signs drawn, not alternating: a sum that runs +, -, +, - in order is exact by accident)
        z[r, cols] = torch.where(torch.rand(len(cols), generator=gen) < 0.5, BIG, -BIG).to(F32)
    gamma, beta = torch.rand(n, generator=gen) + 0.5, torch.randn(n, generator=gen) * 0.2
    g = torch.randn(B, n, generator=gen)
    return dict(z=z, gamma=gamma, beta=beta, g=g, rows=rows)


def ln_ref(p, act, eps, dtype):
    return R.layer_norm_ref(p["z"], p["gamma"], p["beta"], eps, act, p["g"], dtype)


def ln_strata(p, q):
    return (p["rows"], 0) if q in LN_ROW_Q else ({"all": None}, 0)


_LN = {}


def ln_case(B, n, act="relu", eps=1e-5):
    """the case under test (seed 0), its float64 and float32 statements and the bounds of its shape (computed once, left
    unchanged)"""
    key = (B, n, act, eps)
    if key not in _LN:
        bd = Bounds()
        for k in range(POOL):
            p = ln_inputs(B, n, k + 1)
            r64, r32 = ln_ref(p, act, eps, F64), ln_ref(p, act, eps, F32)
            fw = R.layer_norm_ref(_twin(p["z"], 1, k), _twin(p["gamma"], 2, k), _twin(p["beta"], 3, k), eps, act, None, F64)
            d = {x: p[x].double() for x in ("g", "z", "gamma")}
            base = R.layer_norm_backward_form(d["g"], d["z"], r64["mean"], r64["rstd"], d["gamma"])
            bw = R.layer_norm_backward_form(_twin(p["g"], 1, k), _twin(p["z"], 2, k), _twin(r64["mean"], 3, k),
                                            _twin(r64["rstd"], 4, k), _twin(p["gamma"], 5, k))
            for q in LN_ROW_Q + LN_PAR_Q:
                strata, axis = ln_strata(p, q)
                if q in fw:
                    bd.learn(q, strata, axis, r64[q], r32[q], fw[q])
                else:
                    bd.learn(q, strata, axis, r64[q], r32[q], bw[q], base[q])
        p = ln_inputs(B, n, 0)
        _LN[key] = (p, ln_ref(p, act, eps, F64), ln_ref(p, act, eps, F32), bd)
    return _LN[key]


def run_ln(dev, p, act, eps, y="both", stats=True, dz="both", pads=(3, 5, 1, 7, 2, 4), backward=True):
    """the two entry points on NaN-padded strided operands -> cpu tensors.  y / dz: "both" (bf16 + fp32), "bf16", "f32"
    (the typed output alone, in fp32) or "f32only" (y32 / dz32 alone)"""
    B, n = p["z"].shape
    zp, gp = Padded(dev, src=p["z"], pad=pads[0]), Padded(dev, src=p["g"], pad=pads[1])
    gam, bet = Padded(dev, src=p["gamma"], pad=pads[2]), Padded(dev, src=p["beta"], pad=pads[3])
    held = [zp, gp, gam, bet]

    def outs(mode, pad_a, pad_b):
        t = Padded(dev, (B, n), pad_a, dtype=F32 if mode == "f32" else BF16) if mode != "f32only" else None
        t32 = Padded(dev, (B, n), pad_b) if mode in ("both", "f32only") else None
        held.extend(x for x in (t, t32) if x is not None)
        return t, t32

    yo, y32 = outs(y, pads[2], pads[3])
    mean, rstd = (Padded(dev, (B,), pads[4]), Padded(dev, (B,), pads[5])) if stats else (None, None)
    held.extend(x for x in (mean, rstd) if x is not None)
    v = lambda t: None if t is None else t.v  # noqa: E731
    ops.layer_norm_forward(zp.v, gam.v, bet.v, eps, L.ACT[act], y=v(yo), y32=v(y32), mean=v(mean), rstd=v(rstd))
    out = dict(y=None if yo is None else yo.cpu(), y32=None if y32 is None else y32.cpu(),
               mean=None if mean is None else mean.cpu(), rstd=None if rstd is None else rstd.cpu())
    if backward:
        assert stats
        nbytes = L.lib().rg_layer_norm_backward_workspace_bytes(B, n)
        assert nbytes == (B + 3) // 4 * 2 * n * 4
        wbuf, ws = _workspace(dev, nbytes, F32)
        dzo, dz32 = outs(dz, pads[4], pads[5])
        dg, db = Padded(dev, (n,), pads[0]), Padded(dev, (n,), pads[1])
        held.extend([dg, db])
        ops.layer_norm_backward(gp.v, zp.v, mean.v, rstd.v, gam.v, dg.v, db.v, ws, dz=v(dzo), dz32=v(dz32))
        assert bool(wbuf[ws.numel():].isnan().all()), "the workspace beyond workspace_bytes was written"
        assert not bool(ws.isnan().any()), "the workspace is [n_wg, 2n] partials, all of them written"
        out.update(dz=None if dzo is None else dzo.cpu(), dz32=None if dz32 is None else dz32.cpu(), dgamma=dg.cpu(),
                   dbeta=db.cpu())
    for t in held:
        assert t.intact(), "padding of a strided operand was written"
    assert torch.equal(zp.cpu(), p["z"]) and torch.equal(gp.cpu(), p["g"]) and torch.equal(gam.cpu(), p["gamma"])
    return out


def check_ln(dev, B, n, act="relu", eps=1e-5):
    """both entry points, every output, against the bounds of the shape -> worst ratio per quantity"""
    p, r64, _, bd = ln_case(B, n, act, eps)
    got = run_ln(dev, p, act, eps)
    what, worst = f"layer_norm B={B} n={n} {act} eps={eps:g}", {}
    for q, k in (("y", "y32"), ("mean", "mean"), ("rstd", "rstd"), ("dz", "dz32"), ("dgamma", "dgamma"), ("dbeta", "dbeta")):
        strata, axis = ln_strata(p, q)
        worst[q] = _hold(what, q, got[k], r64[q], bd, strata, axis)
    assert _same_bits(got["y"], got["y32"].to(BF16)) and _same_bits(got["dz"], got["dz32"].to(BF16))  # round to nearest even
    return worst


# ---- layer norm: tests ------------------------------------------------------------------------------------------------
def test_layer_norm_cases_hold_every_row_class_where_it_is_said_to_be():
    seen = set()
    for B, n in LN_SHAPES:
        p = ln_inputs(B, n, 0)
        rows, z = p["rows"], p["z"].double()
        assert sum(len(v) for v in rows.values()) == B
        for k, c in enumerate(ROW_CLASSES):
            assert len(rows[c]) == len([r for r in range(B) if (r + n) % 5 == k])
            seen |= {c} if len(rows[c]) else set()
        assert bool((z[rows["constant"]] == 0.75).all())  # the variance is exactly 0
        assert bool((z[rows["large_mean"]].mean(1) > 990).all()) and bool((z[rows["large"]].abs().amax(1) == BIG).all())
        assert bool(((z[rows["large"]].abs() == BIG).sum(1) <= 128).all())
        if n > 1 and len(rows["tiny_spread"]):
            sd = z[rows["tiny_spread"]].std(1, unbiased=False)
            assert bool(((sd > 0) & (sd < 1e-3)).all())
            assert bool((z[rows["ordinary"]].abs().amax(1) < 20).all())
    assert seen == set(ROW_CLASSES)
    assert {(B + 3) // 4 for B, _ in LN_SHAPES} == {1, 2, 3, 4, 5, 8, 9} and {(-B) % 4 for B, _ in LN_SHAPES} == {0, 1, 2, 3}
    assert {ACT_NAMES[(B + n) % len(ACT_NAMES)] for B, n in LN_SHAPES} == set(L.ACT)


def test_torch_fp32_meets_every_layer_norm_bound():
    """no kernel runs: the float32 statement on the case under test (a seed outside the pool) passes what the kernels must"""
    for B, n in LN_SHAPES:
        act = ACT_NAMES[(B + n) % len(ACT_NAMES)]
        p, r64, r32, bd = ln_case(B, n, act)
        for q in LN_ROW_Q + LN_PAR_Q:
            strata, axis = ln_strata(p, q)
            _hold(f"torch-fp32 layer_norm B={B} n={n}", q, r32[q], r64[q], bd, strata, axis)


def test_the_closed_forms_are_the_autograd_statements():
    """in float64, at the statement's own mean and rstd, far inside every bound: the conditioning term measures the statement"""
    for B, n in [(5, 2), (5, 65), (9, 2048)]:
        p, r64, _, bd = ln_case(B, n, ACT_NAMES[(B + n) % len(ACT_NAMES)])
        f = R.layer_norm_backward_form(p["g"].double(), p["z"].double(), r64["mean"], r64["rstd"], p["gamma"].double())
        for q in ("dz", "dgamma", "dbeta"):
            strata, axis = ln_strata(p, q)
            _hold("closed form layer_norm", q, f[q], r64[q], bd, strata, axis, shrink=1024.0)
    for B, n in [(3, 65), (257, 5)]:
        for training in (True, False):
            o = dict(BN_DEFAULT, training=training)
            p, r64, _, bd = bn_case(B, n, 1, o)
            mean = r64["save_mean"] if training else p["rm"].double()
            rstd = r64["save_rstd"] if training else 1.0 / torch.sqrt(p["rv"].double() + BN_EPS)
            f = R.batch_norm_backward_form(p["g"].double(), p["x"].double(), mean, rstd, p["gamma"].double(), training)
            for q in ("dx", "dgamma", "dbeta"):
                _hold("closed form batch_norm", q, f[q], r64[q], bd, p["cols"], f[q].dim() - 1, shrink=1024.0)


@pytest.mark.parametrize("B,n", LN_SMALL)
def test_layer_norm_against_float64(backend, B, n):
    check_ln(backend.device, B, n, ACT_NAMES[(B + n) % len(ACT_NAMES)])


@pytest.mark.parametrize("eps", [1e-5, 1e-12])
@pytest.mark.parametrize("act", ACT_NAMES)
def test_layer_norm_options(backend, act, eps):
    """every activation at both eps against the statement; an output asked for alone, or without mean / rstd, has the bits
    it has when everything is asked for"""
    B, n = 5, 65
    dev = backend.device
    check_ln(dev, B, n, act, eps)
    p = ln_case(B, n, act, eps)[0]
    full = run_ln(dev, p, act, eps)
    a = run_ln(dev, p, act, eps, y="f32", dz="f32")  # the typed output alone, fp32
    assert a["y32"] is None and a["dz32"] is None and _same_bits(a["y"], full["y32"]) and _same_bits(a["dz"], full["dz32"])
    b = run_ln(dev, p, act, eps, y="bf16", dz="bf16")  # the typed output alone, bf16
    assert _same_bits(b["y"], full["y"]) and _same_bits(b["dz"], full["dz"])
    c = run_ln(dev, p, act, eps, y="f32only", dz="f32only")  # y32 / dz32 alone
    assert c["y"] is None and c["dz"] is None and _same_bits(c["y32"], full["y32"]) and _same_bits(c["dz32"], full["dz32"])
    for k in ("dgamma", "dbeta", "mean", "rstd"):
        assert _same_bits(a[k], full[k]) and _same_bits(b[k], full[k]) and _same_bits(c[k], full[k])
    d = run_ln(dev, p, act, eps, stats=False, backward=False)  # mean and rstd null
    assert d["mean"] is None and _same_bits(d["y32"], full["y32"]) and _same_bits(d["y"], full["y"])


def test_layer_norm_of_nearly_constant_rows(backend):
    """tests/fuzz/fuzz_fc_options.py found this one: ten workgroups, eight rows of spread 1e-4 around 1, eps far below their
    variance.  A variance taken around the rounded mean without its residual term misses rstd by 6 ulp here."""
    check_ln(backend.device, 40, 66, "linear", 1e-12)


def test_layer_norm_row_alone_two_runs_and_strides(backend):
    B, n, act = 13, 129, "tanh"
    dev = backend.device
    p = ln_case(B, n, act)[0]
    whole, again = run_ln(dev, p, act, 1e-5), run_ln(dev, p, act, 1e-5)
    for k in whole:
        assert _same_bits(whole[k], again[k]), k  # two runs give the same bits
    other = run_ln(dev, p, act, 1e-5, pads=(0, 0, 0, 0, 0, 0))  # the same rows, contiguous
    for k in whole:
        assert _same_bits(whole[k], other[k]), k  # dgamma and dbeta among them
    for r in (0, 6, 12):  # a row's y and dz depend on that row alone (first wave of a workgroup, a middle one, the last row)
        one = dict(p, z=p["z"][r:r + 1], g=p["g"][r:r + 1])
        alone = run_ln(dev, one, act, 1e-5)
        for k in ("y", "y32", "dz", "dz32", "mean", "rstd"):
            assert _same_bits(whole[k][r:r + 1], alone[k]), (k, r)


def test_layer_norm_refusals_by_code(backend):
    dev = backend.device
    t = torch.zeros(3 * 2049, device=dev)
    ptr, s, lib = t.data_ptr(), L.stream_ptr(), L.lib()
    assert lib.rg_layer_norm_backward_workspace_bytes(0, 8) == 0 and lib.rg_layer_norm_backward_workspace_bytes(8, 0) == 0
    assert lib.rg_layer_norm_backward_workspace_bytes(5, 3) == 2 * 2 * 3 * 4

    def fwd(B=2, n=3, z=ptr, gamma=ptr, beta=ptr, y=ptr, y32=ptr, mean=ptr, rstd=ptr):
        return lib.rg_layer_norm_forward(z, n, gamma, beta, 1e-5, 0, B, n, y, L.DT_F32, n, y32, n, mean, rstd, s)

    def bwd(B=2, n=3, g=ptr, z=ptr, mean=ptr, rstd=ptr, gamma=ptr, dz=ptr, dz32=ptr, dgamma=ptr, dbeta=ptr, ws=ptr, wsb=None):
        wsb = lib.rg_layer_norm_backward_workspace_bytes(B, n) if wsb is None else wsb
        return lib.rg_layer_norm_backward(g, n, z, n, mean, rstd, gamma, B, n, dz, L.DT_F32, n, dz32, n, dgamma, dbeta, ws, wsb, s)

    assert fwd() == 0 and bwd() == 0
    assert fwd(mean=None, rstd=None) == 0 and fwd(y=None) == 0 and fwd(y32=None) == 0 and bwd(dz=None) == 0 and bwd(dz32=None) == 0
    for k in ("z", "gamma", "beta"):
        assert fwd(**{k: None}) == EINVAL, k
    for k in ("g", "z", "mean", "rstd", "gamma", "dgamma", "dbeta"):
        assert bwd(**{k: None}) == EINVAL, k
    assert fwd(y=None, y32=None) == EINVAL and bwd(dz=None, dz32=None) == EINVAL
    for call in (fwd, bwd):
        assert call(B=0) == EINVAL and call(B=-1) == EINVAL and call(n=0) == EINVAL and call(n=-1) == EINVAL
        assert call(B=1, n=2048) == 0 and call(B=1, n=2049) == L.EUNSUPPORTED
    assert bwd(ws=None) == EWORKSPACE and bwd(wsb=2 * 3 * 4 - 1) == EWORKSPACE and bwd(wsb=0) == EWORKSPACE
    f = dict(dtype=F32, device=dev)
    z = torch.zeros(1, 2049, **f)
    with pytest.raises(L.ReagentHipError, match=r"rg_layer_norm_forward failed.*code -3"):
        ops.layer_norm_forward(z, z[0], z[0], 1e-5, 0, y32=torch.empty_like(z))
    with pytest.raises(L.ReagentHipError, match=r"rg_layer_norm_forward failed.*code -1"):
        ops.layer_norm_forward(z[:, :4], z[0, :4], z[0, :4], 1e-5, 0)
    with pytest.raises(L.ReagentHipError, match=r"rg_layer_norm_backward failed.*code -4"):
        ops.layer_norm_backward(z[:, :4], z[:, :4], z[0, :1], z[0, :1], z[0, :4], torch.empty(4, **f), torch.empty(4, **f),
                                torch.empty(7, **f), dz32=torch.empty(1, 4, **f))


# ---- batch norm: cases ------------------------------------------------------------------------------------------------
BN_NS = [1, 63, 64, 65, 129]
BN_BS = [2, 3, 255, 256, 257, 512, 513]  # bn_chunks 1, 1, 1, 1, 2, 2, 3
BN_SHAPES = [(B, n) for B in BN_BS for n in BN_NS]
BN_CAP = [(16384, 3), (16385, 3), (20000, 3)]  # the 64-chunk cap: per = 256, 257, 313 rows
COL_CLASSES = ["ordinary", "mean4096", "mean30000", "constant", "zero"]
BN_EPS = 1e-5
BN_Q = ("y", "save_mean", "save_rstd", "running_mean", "running_var", "dx", "dgamma", "dbeta")
BN_DEFAULT = dict(training=True, gamma=True, beta=True, running=True, updates=1, momentum=0.1)


def _bn_emu_cost(B, n):
    """elements the interpreter sweeps: each of the five kernels of a forward and a backward visits every x[b, c] once (the
    partial-sum kernels as whole 64-column workgroups)"""
    return B * ((n + 63) // 64 * 64)


BN_EMU_BUDGET = 1 << 17  # elements per sweep the interpreter takes in a tenth of a second (513 x 192 is 0.1 s)
BN_SMALL = [s for s in BN_SHAPES if _bn_emu_cost(*s) <= BN_EMU_BUDGET]
BN_LARGE = [s for s in BN_SHAPES + BN_CAP if _bn_emu_cost(*s) > BN_EMU_BUDGET]
assert BN_SMALL == BN_SHAPES and BN_LARGE == BN_CAP


def _shift(B, n):
    return (BN_BS + [b for b, _ in BN_CAP]).index(B) if B in BN_BS or (B, n) in BN_CAP else B


def bn_cols(n, shift):
    """column c is of class (c + shift) mod 5 -> {class: columns}"""
    return {k: torch.tensor([c for c in range(n) if (c + shift) % 5 == i], dtype=torch.long) for i, k in enumerate(COL_CLASSES)}


def bn_inputs(B, n, shift, seed):
    gen = torch.Generator().manual_seed(1_000_003 * seed + 8191 * B + 7 * n + shift)
    x = torch.randn(B, n, generator=gen) * 2 + 1
    cols = bn_cols(n, shift)
    for k, (m, sd) in (("mean4096", (4096.0, 0.01)), ("mean30000", (30000.0, 0.05))):
        x[:, cols[k]] = m + sd * torch.randn(B, len(cols[k]), generator=gen)
    x[:, cols["constant"]] = 0.1
    x[:, cols["zero"]] = 0.0
    r = lambda *s: torch.rand(*s, generator=gen)  # noqa: E731
    return dict(x=x, g=torch.randn(B, n, generator=gen), gamma=r(n) + 0.5, beta=torch.randn(n, generator=gen),
                rm=torch.randn(n, generator=gen) * 0.3, rv=r(n) * 1.5 + 0.5, cols=cols)


def _bn_operands(p, o):
    return (p["gamma"] if o["gamma"] else None, p["beta"] if o["gamma"] and o["beta"] else None,
            p["rm"] if o["running"] or not o["training"] else None, p["rv"] if o["running"] or not o["training"] else None)


def bn_ref(p, o, dtype):
    ga, be, rm, rv = _bn_operands(p, o)
    return R.batch_norm_ref(p["x"], ga, be, rm, rv, o["training"], o["momentum"], BN_EPS, o["updates"], p["g"], dtype)


_BN = {}


def bn_case(B, n, shift, o):
    key = (B, n, shift, tuple(sorted(o.items())))
    if key not in _BN:
        bd = Bounds()
        tr = o["training"]
        for k in range(POOL):
            p = bn_inputs(B, n, shift, k + 1)
            ga, be, rm, rv = _bn_operands(p, o)
            r64, r32 = bn_ref(p, o, F64), bn_ref(p, o, F32)
            fw = R.batch_norm_ref(_twin(p["x"], 1, k), _twin(ga, 2, k), _twin(be, 3, k), _twin(rm, 4, k), _twin(rv, 5, k), tr,
                                  o["momentum"], BN_EPS, o["updates"], None, F64)
            mean = r64["save_mean"] if tr else rm.double()
            rstd = r64["save_rstd"] if tr else 1.0 / torch.sqrt(rv.double() + BN_EPS)
            rstd_t = _twin(rstd, 4, k) if tr else 1.0 / torch.sqrt(_twin(rv, 4, k) + BN_EPS)
            dd = lambda t: None if t is None else t.double()  # noqa: E731
            base = R.batch_norm_backward_form(p["g"].double(), p["x"].double(), mean, rstd, dd(ga), tr)
            bw = R.batch_norm_backward_form(_twin(p["g"], 1, k), _twin(p["x"], 2, k), _twin(mean, 3, k), rstd_t, _twin(ga, 5, k), tr)
            for q in BN_Q:
                if r64.get(q) is None:
                    continue
                axis = r64[q].dim() - 1
                if q in bw:
                    bd.learn(q, p["cols"], axis, r64[q], r32[q], bw[q], base[q])
                else:
                    bd.learn(q, p["cols"], axis, r64[q], r32[q], fw[q])
        p = bn_inputs(B, n, shift, 0)
        _BN[key] = (p, bn_ref(p, o, F64), bn_ref(p, o, F32), bd)
    return _BN[key]


def run_bn(dev, p, o, pads=(3, 5, 1, 2), want=("dx", "dgamma", "dbeta")):
    """forward and backward on NaN-padded strided x, g, y, dx -> cpu tensors (None where not asked for or not defined)"""
    B, n = p["x"].shape
    tr = o["training"]
    ga, be, rm, rv = _bn_operands(p, o)
    xp, gp = Padded(dev, src=p["x"], pad=pads[0]), Padded(dev, src=p["g"], pad=pads[1])
    yp = Padded(dev, (B, n), pads[2])
    dxp = Padded(dev, (B, n), pads[3]) if "dx" in want else None
    vec = lambda t, k: None if t is None else Padded(dev, src=t, pad=k)  # noqa: E731
    gam, bet, rmp, rvp = vec(ga, 1), vec(be, 2), vec(rm, 3), vec(rv, 4)
    sm, sr = (Padded(dev, (n,), 2), Padded(dev, (n,), 3)) if tr else (None, None)
    dg, db = (Padded(dev, (n,), 1) if "dgamma" in want else None), (Padded(dev, (n,), 4) if "dbeta" in want else None)
    nbytes = L.lib().rg_batch_norm_workspace_bytes(B, n)
    chunks = min(64, (B + 255) // 256)
    assert nbytes == chunks * 2 * n * 8 + 2 * n * 4
    wbuf, ws = _workspace(dev, nbytes, F64)
    v = lambda t: None if t is None else t.v  # noqa: E731
    ops.batch_norm_forward(xp.v, v(gam), v(bet), v(rmp), v(rvp), tr, o["momentum"], BN_EPS, yp.v, v(sm), v(sr), ws if tr else None,
                           stat_updates=o["updates"])
    if tr:
        ops.batch_norm_backward(gp.v, xp.v, v(gam), sm.v, sr.v, None, True, BN_EPS, ws, v(dxp), v(dg), v(db))
    else:
        ops.batch_norm_backward(gp.v, xp.v, v(gam), rmp.v, None, rvp.v, False, BN_EPS, ws, v(dxp), v(dg), v(db))
    assert bool(wbuf[ws.numel():].isnan().all()), "the workspace beyond workspace_bytes was written"
    for t in (xp, gp, yp, dxp, gam, bet, rmp, rvp, sm, sr, dg, db):
        assert t is None or t.intact(), "padding of a strided operand was written"
    assert torch.equal(xp.cpu(), p["x"]) and torch.equal(gp.cpu(), p["g"])
    c = lambda t: None if t is None else t.cpu()  # noqa: E731
    return dict(y=c(yp), save_mean=c(sm), save_rstd=c(sr), running_mean=c(rmp), running_var=c(rvp), dx=c(dxp), dgamma=c(dg),
                dbeta=c(db))


def check_bn(dev, B, n, shift=None, **opts):
    """forward and backward of one mode, every output the mode defines, against the bounds of the shape"""
    o = dict(BN_DEFAULT, **opts)
    shift = _shift(B, n) if shift is None else shift
    p, r64, _, bd = bn_case(B, n, shift, o)
    got = run_bn(dev, p, o)
    what = (f"batch_norm B={B} n={n} {'train' if o['training'] else 'eval'} gamma={int(o['gamma'])} beta={int(o['beta'])} "
            f"running={int(o['running'])} updates={o['updates']} momentum={o['momentum']}")
    worst = {}
    for q in BN_Q:
        if r64.get(q) is None:
            continue
        if not o["training"] and q.startswith("running"):
            assert _same_bits(got[q], p["rm" if q == "running_mean" else "rv"])  # eval mode leaves them alone
            continue
        worst[q] = _hold(what, q, got[q], r64[q], bd, p["cols"], r64[q].dim() - 1)
    if o["gamma"] and not o["beta"]:  # a zero bias still has a gradient
        assert got["dbeta"] is not None and r64["dbeta"] is None
    return worst, got, p


# ---- batch norm: tests ------------------------------------------------------------------------------------------------
def test_batch_norm_cases_hold_every_column_class_where_it_is_said_to_be():
    seen = set()
    for B, n in BN_SHAPES + BN_CAP:
        p = bn_inputs(B, n, _shift(B, n), 0)
        cols, x = p["cols"], p["x"].double()
        assert sum(len(v) for v in cols.values()) == n
        for i, k in enumerate(COL_CLASSES):
            assert len(cols[k]) == len([c for c in range(n) if (c + _shift(B, n)) % 5 == i])
            seen |= {(k, n)} if len(cols[k]) else set()
        assert bool((x[:, cols["constant"]] == float(np.float32(0.1))).all()) and bool((x[:, cols["zero"]] == 0).all())
        assert bool(((x[:, cols["mean4096"]] - 4096).abs() < 0.1).all()) and bool(((x[:, cols["mean30000"]] - 30000).abs() < 0.5).all())
        assert bool((x[:, cols["ordinary"]].abs() < 20).all())
    assert {k for k, n in seen if n == 1} == set(COL_CLASSES) and {k for k, n in seen if n == 3} == set(COL_CLASSES)
    assert sorted({min(64, (B + 255) // 256) for B, _ in BN_SHAPES + BN_CAP}) == [1, 2, 3, 64]


def test_torch_fp32_meets_every_batch_norm_bound():
    """no kernel runs (see the layer-norm twin of this test)"""
    for B, n in BN_SHAPES + BN_CAP:
        for training in (True, False):
            p, r64, r32, bd = bn_case(B, n, _shift(B, n), dict(BN_DEFAULT, training=training))
            for q in BN_Q:
                if r64.get(q) is not None:
                    _hold(f"torch-fp32 batch_norm B={B} n={n} training={training}", q, r32[q], r64[q], bd, p["cols"], r64[q].dim() - 1)


@pytest.mark.parametrize("B,n", BN_SMALL)
def test_batch_norm_against_float64(backend, B, n):
    check_bn(backend.device, B, n)
    check_bn(backend.device, B, n, training=False)


@pytest.mark.gpu
@pytest.mark.parametrize("B,n", BN_LARGE)
def test_batch_norm_against_float64_at_the_chunk_cap(B, n):
    check_bn("cuda", B, n)
    check_bn("cuda", B, n, training=False)


BN_OPTIONS = [dict(gamma=False), dict(beta=False), dict(running=False), dict(updates=0), dict(updates=2),
              dict(momentum=1.0), dict(momentum=1.0, updates=2), dict(training=False, gamma=False),
              dict(training=False, beta=False)]


@pytest.mark.parametrize("opts", BN_OPTIONS, ids=lambda o: "-".join(f"{k}={v}" for k, v in o.items()))
@pytest.mark.parametrize("B,n", [(3, 65), (257, 5)])
def test_batch_norm_options(backend, B, n, opts):
    _, got, p = check_bn(backend.device, B, n, shift=1, **opts)
    o = dict(BN_DEFAULT, **opts)
    if o["training"] and o["running"] and o["updates"] == 0:  # no evaluation: the running statistics keep their bits
        assert _same_bits(got["running_mean"], p["rm"]) and _same_bits(got["running_var"], p["rv"])
    if not o["running"]:
        assert got["running_mean"] is None and got["running_var"] is None


@pytest.mark.parametrize("training", [True, False])
def test_batch_norm_backward_outputs_omitted_in_turn(backend, training):
    o = dict(BN_DEFAULT, training=training)
    p = bn_case(257, 5, 1, o)[0]
    full = run_bn(backend.device, p, o)
    for gone in ("dx", "dgamma", "dbeta"):
        part = run_bn(backend.device, p, o, want=tuple(q for q in ("dx", "dgamma", "dbeta") if q != gone))
        assert part[gone] is None
        for q in BN_Q:
            if q != gone and full[q] is not None:
                assert _same_bits(part[q], full[q]), (gone, q)
    again = run_bn(backend.device, p, o, pads=(0, 0, 0, 0))  # two runs, other strides: the same bits
    for q in BN_Q:
        assert full[q] is None or _same_bits(again[q], full[q]), q


def test_batch_norm_of_one_row_in_training(backend):
    """torch refuses one value per channel in training mode.  The module path refuses as torch does; the C entry point
    itself is total: it normalises the row to beta with rstd = 1 / sqrt(eps) and feeds the (biased = 0) variance to
    running_var."""
    from reagent_amd.models import FullyConnectedNetwork

    dev = backend.device
    x = torch.tensor([[1.5, -2.0, 0.0]])
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        R.batch_norm_ref(x, None, None, None, None, True, 0.1, BN_EPS)
    net = FullyConnectedNetwork([3, 4, 2], ["relu", "linear"], use_batch_norm=True).to(dev)
    st = net.stack()
    st.stage_weights(need_transposed=True)
    xc, _ = st.stage_input(x.to(dev), need_transposed=True)
    bn = net.batch_norms()[0]
    before = (bn.running_mean.clone(), bn.running_var.clone(), bn.num_batches_tracked.clone())
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        st.forward(xc, torch.empty(1, 2, device=dev), save=True)
    assert torch.equal(bn.running_mean, before[0]) and torch.equal(bn.running_var, before[1])
    assert torch.equal(bn.num_batches_tracked, before[2])
    net.eval()  # eval mode takes one row, as torch does
    st.forward(xc, torch.empty(1, 2, device=dev), save=False)
    f = dict(dtype=F32, device=dev)
    y, sm, sr, rm, rv = torch.empty(1, 3, **f), torch.empty(3, **f), torch.empty(3, **f), torch.zeros(3, **f), torch.ones(3, **f)
    beta = torch.tensor([0.25, -1.0, 2.0], **f)
    ops.batch_norm_forward(x.to(dev), torch.ones(3, **f), beta, rm, rv, True, 0.1, BN_EPS, y, sm, sr, ops.batch_norm_workspace(1, 3, dev))
    assert torch.equal(sm.cpu(), x[0]) and torch.equal(y.cpu()[0], beta.cpu())
    assert torch.equal(sr.cpu(), torch.full((3,), float(np.float32(1.0 / math.sqrt(float(np.float32(BN_EPS)))))))
    assert torch.equal(rv.cpu(), torch.full((3,), float(np.float32(1.0) - np.float32(0.1))))


def test_batch_norm_refusals_by_code(backend):
    dev = backend.device
    t = torch.zeros(4096, device=dev)
    ptr, s, lib = t.data_ptr(), L.stream_ptr(), L.lib()
    assert lib.rg_batch_norm_workspace_bytes(0, 8) == 0 and lib.rg_batch_norm_workspace_bytes(8, 0) == 0
    need = lib.rg_batch_norm_workspace_bytes(2, 3)
    assert need == 2 * 3 * 8 + 2 * 3 * 4

    def fwd(B=2, n=3, x=ptr, gamma=ptr, beta=ptr, rm=ptr, rv=ptr, training=1, updates=1, y=ptr, sm=ptr, sr=ptr, ws=ptr, wsb=need):
        return lib.rg_batch_norm_forward(x, n, gamma, beta, rm, rv, training, updates, 0.1, BN_EPS, B, n, y, n, sm, sr, ws, wsb, s)

    def bwd(B=2, n=3, g=ptr, x=ptr, gamma=ptr, mean=ptr, rstd=ptr, rv=ptr, training=1, dx=ptr, dgamma=ptr, dbeta=ptr, ws=ptr, wsb=need):
        return lib.rg_batch_norm_backward(g, n, x, n, gamma, mean, rstd, rv, training, BN_EPS, B, n, dx, n, dgamma, dbeta, ws, wsb, s)

    assert fwd() == 0 and bwd() == 0 and fwd(training=0, ws=None, wsb=0, sm=None, sr=None) == 0 and bwd(training=0, rstd=None) == 0
    assert fwd(gamma=None, beta=None) == 0 and fwd(rm=None, rv=None) == 0 and fwd(updates=0) == 0 and bwd(gamma=None, rv=None) == 0
    for k in ("x", "y"):
        assert fwd(**{k: None}) == EINVAL, k
    assert fwd(sm=None) == EINVAL and fwd(sr=None) == EINVAL  # training needs both
    assert fwd(training=0, rm=None) == EINVAL and fwd(training=0, rv=None) == EINVAL  # eval needs the running statistics
    assert fwd(updates=-1) == EINVAL and fwd(training=0, updates=-1) == EINVAL
    for k in ("g", "x", "mean"):
        assert bwd(**{k: None}) == EINVAL, k
    assert bwd(rstd=None) == EINVAL and bwd(training=0, rv=None) == EINVAL
    assert bwd(dx=None, dgamma=None, dbeta=None) == EINVAL
    for call in (fwd, bwd):
        assert call(B=0) == EINVAL and call(B=-1) == EINVAL and call(n=0) == EINVAL and call(n=-1) == EINVAL
        assert call(ws=None) == EWORKSPACE and call(wsb=need - 1) == EWORKSPACE
    f = dict(dtype=F32, device=dev)
    x = torch.zeros(2, 3, **f)
    with pytest.raises(L.ReagentHipError, match=r"rg_batch_norm_forward failed.*code -1"):
        ops.batch_norm_forward(x, None, None, None, None, True, 0.1, BN_EPS, torch.empty_like(x), None, None, ops.batch_norm_workspace(2, 3, dev))
    with pytest.raises(L.ReagentHipError, match=r"rg_batch_norm_forward failed.*code -4"):
        ops.batch_norm_forward(x, None, None, None, None, True, 0.1, BN_EPS, torch.empty_like(x), x[0], x[1], torch.empty(8, dtype=F64, device=dev))
    with pytest.raises(L.ReagentHipError, match=r"rg_batch_norm_backward failed.*code -1"):
        ops.batch_norm_backward(x, x, None, x[0], None, None, True, BN_EPS, ops.batch_norm_workspace(2, 3, dev), torch.empty_like(x))


# ---- dropout ----------------------------------------------------------------------------------------------------------
def run_dropout(dev, x, p, seed=7, offset=3, keep=None, pads=(3, 5)):
    """-> (y, keep) on NaN-padded strided x and y; keep given: replayed (generate = 0), its bytes must stay"""
    B, n = x.shape
    xp, yp = Padded(dev, src=x, pad=pads[0]), Padded(dev, (B, n), pads[1])
    kbuf = torch.full((B * n + 8,), 7, dtype=torch.uint8, device=dev)
    k = kbuf[4:4 + B * n]
    if keep is not None:
        k.copy_(keep)
    ops.dropout(xp.v, p, k, yp.v, seed=seed, offset=offset, generate=keep is None)
    assert xp.intact() and yp.intact() and bool((kbuf[:4] == 7).all()) and bool((kbuf[4 + B * n:] == 7).all())
    assert keep is None or torch.equal(k.cpu(), keep.cpu())
    return yp.cpu(), k.cpu().clone()


def _binomial_ok(kept, total, p, sigmas=6.0):
    """the kept share lies within `sigmas` standard deviations of a Binomial(total, 1 - p) (plus the one count that 24-bit
    uniforms can shift the threshold by)"""
    return abs(kept - total * (1.0 - p)) <= sigmas * math.sqrt(total * p * (1.0 - p)) + total * 2.0 ** -24 + 1e-9


@pytest.mark.parametrize("B,n", [(1, 1), (1, 3), (2, 2), (1, 5), (5, 1), (31, 33), (1, 1025), (41, 25)])
@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
def test_dropout_against_the_statement(backend, B, n, p):
    dev = backend.device
    x = torch.randn(B, n, generator=torch.Generator().manual_seed(B * n))
    y, keep = run_dropout(dev, x, p)
    assert bool((keep <= 1).all())
    k = keep.view(B, n)
    assert torch.equal(y, R.dropout_ref(x, k, p, F32))  # one fp32 multiplication: exact
    # against float64: the scale and the product are rounded once each, half an ulp of the result apiece
    assert _maxabs(y.double() - R.dropout_ref(x, k, p, F64)) <= 2 * _ulp(_maxabs(R.dropout_ref(x, k, p, F64)))
    kept = int(keep.sum())
    assert _binomial_ok(kept, B * n, p) and (p > 0 or kept == B * n)
    y2, keep2 = run_dropout(dev, x, p, pads=(0, 1))  # the same (seed, offset), other strides: the same mask
    assert torch.equal(keep2, keep) and _same_bits(y2, y)
    g = torch.randn(B, n, generator=torch.Generator().manual_seed(5))
    y3, _ = run_dropout(dev, x, p, keep=keep)  # replay
    assert _same_bits(y3, y)
    dg, _ = run_dropout(dev, g, p, keep=keep)
    assert torch.equal(dg, R.dropout_ref(g, k, p, F32))
    if p > 0 and B * n >= 1023:
        _, keep4 = run_dropout(dev, x, p, offset=4)  # another offset: an independent mask, differing where exactly one keeps
        differ = int((keep4 != keep).sum())
        q = 2 * p * (1 - p)
        assert differ > 0 and abs(differ - B * n * q) <= 6.0 * math.sqrt(B * n * q * (1 - q))
        _, keep5 = run_dropout(dev, x, p, seed=8)
        assert not torch.equal(keep5, keep)


@pytest.mark.gpu
def test_dropout_second_trip_of_the_grid_stride_loop():
    """more than 4096 * 256 groups of four: replay and the kept share only"""
    B, n, p = 4099, 1025, 0.1
    assert (B * n + 3) // 4 > 4096 * 256
    x = torch.randn(B, n, generator=torch.Generator().manual_seed(1))
    y, keep = run_dropout("cuda", x, p)
    assert bool((keep <= 1).all()) and _binomial_ok(int(keep.sum()), B * n, p)
    tail = keep[4 * 4096 * 256:]  # drawn in the second trip
    assert _binomial_ok(int(tail.sum()), tail.numel(), p)
    y2, _ = run_dropout("cuda", x, p, keep=keep)
    assert _same_bits(y2, y) and torch.equal(y, R.dropout_ref(x, keep.view(B, n), p, F32))


def test_dropout_refusals_by_code(backend):
    dev = backend.device
    t = torch.zeros(64, device=dev)
    k = torch.zeros(64, dtype=torch.uint8, device=dev)
    ptr, s, lib = t.data_ptr(), L.stream_ptr(), L.lib()

    def call(B=2, n=3, p=0.5, x=ptr, keep=k.data_ptr(), y=ptr, generate=1):
        return lib.rg_dropout(x, n, B, n, p, generate, 1, 2, keep, y, n, s)

    assert call() == 0 and call(p=0.0) == 0 and call(generate=0) == 0
    for p in (-0.1, 1.0, 1.5, NAN, math.inf):
        assert call(p=p) == EINVAL, p
    for kw in (dict(x=None), dict(y=None), dict(keep=None), dict(B=0), dict(n=0), dict(B=-1)):
        assert call(**kw) == EINVAL, kw
    x = torch.zeros(2, 3, device=dev)
    with pytest.raises(L.ReagentHipError, match=r"rg_dropout failed.*code -1"):
        ops.dropout(x, 1.0, k, torch.empty_like(x))
