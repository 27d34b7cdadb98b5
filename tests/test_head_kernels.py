"""rg_qr_head, rg_c51_head, rg_cpe_head and rg_bcq_filter against the float64 statements of tests/head_refs.py, at the
smallest shapes where each loop structure of heads.hip changes behaviour: a second trip of the 64- and 256-stride loops
(N = 65, 257), the LDS caps (N = 1024, A = 256), C51's one-atom-per-lane branch with all eight slots per wave and a second
sweep (N = 64, A = 256), a second workgroup and its `b >= batch` tail (B = 257, 513, 700).

Every launch reads its inputs from `[:B]` views of buffers whose extra row is NaN and writes into `[:B]` views of buffers
whose extra row holds a sentinel; every case is launched twice into separate outputs, which must be bit-identical.

The bounds are not derived from the kernels: QR / C51 use the ones tests/fuzz/fuzz_heads.py holds them to, the CPE losses
and gradients the forms that fuzzer applies to the DQN head (same arithmetic per element), the propensities two roundings of
the exponent's argument plus a few ulps for expf and the division.  Each test prints `HEADERR <kernel> <output> <error>
<bound>` lines before it asserts (pytest -s / -rP shows them).

Worst share of its bound at these shapes, MI355X (the interpreter gives the same figures to within a few per cent):
  QR   loss 0.5 %   dq 30 % (N = 1024, A = 5)    all_q 0.1 %
  C51  loss 4 %     dq 43 % (N = 1024, A = 5)    all_q 2 %
  CPE  losses 0.5 % gradients 3 %                propensities 5 % (3.4e-7 of 6.7e-6 at T = 0.35, A = 33)
  BCQ  at most 1.2e-4 of a case's entries lie in the exempt band around the step (cap 1e-3)"""
import pytest
import torch
import torch.nn.functional as F

import head_refs as R
import reagent_amd._lib as L
from reagent_amd import ops

SENTINEL = -777.25
NAN = float("nan")
EINVAL = -1  # RG_EINVAL

_REF_CACHE = {}


# ---- guarded buffers ----------------------------------------------------------------------------
def _in(x, dev):
    """x on the device as the leading view of a buffer whose one extra row (element, for vectors) is NaN"""
    if x is None:
        return None
    buf = torch.full((x.shape[0] + 1,) + tuple(x.shape[1:]), NAN, dtype=x.dtype)
    buf[:-1] = x
    v = buf.to(dev)[:-1]
    assert v.is_contiguous() and v.shape == x.shape
    return v


class _Out:
    """[:rows] view of a buffer with one extra guard row filled with a sentinel"""

    def __init__(self, dev, rows, cols=None, fill=SENTINEL):
        shape = (rows + 1,) if cols is None else (rows + 1, cols)
        self.buf = torch.full(shape, fill, dtype=torch.float32).to(dev)
        self.view = self.buf[:rows]
        self.fill = fill

    def cpu(self):
        guard = self.buf[-1:].cpu()
        assert torch.equal(guard, torch.full_like(guard, self.fill)), "guard row written"
        return self.view.cpu()


def _report(kernel, output, err, bound, case):
    print(f"HEADERR {kernel} {output} {err:.3e} {bound:.3e} ({100 * err / bound:.0f} %) {case}")


def _twice(launch):
    a, b = launch(), launch()
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), f"{k}: two launches differ"
        assert not torch.isnan(a[k]).any(), f"{k}: NaN (a read past the end of an input?)"
    return a


# ---- QR / C51: shared case construction ---------------------------------------------------------
PLANTS = ("tie", "tie_masked", "all_masked")


def _atom_case(kind, seed, B, A, N, maxq, double_q, scale, boosts, gexp, plant, gamma, quarters=False, qrange=None):
    """Host inputs of one QR / C51 case.  Planted rows (maxq, double-Q) come first: two actions with bit-identical online
    rows and different target rows (the lower index must win), the same with the lower index masked (the other must
    win), a fully masked row (fp32: every key is -1e9, action 0 wins)."""
    g = torch.Generator().manual_seed(seed)
    q, qo, qt = (torch.randn(B, A * N, generator=g) * scale for _ in range(3))
    if quarters:  # td == 0 sits on the quantile indicator's edge
        q, qt = (q * 4).round() / 4, (qt * 4).round() / 4
    act = F.one_hot(torch.randint(0, A, (B,), generator=g), A).float()
    if maxq:
        mask = (torch.rand(B, A, generator=g) < 0.6).float()
        mask[torch.arange(B), torch.randint(0, A, (B,), generator=g)] = 1.0  # every ordinary row keeps a possible action
    else:
        mask = F.one_hot(torch.randint(0, A, (B,), generator=g), A).float()  # SARSA: the logged next action
    nt = (torch.rand(B, generator=g) < 0.8).float()
    if kind == "qr":
        reward = (torch.randn(B, generator=g) * 4).round() / 4
    else:
        reward = torch.randn(B, generator=g) * (qrange[1] - qrange[0]) / 4
        reward[torch.rand(B, generator=g) < 0.3] = 0.0
    planted = []
    if plant:
        assert maxq and double_q and A >= 2 and B >= 2
        for row, what in enumerate(PLANTS[:min(3, B - 1)]):
            nt[row] = 1.0
            if what == "all_masked":
                mask[row] = 0.0
                planted.append((row, what, 0))
                continue
            lo, hi = sorted(torch.randperm(A, generator=g)[:2].tolist())
            v = qo.view(B, A, N)
            v[row] *= 0.05  # the other actions stay clear of the pair
            if kind == "qr":
                common = torch.randn(N, generator=g) * scale + 10 * scale
            else:
                common = torch.randn(N, generator=g) * 0.05
                common[-1] += 12.0  # nearly all mass on the top atom: expected value ~ qmax
            v[row, lo] = common
            v[row, hi] = common
            mask[row] = (torch.rand(A, generator=g) < 0.6).float()
            mask[row, hi] = 1.0
            mask[row, lo] = 1.0 if what == "tie" else 0.0
            planted.append((row, what, lo if what == "tie" else hi))
    first = len(planted)  # first ordinary row
    if B - first >= 2:
        nt[B - 1], nt[first] = 0.0, 1.0  # a terminal and a non-terminal ordinary row
        if not maxq:
            mask[B - 1] = 0.0  # SARSA: a terminal transition logs no next action (C51: the projected mass sums to 0, not 1)
    if kind == "c51" and B - first >= 1:
        reward[first] = 0.0  # reward 0, not terminal: with gamma 1 every target atom lands exactly on the grid
        if B - first >= 2:
            reward[B - 1] = 0.0  # reward 0, terminal: every atom lands on the grid point of 0 (where 0 is one)
    return dict(kind=kind, B=B, A=A, N=N, maxq=maxq, double_q=double_q, gamma=gamma, q=q, qo=qo if double_q else None, qt=qt,
                act=act, mask=mask, reward=reward, nt=nt, boosts=torch.randn(A, generator=g) if boosts else None,
                gexp=torch.randint(1, 4, (B,), generator=g).float() if gexp else None, planted=planted, qrange=qrange,
                quant=((0.5 + torch.arange(N)) / float(N)).float(),
                support=torch.linspace(qrange[0], qrange[1], N) if qrange else None)


def _atom_ref(key, c):
    if key in _REF_CACHE:
        return _REF_CACHE[key]
    fp32_rows = [row for row, what, _ in c["planted"] if what == "all_masked"]
    if c["kind"] == "qr":
        ref = R.qr_head_ref(c["q"], c["qo"], c["qt"], c["act"], c["mask"], c["reward"], c["boosts"], c["nt"], c["gamma"],
                            c["gexp"], c["quant"], c["N"], c["maxq"], fp32_rows)
    else:
        ref = R.c51_head_ref(c["q"], c["qo"], c["qt"], c["act"], c["mask"], c["reward"], c["boosts"], c["nt"], c["gamma"],
                             c["gexp"], c["support"], c["qrange"][0], c["qrange"][1], c["N"], c["maxq"], fp32_rows)
    if c["maxq"]:  # on the reference alone: the choice of every row is beyond what fp32 rounding of the selection can move
        sel, mask = ref["select"], c["mask"].double()
        for row, what, winner in c["planted"]:
            assert int(ref["next_idx"][row]) == winner, (row, what)
        ordinary = torch.arange(len(c["planted"]), c["B"])
        if len(ordinary):
            assert (mask[ordinary].sum(1) >= 1).all()
            key_ = sel[ordinary] + R.NOT_POSSIBLE * (1 - mask[ordinary])
            top = key_.topk(min(2, c["A"]), dim=1).values
            gap = top[:, 0] - top[:, 1] if c["A"] > 1 else torch.full((len(ordinary),), float("inf"), dtype=torch.float64)
            need = 1e-4 * max(1.0, sel.abs().max().item())
            assert (gap > need).all(), f"arg-max gap {gap.min().item():.3e} <= {need:.3e}: replace the seed"
    _REF_CACHE[key] = ref
    return ref


def _atom_launch(c, dev, want_all_q):
    B, A, N = c["B"], c["A"], c["N"]
    ins = [_in(c[k], dev) for k in ("q", "qo", "qt", "act", "mask", "reward", "boosts", "nt")]
    gexp, tail = _in(c["gexp"], dev), _in(c["quant"] if c["kind"] == "qr" else c["support"], dev)

    def launch():
        dq, parts, allq = _Out(dev, B, A * N), _Out(dev, B), _Out(dev, B, A)
        aq = allq.view if want_all_q else None
        if c["kind"] == "qr":
            ops.qr_head(*ins, c["gamma"], gexp, tail, N, c["maxq"], dq.view, parts.view, aq)
        else:
            ops.c51_head(*ins, c["gamma"], gexp, tail, c["qrange"][0], c["qrange"][1], N, c["maxq"], dq.view, parts.view, aq)
        out = dict(dq=dq.cpu(), parts=parts.cpu(), all_q=allq.cpu())
        if not want_all_q:
            assert torch.equal(out.pop("all_q"), torch.full((B, A), SENTINEL))
        return out

    return _twice(launch)


#            N     A   B  maxq   double boosts gexp  plant  gamma scale allq   quarters
QR_CASES = [(1,    5,  5, True,  True,  True,  True,  True,  0.9, 1.0, True,  False),
            (63,   33, 5, True,  False, False, False, False, 0.9, 5.0, False, False),
            (64,   5,  3, False, False, True,  False, False, 0.9, 1.0, True,  False),
            (65,   256, 3, True, True,  False, False, True,  1.0, 1.0, True,  False),
            (255,  33, 3, True,  True,  False, False, False, 1.0, 1.0, True,  True),
            (256,  5,  5, False, True,  False, True,  False, 0.9, 0.2, False, False),
            (257,  33, 3, True,  True,  False, False, True,  0.9, 5.0, True,  False),
            (1024, 5,  3, True,  True,  True,  True,  False, 0.9, 1.0, True,  False),
            (65,   1,  5, True,  False, False, False, False, 1.0, 1.0, True,  True),
            (255,  3,  1, False, False, False, False, False, 0.0, 1.0, True,  False),
            (257,  4,  3, True,  False, True,  False, False, 0.9, 0.2, True,  False),
            (64,   4,  5, True,  True,  False, True,  True,  1.0, 5.0, True,  True),
            (1024, 256, 1, True, True,  False, False, False, 0.9, 1.0, True,  False)]


@pytest.mark.parametrize("case", range(len(QR_CASES)), ids=lambda i: "N%d-A%d-B%d" % QR_CASES[i][:3])
def test_qr_head_against_float64(backend, case):
    N, A, B, maxq, double_q, boosts, gexp, plant, gamma, scale, want_all_q, quarters = QR_CASES[case]
    c = _atom_case("qr", 4100 + case, B, A, N, maxq, double_q, scale, boosts, gexp, plant, gamma, quarters)
    ref = _atom_ref(("qr", case), c)
    got = _atom_launch(c, backend.device, want_all_q)
    tag = dict(N=N, A=A, B=B)
    loss, lref = got["parts"].double().sum().item(), ref["loss"].item()
    gs = max(1e-30, ref["dq"].abs().max().item())
    errs = [("loss", abs(loss - lref), 2e-5 * max(1.0, abs(lref))),
            ("dq", (got["dq"].double() - ref["dq"]).abs().max().item(), 3e-5 * gs + 1e-9)]
    if want_all_q:
        errs.append(("all_q", (got["all_q"].double() - ref["all_q"]).abs().max().item(), 1e-5 * max(1.0, c["q"].abs().max().item())))
    for name, err, bound in errs:
        _report("qr", name, err, bound, tag)
    for name, err, bound in errs:
        assert err <= bound, (name, err, bound)
    # d loss / d q lives in the logged action's atoms only
    assert torch.equal(got["dq"].view(B, A, N) * (1 - c["act"]).unsqueeze(-1), torch.zeros(B, A, N))


#             N     A    B  range          maxq   double boosts gexp  plant  gamma scale allq
C51_CASES = [(2,    5,   5, (0.0, 5.0),     True,  True,  False, False, True,  1.0, 1.0, True),
             (51,   37,  5, (-10.0, 10.0),  True,  False, False, False, False, 0.9, 4.0, True),
             (64,   37,  4, (-100.0, 200.0), True, True,  False, False, True,  1.0, 1.0, True),
             (64,   256, 3, (-10.0, 10.0),  True,  True,  True,  False, True,  0.9, 1.0, True),
             (65,   32,  3, (0.0, 5.0),     False, False, False, True,  False, 1.0, 0.2, True),
             (255,  33,  3, (-10.0, 10.0),  True,  True,  False, False, True,  1.0, 1.0, True),
             (257,  37,  3, (-100.0, 200.0), True, False, False, False, False, 0.5, 4.0, False),
             (1024, 5,   2, (-10.0, 10.0),  True,  True,  True,  True,  False, 1.0, 1.0, True),
             (65,   1,   5, (-10.0, 10.0),  True,  False, False, False, False, 1.0, 1.0, True),
             (257,  4,   3, (0.0, 5.0),     False, True,  False, False, False, 1.0, 1.0, True),
             (65,   256, 1, (0.0, 5.0),     True,  True,  False, True,  False, 0.9, 4.0, False),
             (64,   4,   5, (-100.0, 200.0), False, False, False, False, False, 1.0, 1.0, True),
             (1024, 33,  1, (0.0, 5.0),     True,  False, False, False, False, 1.0, 0.2, True),
             (1024, 256, 1, (-10.0, 10.0),  True,  True,  False, False, False, 0.9, 1.0, True)]


@pytest.mark.parametrize("case", range(len(C51_CASES)), ids=lambda i: "N%d-A%d-B%d" % C51_CASES[i][:3])
def test_c51_head_against_float64(backend, case):
    N, A, B, qrange, maxq, double_q, boosts, gexp, plant, gamma, scale, want_all_q = C51_CASES[case]
    c = _atom_case("c51", 5100 + case, B, A, N, maxq, double_q, scale, boosts, gexp, plant, gamma, qrange=qrange)
    ref = _atom_ref(("c51", case), c)
    got = _atom_launch(c, backend.device, want_all_q)
    tag = dict(N=N, A=A, B=B, range=qrange)
    loss, lref = got["parts"].double().sum().item(), ref["loss"].item()
    gs = max(1e-30, ref["dq"].abs().max().item())
    errs = [("loss", abs(loss - lref), 5e-5 * max(1.0, abs(lref))),
            ("dq", (got["dq"].double() - ref["dq"]).abs().max().item(), 2e-4 * gs + 1e-9)]
    if want_all_q:
        errs.append(("all_q", (got["all_q"].double() - ref["all_q"]).abs().max().item(),
                     2e-5 * max(1.0, abs(qrange[0]), abs(qrange[1]))))
    for name, err, bound in errs:
        _report("c51", name, err, bound, tag)
    for name, err, bound in errs:
        assert err <= bound, (name, err, bound)
    assert torch.equal(got["dq"].view(B, A, N) * (1 - c["act"]).unsqueeze(-1), torch.zeros(B, A, N))


def test_atom_head_limits(backend):
    """one atom or action past the LDS caps is RG_EUNSUPPORTED, a single atom is RG_EINVAL for C51: an error, nothing written"""
    dev = backend.device
    for head, A, N, code in (("qr", 1, 1025, L.EUNSUPPORTED), ("c51", 1, 1025, L.EUNSUPPORTED), ("qr", 257, 1, L.EUNSUPPORTED),
                             ("c51", 257, 2, L.EUNSUPPORTED), ("c51", 3, 1, EINVAL)):
        B = 2
        q = _in(torch.zeros(B, A * N), dev)
        act = _in(F.one_hot(torch.zeros(B, dtype=torch.int64), A).float(), dev)
        vec, tail = _in(torch.ones(B), dev), _in(torch.linspace(0.0, 1.0, N), dev)
        dq, parts, allq = _Out(dev, B, A * N), _Out(dev, B), _Out(dev, B, A)
        with pytest.raises(L.ReagentHipError, match=r"\(code %d\)" % code):
            if head == "qr":
                ops.qr_head(q, q, q, act, act, vec, None, vec, 0.9, None, tail, N, True, dq.view, parts.view, allq.view)
            else:
                ops.c51_head(q, q, q, act, act, vec, None, vec, 0.9, None, tail, 0.0, 1.0, N, True, dq.view, parts.view,
                             allq.view)
        for o in (dq, parts, allq):
            assert torch.equal(o.cpu(), torch.full_like(o.cpu(), SENTINEL)), (head, A, N)


# ---- rg_cpe_head --------------------------------------------------------------------------------
#             B    A   M  temp  loss     gamma gexp   scale
CPE_CASES = [(1,   1,  1, 1.0,  "mse",   0.9,  False, 1.0),
             (1,   7,  4, 0.35, "huber", 1.0,  False, 0.3),
             (2,   3,  2, 0.35, "huber", 1.0,  True,  0.3),
             (2,   2,  1, 10.0, "mse",   0.0,  False, 3.0),
             (255, 7,  4, 10.0, "huber", 0.9,  False, 3.0),
             (256, 2,  2, 1.0,  "mse",   0.0,  True,  1.0),
             (257, 33, 1, 0.35, "huber", 0.9,  True,  1.0),
             (257, 1,  2, 1.0,  "huber", 1.0,  False, 30.0),
             (513, 3,  4, 1.0,  "huber", 1.0,  False, 0.3),
             (700, 7,  2, 10.0, "mse",   0.9,  True,  30.0),
             (700, 33, 4, 0.35, "huber", 0.9,  False, 1.0)]


@pytest.mark.parametrize("case", range(len(CPE_CASES)), ids=lambda i: "B%d-A%d-M%d" % CPE_CASES[i][:3])
def test_cpe_head_against_float64(backend, case):
    B, A, M, temp, loss, gamma, gexp, scale = CPE_CASES[case]
    dev = backend.device
    g = torch.Generator().manual_seed(6100 + case)
    reward_est, q_cpe, tgt_next = (torch.randn(B, M * A, generator=g) * scale for _ in range(3))
    scores = torch.randn(B, A, generator=g) * 2.0
    mask = (torch.rand(B, A, generator=g) < 0.6).float()
    mask[torch.rand(B, generator=g) < 0.1] = 0.0  # about a tenth of the rows fully masked: 0 / 0 -> a zero row
    flat = torch.rand(B, generator=g) < 0.1       # rows whose scores are all equal
    scores[flat] = scores[flat][:, :1].expand(-1, A).clone()
    if B >= 2:
        mask[0], mask[1] = 0.0, 1.0
        scores[1] = scores[1, 0]
    act = F.one_hot(torch.randint(0, A, (B,), generator=g), A).float()
    reward = torch.randn(B, generator=g) * scale
    extra = torch.randn(B, M - 1, generator=g) * scale if M > 1 else None
    nt = (torch.rand(B, generator=g) < 0.8).float()
    if B >= 2:
        nt[0], nt[B - 1] = 1.0, 0.0
    gx = torch.randint(1, 4, (B,), generator=g).float() if gexp else None
    ref = _REF_CACHE.get(("cpe", case))
    if ref is None:
        ref = _REF_CACHE[("cpe", case)] = R.cpe_head_ref(reward_est, q_cpe, tgt_next, scores, mask, act, reward, extra, nt,
                                                          gamma, gx, temp, M, loss)
    ins = [_in(t, dev) for t in (reward_est, q_cpe, tgt_next, scores, mask, act, reward, extra, nt)]
    gxd = _in(gx, dev)
    P = ops.dqn_head_partials(B)
    assert P == (B + 255) // 256

    def launch(with_prop=True):
        dre, dqc = _Out(dev, B, M * A, fill=3.5), _Out(dev, B, M * A, fill=3.5)  # the kernel zeroes what it does not set
        rp, cp, prop = _Out(dev, P), _Out(dev, P), _Out(dev, B, A)
        assert rp.view.numel() == P and cp.view.numel() == P
        ops.cpe_head(*ins, gamma, gxd, temp, M, L.LOSS[loss], dre.view, dqc.view, rp.view, cp.view,
                     prop.view if with_prop else None)
        out = dict(d_reward_est=dre.cpu(), d_q_cpe=dqc.cpu(), reward_parts=rp.cpu(), cpe_parts=cp.cpu(), prop=prop.cpu())
        if not with_prop:
            assert torch.equal(out.pop("prop"), torch.full((B, A), SENTINEL))
        return out

    got = _twice(launch)
    without = launch(with_prop=False)
    for k in without:
        assert torch.equal(without[k], got[k]), f"{k} depends on propensities_out"
    tag = dict(B=B, A=A, M=M, T=temp, loss=loss)
    vscale = max(1.0, reward_est.abs().max().item(), q_cpe.abs().max().item(), tgt_next.abs().max().item())
    errs = []
    for name, parts, want in (("reward_loss", "reward_parts", "reward_loss"), ("cpe_loss", "cpe_parts", "cpe_loss")):
        val, w = got[parts].double().sum().item() / (B * M), ref[want].item()
        errs.append((name, abs(val - w), 2e-5 * max(1.0, abs(w))))
    for name in ("d_reward_est", "d_q_cpe"):
        errs.append((name, (got[name].double() - ref[name]).abs().max().item(),
                     2e-6 * max(1.0, ref[name].abs().max().item()) + 1e-7 * vscale))
    errs.append(("propensities", (got["prop"].double() - ref["propensities"]).abs().max().item(),
                 4 * 2.0 ** -24 * ((scores / temp).abs().max().item() + 4)))
    for name, err, bound in errs:
        _report("cpe", name, err, bound, tag)
    for name, err, bound in errs:
        assert err <= bound, (name, err, bound)
    # exactly zero outside the logged action's column of every metric; a zero row where nothing is possible
    off = (1 - act).unsqueeze(1).expand(B, M, A).reshape(B, M * A)
    for name in ("d_reward_est", "d_q_cpe"):
        assert torch.equal(got[name] * off, torch.zeros(B, M * A)), name
    assert torch.equal(got["prop"][mask.sum(1) == 0], torch.zeros(int((mask.sum(1) == 0).sum()), A))
    assert torch.equal(got["prop"] * (1 - mask), torch.zeros(B, A))


def test_cpe_head_checks_partial_lengths(backend):
    """ops.cpe_head refuses partial buffers shorter than dqn_head_partials(B) (the kernel would write past them)"""
    dev, B, A = backend.device, 257, 2
    z = torch.zeros(B, A, device=dev)
    act = F.one_hot(torch.zeros(B, dtype=torch.int64), A).float().to(dev)
    v = torch.zeros(B, device=dev)
    for short_r, short_c in ((1, 2), (2, 1)):
        with pytest.raises(AssertionError):
            ops.cpe_head(z, z, z, z, act, act, v, None, v, 0.9, None, 1.0, 1, L.LOSS["mse"], torch.empty_like(z), torch.empty_like(z),
                         torch.empty(short_r, device=dev), torch.empty(short_c, device=dev))


# ---- rg_bcq_filter ------------------------------------------------------------------------------
BCQ_SHAPES = [(1, 1), (1, 5), (255, 2), (256, 33), (257, 5), (257, 1), (700, 33), (700, 2)]
BCQ_THRESHOLDS = (0.0, 0.05, 0.3, 0.6, 1.0)
BCQ_SCALES = (0.3, 2.0, 10.0)
BCQ_BAND = 1e-5


@pytest.mark.parametrize("B,A", BCQ_SHAPES)
def test_bcq_filter_against_float64(backend, B, A):
    dev = backend.device
    g = torch.Generator().manual_seed(7100 + 40 * B + A)
    worst_share = 0.0
    for scale in BCQ_SCALES:
        logits = torch.randn(B, A, generator=g) * scale
        if A >= 2:  # in about a third of the rows a second entry ties with the maximum bit for bit
            rows = torch.nonzero(torch.rand(B, generator=g) < 0.34).reshape(-1)
            if B == 1:
                rows = torch.tensor([0])
            other = (logits[rows].argmax(1) + torch.randint(1, A, (len(rows),), generator=g)) % A
            logits[rows, other] = logits[rows].max(1).values
        mask = (torch.rand(B, A, generator=g) < 0.7).float()
        logits_d = _in(logits, dev)
        for thr in BCQ_THRESHOLDS:
            want, ratio = R.bcq_filter_ref(logits, thr, mask)
            # on the reference alone: the step's band holds at most 0.1 % of the case's entries.  Row maxima (ratio == 1,
            # planted ties included) are not in it: they survive every threshold exactly.
            band = ((ratio - float(torch.tensor(thr, dtype=torch.float32))).abs() <= BCQ_BAND) & (ratio != 1.0)
            if thr == 0.0:
                band = torch.zeros_like(band)
            assert band.sum().item() <= max(0, int(1e-3 * B * A)), (B, A, scale, thr, band.sum().item())
            worst_share = max(worst_share, band.sum().item() / (B * A))

            def launch():
                out = _Out(dev, B, A, fill=7.0)
                out.view.copy_(mask.to(dev))
                ops.bcq_filter(logits_d, thr, out.view)
                return dict(mask=out.cpu())

            got = _twice(launch)["mask"]
            assert torch.equal(got * (1 - mask), torch.zeros(B, A)), "a 0 of the incoming mask must stay 0"
            assert ((got == 0) | (got == 1)).all()
            if thr == 0.0:
                assert torch.equal(got, mask), (scale, thr)
            top = ratio == 1.0  # the row's maximal entries, bit-for-bit ties included, survive every threshold up to 1
            assert torch.equal(got[top], mask[top]), (scale, thr)
            assert torch.equal(got.double()[~band], want[~band]), (scale, thr, int((got.double() != want)[~band].sum()))
    print(f"HEADERR bcq band-share {worst_share:.3e} 1.000e-03 B={B} A={A}")
