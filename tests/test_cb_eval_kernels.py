"""rg_cb_eval_ingest (reagent_amd/csrc/cb_eval.hip) against the torch statement of the reference's formulas
(reagent/evaluation/cb/utils.py:9-47, policy_evaluator.py:22-68, base_trainer.py:127-129) in fp32 and in float64, on the
interpreter and, under `-m gpu`, on the MI355X.  u = 2^-24.

Rows.  Where no exp is involved (no action_log_probability) importance_weight and effective_weight are BIT-EQUAL to the
torch fp32 statement: int -> float, two IEEE divisions, a compare, two multiplications, each rounded on its own.

Where exp is involved.  p = exp(logp) comes from two implementations, each documented to at most 1 ulp of the true value
(glibc expf on the interpreter: below 1 ulp; the device library's exp: 1 ulp; torch's vectorised CPU exp, Sleef u10: 1.0
ulp; torch's device exp is the device library's).  So the two p differ by at most 2 ulp(p) <= 2 * 2^-23 p, the two
quotients 1 / p by at most that relative amount plus one rounding (2^-24) each: 3 * 2^-23 relative, before second-order
terms.  One spacing of fp32 at x is between 2^-24 |x| and 2^-23 |x|, so that is between 3 and 6 spacings depending on where
1 / p lies in its binade.  Six spacings would let through an exp that is worse than documented wherever 1 / p lies low in
its binade, so the bound is also capped at 4 spacings, and what is asserted is the smaller of the two everywhere:
    |iw - iw_torch| <= min(3 * 2^-23 |iw_torch|, 4 spacing(iw_torch)),
and the same for effective_weight (its one further multiplication by w adds a rounding on each side: + 2^-23 relative in
the first term, still capped by 4 spacings).  A clipped row is exactly the clip on both sides.

Sums.  Each of the nine buffers is held to the any-order fp32 bound
    |S - S64| <= (B + 2) u sum|terms| + 2 u |buffer|
against the float64 statement, and torch's own fp32 sums are held to the same bound in the same test, so it is fair to the
reference.  The float64 statement of a sum takes the importance weights of the implementation it judges (ours, or
torch's): the bound is one of summation and of the two products a term is made of, not of exp -- the rows are held to
their own bound above.  Without exp the two sets of importance weights are the same bits anyway.
"""
import itertools
import os

import pytest
import torch

from kernel_remarks import HIPCC, kernel_resources

U = 2.0 ** -24
EINVAL = -1
F32, F64 = torch.float32, torch.float64
CLIP = 4.0
LITERAL_BROADCAST_MAX = 300  # above it the [B, B] product of the size quirk is not materialised (8200^2 doubles)
NAMES = ("sum_weight_all_data", "sum_reward_weighted_all_data", "sum_size_weighted_all_data",
         "sum_reward_importance_weighted_accepted", "sum_reward_weighted_accepted", "sum_weight_accepted",
         "sum_importance_weight_accepted", "sum_size_weighted_accepted", "sum_weight_since_update")


def _inputs(B, A, weighted, logp, presence, seed):
    """on the host: action, model_action [B, 1]; reward [B, 1]; weight, logp [B, 1] or None; presence [B, A] bool or None
    (the logged arm present)"""
    g = torch.Generator().manual_seed(seed)
    d = dict(action=torch.randint(0, A, (B, 1), generator=g), model_action=torch.randint(0, A, (B, 1), generator=g),
             reward=torch.randn(B, 1, generator=g), weight=None, logp=None, presence=None, arms=A)
    if weighted:
        d["weight"] = 0.5 + torch.rand(B, 1, generator=g)
    if logp:
        d["logp"] = torch.log(0.05 + 0.95 * torch.rand(B, 1, generator=g))  # 1 / p in [1, 20]: some above CLIP, some below
    if presence:
        m = torch.rand(B, A, generator=g) < 0.6
        m[torch.arange(B), d["action"].reshape(-1)] = True
        d["presence"] = m
    return d


def _rows(d, clip, dtype):
    """add_importance_weights (utils.py:9-47) as the reference writes it, in `dtype` -> importance_weight [B, 1]"""
    if d["logp"] is not None:
        prob = torch.exp(d["logp"].to(dtype))
    else:
        if d["presence"] is not None:
            sizes = d["presence"].sum(1, keepdim=True)
        else:
            sizes = torch.ones_like(d["action"]) * d["arms"]
        prob = (torch.ones_like(sizes) / sizes).to(dtype) if dtype == F32 else torch.ones_like(sizes).to(dtype) / sizes.to(dtype)
    iw = torch.ones_like(prob) / prob
    if clip is not None:
        iw = torch.clamp(iw, max=clip)
    return (d["action"] == d["model_action"]) * iw


def _sums(d, iw, dtype):
    """_process_all_data + _process_used_data (policy_evaluator.py:22-68) and the trainer's since-update sum, as the reference
    writes them (the [B, 1] sizes against the squeezed weights included), in `dtype` from the importance weights `iw`
    -> (the nine sums in NAMES' order, the nine sums of |terms|), float64 tensors"""
    reward = d["reward"].to(dtype)
    weights = d["weight"].to(dtype) if d["weight"] is not None else torch.ones_like(reward)
    iw = iw.to(dtype)
    eff = weights * iw
    acc = (iw > 0).to(dtype)
    if d["presence"] is not None:
        sizes = d["presence"].sum(1)
    else:
        sizes = torch.ones_like(reward) * d["arms"]
    terms = [weights, weights * reward, weights.squeeze() * sizes, eff * reward, weights * acc * reward, weights * acc, eff,
             (weights * acc).squeeze() * sizes, weights]
    B = reward.shape[0]
    if d["presence"] is None and B > LITERAL_BROADCAST_MAX:
        # the [B, B] product is B copies of one column: B * the column's sum (held against the literal product at every
        # smaller B of this file, where both are computed)
        col = [weights * d["arms"], weights * acc * d["arms"]]
        sums = [t.sum().double() for t in terms]
        abss = [t.double().abs().sum() for t in terms]
        for k, c in zip((2, 7), col):
            sums[k], abss[k] = B * c.sum().double(), B * c.double().abs().sum()
        return torch.stack(sums), torch.stack(abss)
    return (torch.stack([t.sum().double() for t in terms]), torch.stack([t.double().abs().sum() for t in terms]))


def _run(d, clip, dev, state=None):
    """the kernel through ops.cb_eval_ingest -> importance_weight, effective_weight [B, 1] and the nine buffers [9] (host)"""
    from reagent_amd import ops

    B = d["action"].shape[0]
    t = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in d.items()}
    if state is None:
        state = torch.zeros(9, dtype=F32, device=dev)
    out = torch.empty(2, B, 1, dtype=F32, device=dev)
    ops.cb_eval_ingest(t["action"].reshape(-1), t["model_action"].reshape(-1), t["reward"].reshape(-1),
                       None if t["weight"] is None else t["weight"].reshape(-1),
                       None if t["logp"] is None else t["logp"].reshape(-1), t["presence"], d["arms"], clip, out[0], out[1],
                       ops.cb_eval_partials(B, dev), [state[k:k + 1] for k in range(8)], state[8:])
    return out[0].cpu(), out[1].cpu(), state


def _spacing(x):
    x = x.abs().float()
    return (torch.nextafter(x, torch.full_like(x, float("inf"))) - x).double()


def _check_rows(got, ref, exp, rel, what):
    if not exp:
        assert torch.equal(got, ref), what
        return
    err = (got.double() - ref.double()).abs()
    bound = torch.minimum(rel * ref.double().abs(), 4 * _spacing(ref))
    assert (err <= bound).all(), (what, (err / bound.clamp_min(1e-300)).max().item())


def _check_sums(got, before, want, abs_terms, B, what):
    got, before = got.double().cpu(), before.double().cpu()
    ref = before + want
    bound = (B + 2) * U * abs_terms + 2 * U * ref.abs()
    err = (got - ref).abs()
    assert (err <= bound).all(), (what, [(n, e, b) for n, e, b in zip(NAMES, err.tolist(), bound.tolist()) if e > b])


def _check_combination(dev, B, A, weighted, logp, presence, clip, reruns=True):
    """one combination of weight / log-probability / arm_presence / clip at one shape: the rows, acceptance, the nine sums
    (ours and torch's own fp32 ones), the size quirk; with `reruns` a bit-identical second run and accumulation across two
    calls"""
    what = (B, A, weighted, logp, presence, clip)
    d = _inputs(B, A, weighted, logp, presence, 1000 * B + 10 * A + 4 * weighted + 2 * logp + presence)
    iw32 = _rows(d, clip, F32)
    w32 = d["weight"] if weighted else torch.ones(B, 1)
    iw, eff, state = _run(d, clip, dev)
    assert iw.shape == eff.shape == (B, 1) and iw.dtype == eff.dtype == F32
    _check_rows(iw, iw32, logp, 3 * 2.0 ** -23, what + ("importance_weight",))
    _check_rows(eff, w32 * iw32, logp, 4 * 2.0 ** -23, what + ("effective_weight",))
    assert torch.equal(eff, w32 * iw), what  # the product the trainers would otherwise form: the same bits
    # acceptance is exact, and it is the match of the two actions (1 / p > 0 for every row drawn here)
    assert torch.equal(iw > 0, iw32 > 0) and torch.equal(iw > 0, d["action"] == d["model_action"]), what
    if clip is not None:
        assert (iw <= clip).all() and torch.equal(iw == clip, iw32 == clip), what
        if B >= 257 and logp:
            assert (iw == clip).any() and ((iw > 0) & (iw < clip)).any(), what
    zero = torch.zeros(9, dtype=F64)
    want, abs_terms = _sums(d, iw, F64)
    _check_sums(state, zero, want, abs_terms, B, what + ("ours",))
    ref32, _ = _sums(d, iw32, F32)
    want_t, abs_t = _sums(d, iw32, F64)
    _check_sums(ref32, zero, want_t, abs_t, B, what + ("torch fp32",))
    # the size quirk: B * A * sum w without arm_presence, the plain sum with it
    sw = (d["weight"].double().sum() if weighted else torch.tensor(float(B), dtype=F64))
    if presence:
        plain = (w32.double().reshape(-1) * d["presence"].sum(1).double()).sum()
        assert abs(want[2] - plain) <= 1e-12 * plain
    else:
        assert abs(want[2] - B * A * sw) <= 1e-12 * B * A * sw
        assert abs(state[2].item() - B * A * sw.item()) <= (B + 2) * U * B * A * sw.item(), what
    if not reruns:
        return
    # a second run from the same state: the same bits; a second call on the first one's state: the sums add up
    iw2, eff2, state2 = _run(d, clip, dev)
    assert torch.equal(iw, iw2) and torch.equal(eff, eff2) and torch.equal(state, state2), what
    first = state.clone()
    _, _, state3 = _run(d, clip, dev, state=state)
    assert state3.data_ptr() == state.data_ptr()
    _check_sums(state3, first, want, abs_terms, B, what + ("second call",))
    assert (state3[0] > first[0]).item() and torch.equal(state3[0], state3[8]), what


@pytest.mark.parametrize("A", [1, 3, 8])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 257, 8200])  # 8200 rows: 33 slices, the finishing launch reads 32 a pass
def test_ingest_against_torch(backend, B, A):
    """all eight combinations of weight / log-probability / arm_presence x the clip on and off.  The interpreter needs about
    a second a launch at 8200 rows, so that size takes the two extreme combinations here (the reruns with everything given
    only) and three more in test_many_slices_with_the_other_paths"""
    combos = list(itertools.product(itertools.product((False, True), repeat=3), (None, CLIP)))
    if B > 257:
        combos = [combos[0], combos[-1]]
    for i, ((weighted, logp, presence), clip) in enumerate(combos):
        _check_combination(backend.device, B, A, weighted, logp, presence, clip, reruns=B <= 257 or i == 1)


@pytest.mark.parametrize("weighted,logp,presence,clip", [(False, False, True, None), (True, False, False, None),
                                                          (True, True, False, CLIP), (False, True, True, None)])
def test_many_slices_with_the_other_paths(backend, weighted, logp, presence, clip):
    """B = 8200, A = 3: the finishing launch's second pass with presence alone (plain sizes, no exp), with weights alone (the
    size quirk times weights), with log-probabilities and weights under the clip, and with log-probabilities and presence
    unclipped"""
    _check_combination(backend.device, 8200, 3, weighted, logp, presence, clip, reruns=False)


def test_quirk_is_the_references_number(backend):
    """the unmodified reference on B = 37, A = 4, one unweighted batch without arm_presence: sum_size_weighted_all_data_local
    = 5476 = 37 * 37 * 4 (exact in fp32; the torch statement of this file gives it too); with every arm marked present it
    is 37 * 4"""
    d = _inputs(37, 4, False, False, False, 5)
    _, _, state = _run(d, None, backend.device)
    assert state[2].item() == 5476.0 == _sums(d, _rows(d, None, F32), F32)[0][2].item()
    accepted = (d["action"] == d["model_action"]).sum().item()
    assert state[7].item() == 37 * 4 * accepted and state[5].item() == accepted and state[0].item() == 37
    d["presence"] = torch.ones(37, 4, dtype=torch.bool)
    _, _, state = _run(d, None, backend.device)
    assert state[2].item() == 37 * 4 and state[7].item() == 4 * accepted


def test_zero_probability_on_a_rejected_row_is_nan(backend):
    """logp = -inf on a rejected row with no clip: 0 * (1 / 0) = NaN in the reference, NaN here; with a clip it is 0 * clip.
    A NaN importance weight is not accepted (NaN > 0 is false) and poisons exactly the sums of the effective weight"""
    B, A = 70, 3
    d = _inputs(B, A, True, True, False, 11)
    d["action"][5], d["model_action"][5] = 0, 1  # rejected
    d["logp"][5] = float("-inf")
    d["action"][6], d["model_action"][6] = 2, 2  # accepted, probability 0: inf
    d["logp"][6] = float("-inf")
    d["action"][7], d["model_action"][7] = 0, 2  # rejected, logp NaN
    d["logp"][7] = float("nan")
    iw32 = _rows(d, None, F32)
    assert torch.isnan(iw32[5]) and torch.isinf(iw32[6]) and torch.isnan(iw32[7])
    iw, eff, state = _run(d, None, backend.device)
    assert torch.isnan(iw[5]) and torch.isinf(iw[6]) and torch.isnan(iw[7]) and torch.isnan(eff[5])
    keep = torch.ones(B, dtype=torch.bool)
    keep[5:8] = False
    _check_rows(iw[keep], iw32[keep], True, 3 * 2.0 ** -23, "the other rows")
    ref32, _ = _sums(d, iw32, F32)
    nan = torch.isnan(state.cpu())
    assert torch.equal(nan, torch.isnan(ref32)) and nan.tolist() == [False, False, False, True, False, False, True, False, False]
    want, abs_terms = _sums(d, iw, F64)
    ok = ~nan
    _check_sums(state.cpu()[ok], torch.zeros(9, dtype=F64)[ok], want[ok], abs_terms[ok], B, "the sums without a NaN")
    iw_c, _, _ = _run(d, CLIP, backend.device)
    ref_c = _rows(d, CLIP, F32)
    assert iw_c[5].item() == 0.0 == ref_c[5].item() and iw_c[6].item() == CLIP == ref_c[6].item()
    assert torch.isnan(iw_c[7]) and torch.isnan(ref_c[7])  # torch.clamp passes a NaN, and so does the kernel


def test_add_importance_weights_is_the_kernels(backend):
    """the public function (the reference's signature) on a CBInput: the kernel's rows, no evaluator state needed"""
    from reagent_amd.core.types import CBInput
    from reagent_amd.evaluation.cb.utils import add_importance_weights

    dev = backend.device
    B, A = 65, 5
    d = _inputs(B, A, True, False, True, 3)
    batch = CBInput(context_arm_features=torch.zeros(B, A, 2, device=dev), action=d["action"].to(dev),
                    reward=d["reward"].to(dev), weight=d["weight"].to(dev), arm_presence=d["presence"].to(dev))
    for clip in (None, 2.0):
        new = add_importance_weights(batch, d["model_action"].to(dev), clip)
        assert new is not batch and batch.importance_weight is None and new.weight is batch.weight
        assert torch.equal(new.importance_weight.cpu(), _rows(d, clip, F32))
    with pytest.raises(AssertionError):
        add_importance_weights(batch, d["model_action"].reshape(-1).to(dev))


def test_einval(backend):
    import reagent_amd._lib as L

    lib, dev, p = L.lib(), backend.device, L.ptr
    B, A = 8, 3
    i64 = torch.zeros(B, dtype=torch.int64, device=dev)
    f = torch.zeros(B, dtype=F32, device=dev)
    out = torch.zeros(2, B, dtype=F32, device=dev)
    part = torch.zeros(8, dtype=F64, device=dev)
    state = torch.zeros(9, dtype=F32, device=dev)

    def call(B_=B, A_=A, null=None):
        ptrs = [p(i64), p(i64), p(f), None, None, None, p(out[0]), p(out[1]), p(part)] + [p(state[k:k + 1]) for k in range(9)]
        if null is not None:
            ptrs[null] = None
        return lib.rg_cb_eval_ingest(*ptrs[:6], B_, A_, 0, 0.0, *ptrs[6:], None)

    assert call(B_=0) == EINVAL and call(B_=-2) == EINVAL and call(A_=0) == EINVAL
    for null in (0, 1, 2, 6, 7, 8) + tuple(range(9, 18)):
        assert call(null=null) == EINVAL, null
    assert not state.any()  # none of the refused calls ran
    assert call() == 0 and state[0].item() == B
    assert lib.rg_cb_eval_ingest_partials(0) == 0 and lib.rg_cb_eval_ingest_partials(256) == 1
    assert lib.rg_cb_eval_ingest_partials(257) == 2 and lib.rg_cb_eval_ingest_partials(8200) == 33


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_cb_eval_kernels_have_no_scratch(tmp_path):
    """cb_eval.hip compiled for gfx950 with the resource remarks on: no scratch, no spilled register, and the LDS the two
    kernels declare (4 waves x 8 doubles; 256 doubles)"""
    kernels = kernel_resources("cb_eval.hip", tmp_path)
    for want, lds in (("cb_eval_ingest_kernel", 4 * 8 * 8), ("cb_eval_finish_kernel", 256 * 8)):
        (k,) = [k for k in kernels if want in k]
        v = kernels[k]
        assert v.get("VGPRs Spill", 0) == 0 and v.get("SGPRs Spill", 0) == 0 and v["ScratchSize [bytes/lane]"] == 0, (k, v)
        assert v["LDS Size [bytes/block]"] == lds and v["VGPRs"] <= 64, (k, v)
    assert len(kernels) == 2, list(kernels)
