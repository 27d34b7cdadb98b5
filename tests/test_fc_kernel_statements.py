"""The FullyConnected GEMM entry points (reagent_amd/csrc/fc.hip on rg_gemm.h: rg_fc_forward, rg_fc_dgrad, rg_fc_wgrad,
rg_act_backward, rg_transpose_cast) held to the statements of tests/fc_refs.py at every tile, slab and alignment edge.

Exact statements.  Integer operands of magnitude <= 4 (K * 16 + 4 < 2^24, so every partial sum is an fp32 integer in any
order and through any MFMA) must give the int64 product; one-hot operands must hand a real operand through bit for bit.
Equality is of VALUES where the statement is an integer (a masked product may carry the sign of what it masked: -0.0),
of BITS between two runs or two paths of the kernels.

Float64 statements.  |got - ref| <= (2 K + 4) u S_ij + 2^-126 per ELEMENT (fc_refs.py), times |act'(h)| in the backward,
one ulp for leaky_relu's product and A_act u max(|ref|, 2^-126) for tanh, sigmoid and softplus; a bf16 output, rounded
from an fp32 value within that bound bd, is held to bd (1 + 2^-8) + 2^-8 |ref| (fc_refs.bf16_rounded: bf16's unit roundoff
is 2^-8) and is bit for bit the cast of the fp32 output.  A_act is measured, not chosen: 4 x the largest error, in units of
u |ref|, of torch's own fp32 activation and of its fp32 backward through the output, over the pre-activations of the cases
of this file (measured_A_act below), and may not exceed twice the values profiles/NOTES_r31.md records.  Nothing else is a
tolerance.

Where the interpreter runs less than the MI355X, for its time, the list of cases says so itself (cases(), gemm_calls(),
WGRAD_ROWS, CHAIN_ROWS): every id that is collected runs what its name says.

Every operand is a view into a NaN-filled parent and every output a view into a sentinel-filled one (fc_refs.Box): after a
call the parent outside the view holds its filling, bit for bit, the operands are unchanged and every output element is
written.  Every line "RATIO ..." printed is the worst kernel error / bound of one output of one call."""
import functools
import itertools

import pytest
import torch

import fc_refs as R
import reagent_amd._lib as L
from fc_refs import BF16, F32, Box, Layout
from reagent_amd import ops

PRECS = [pytest.param(L.PREC_F32, id="f32"), pytest.param(L.PREC_BF16, id="bf16")]
VEC, BK = {L.PREC_F32: 4, L.PREC_BF16: 8}, {L.PREC_F32: 16, L.PREC_BF16: 64}
ALL3 = ("t", "f32", "tt")  # the typed row-major output, the fp32 one, the typed transposed one
COMBOS = [c for n in (3, 1, 2) for c in itertools.combinations(ALL3, n)]  # every non-empty choice, all three first
ALIGNED = Layout()  # vector loads, pair and 8-byte stores
FALLBACKS = Layout(a_off=1, b_off=1, a_vec=False, b_vec=False, ldy_even=False, ldyt4=False, y32_off=1)  # every scalar path
BACKENDS = ("emu", "hip")
Fn = torch.nn.functional


@pytest.fixture(autouse=True)
def _one_torch_thread():
    """The statements are thousands of small torch operations.  Intra-op threads gain them nothing, and when the suite's
    worker processes share the cores their spin-waits cost a file like this a factor of 30 (and the other workers their
    cores).  One thread while a test of this file runs; the setting found is put back."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def cases(rows):
    """rows of (backend name, values...) -> parameters of a test that takes the `backend` fixture indirectly and the values"""
    name = {L.PREC_F32: "f32", L.PREC_BF16: "bf16"}
    return [pytest.param(b, prec, *v, id="-".join([b, name[prec]] + [str(x) for x in v]), marks=[pytest.mark.gpu] if b == "hip" else [])
            for b, prec, *v in rows]


def _ceil(a, b):
    return -(-a // b)


def _cd(prec):
    return ops.compute_dtype(prec)


def _gen(*key):
    return torch.Generator().manual_seed(sum(int(k) * m for k, m in zip(key, (1_000_003, 40_009, 4_099, 257, 17, 1))) + 5)


def _settle(inputs, outputs):
    for b in inputs:
        assert b.outside_intact() and b.unchanged(), "an operand or its NaN surroundings were written"
    for b in outputs:
        assert b.outside_intact(), "the sentinel outside an output view was written"
        assert b.written(), "an output element is NaN or was not written"


# ---- the calls ----------------------------------------------------------------------------------------------------------
def run_gemm(dev, kind, prec, a, b, extra, act, outs=ALL3, lay=Layout()):
    """rg_fc_forward (extra = bias [N]) or rg_fc_dgrad (extra = ht [N, M] or None) of A [M, K] and B [N, K], as float
    tensors holding compute-type values -> {output name: cpu tensor}"""
    cd, V = _cd(prec), VEC[prec]
    (M, K), N = a.shape, b.shape[0]
    A = Box(dev, M, K, cd, R.pitch_for(K, V, lay.a_vec), lay.a_off, src=a)
    B = Box(dev, N, K, cd, R.pitch_for(K, V, lay.b_vec), lay.b_off, src=b)
    if extra is None:
        E = None
    elif kind == "forward":
        E = Box(dev, 1, N, F32, N + 3, 1, src=extra[None])
    else:
        E = Box(dev, N, M, cd, R.pitch_for(M, 2, False), 1, src=extra)
    ldy = R.pitch_for(N, 2, lay.ldy_even)  # the typed and the fp32 output share it
    o = dict(t=Box(dev, M, N, cd, ldy, 0, R.SENTINEL) if "t" in outs else None,
             f32=Box(dev, M, N, F32, ldy, lay.y32_off, R.SENTINEL) if "f32" in outs else None,
             tt=Box(dev, N, M, cd, R.pitch_for(M, 4, lay.ldyt4), 0, R.SENTINEL) if "tt" in outs else None)
    v = {k: None if x is None else x.v for k, x in o.items()}
    if kind == "forward":
        ops.fc_forward(A.v, B.v, None if E is None else E.v[0], L.ACT[act], prec, y=v["t"], y32=v["f32"], yt=v["tt"])
    else:
        ops.fc_dgrad(A.v, B.v, None if E is None else E.v, L.ACT[act], prec, dx=v["t"], dx32=v["f32"], dxt=v["tt"])
    _settle([x for x in (A, B, E) if x is not None], [x for x in o.values() if x is not None])
    return {k: x.cpu() for k, x in o.items() if x is not None}


def run_wgrad(dev, prec, dzt, xt, with_db=True, lay=Layout()):
    """rg_fc_wgrad of dz^T [out, batch] and x^T [in, batch] -> dw, db (or None), the split count seen through the
    workspace query"""
    cd, V = _cd(prec), VEC[prec]
    (out_f, batch), in_f = dzt.shape, xt.shape[0]
    A = Box(dev, out_f, batch, cd, R.pitch_for(batch, V, lay.a_vec), lay.a_off, src=dzt)
    B = Box(dev, in_f, batch, cd, R.pitch_for(batch, V, lay.b_vec), lay.b_off, src=xt)
    DW = Box(dev, out_f, in_f, F32, in_f, 0, R.SENTINEL)  # dw is contiguous by contract
    DB = Box(dev, 1, out_f, F32, out_f + 3, 1, R.SENTINEL) if with_db else None
    nbytes = ops.fc_wgrad_workspace_bytes(out_f, in_f, batch, prec)
    splits, rest = divmod(nbytes, 4 * (out_f * in_f + out_f))
    assert rest == 0 and splits >= 1
    wbuf, ws = R.workspace(dev, nbytes)
    ops.fc_wgrad(A.v, B.v, DW.v, None if DB is None else DB.v[0], ws, prec)
    assert R.same_bits(wbuf[ws.numel():], torch.full((16,), R.SENTINEL)), "the workspace beyond workspace_bytes was written"
    assert not bool(ws[:splits * out_f * in_f].isnan().any()) and not bool((ws[:splits * out_f * in_f] == R.SENTINEL).any()), \
        "a split's slab of dw partials was not written"
    _settle([A, B], [DW] + ([DB] if with_db else []))
    return DW.cpu(), (DB.cpu()[0] if with_db else None), splits


# ---- 1. exact statements: the edge table --------------------------------------------------------------------------------
def _star(prec):
    kb = 17 if prec == L.PREC_F32 else 65
    ks = (1, 3, 4, 5, 15, 16, 17, 31, 32, 33) if prec == L.PREC_F32 else (1, 7, 8, 9, 63, 64, 65, 127, 128, 129)
    s = [(M, 33, kb) for M in (1, 3, 4, 5, 31, 32, 33, 127, 128, 129, 257)]             # wide, M
    s += [(129, N, kb) for N in (33, 63, 64, 65, 127, 128, 129, 257)]                   # wide, N
    s += [(M, N, kb) for N in (1, 2, 31, 32) for M in (5, 255, 256, 257)]               # narrow
    s += [(129, 33, K) for K in ks]                                                     # K, the wide tile
    s += [(129, 31, K) for K in ks]                                                     # K, the narrow tile
    s += [(897, 33, 5), (1024, 33, 5), (1793, 3, 5), (2048, 3, 5)]                      # 8 row tiles: decode_wg's XCD branch
    s += [(897, 129, 5)]                                                                # ... with two column tiles inside it
    return list(dict.fromkeys(s))


CORNERS = [(1, 1, 1), (257, 257, 33), (129, 32, 17), (129, 33, 17)]  # the last two: narrow / wide on either side of N = 32
ALIGN_SHAPE = (129, 65, 33)
GEMM_SHAPES = {p: list(dict.fromkeys(_star(p) + CORNERS)) for p in (L.PREC_F32, L.PREC_BF16)}
GEMM_CASES = [pytest.param(p.values[0], *s, id=f"{p.id}-{s[0]}-{s[1]}-{s[2]}") for p in PRECS for s in GEMM_SHAPES[p.values[0]]]
WGRAD_BATCHES = {L.PREC_F32: (1, 15, 16, 17, 100, 128, 300), L.PREC_BF16: (1, 63, 64, 65, 448, 512, 1200)}
WGRAD_SPLIT_CLASSES = {L.PREC_F32: (100, 128, 300), L.PREC_BF16: (448, 512, 1200)}  # 7, 8, 10 padded to 16 at (40, 24)
WGRAD_SHAPES = [(40, 24), (2, 4), (32, 257), (33, 129), (129, 33)]
# the MI355X: every shape at every batch, with and without db, each at both layouts.  The interpreter, for its time: (40, 24)
# at every batch and the other shapes at BK + 1 and the padded split count; with db and ALIGNED, and at (40, 24) and (2, 4),
# the shapes of BIAS_MODE 1 and 2, without db and with FALLBACKS as well
WGRAD_CALLS = {"all": [(True, ALIGNED), (False, FALLBACKS), (True, FALLBACKS), (False, ALIGNED)],
               "db-nodb": [(True, ALIGNED), (False, FALLBACKS)], "db": [(True, ALIGNED)]}
WGRAD_ROWS = [(b, p, o, i, n, "all" if b == "hip" else "db-nodb" if k < 2 else "db")
              for b in BACKENDS for p in (L.PREC_F32, L.PREC_BF16) for k, (o, i) in enumerate(WGRAD_SHAPES)
              for n in (WGRAD_BATCHES[p] if b == "hip" or k == 0 else (WGRAD_BATCHES[p][3], WGRAD_BATCHES[p][6]))]


@functools.lru_cache(maxsize=None)
def int_case(kind, M, N, K, seed=0):
    """integer operands and the int64 statements -> (a, b, extra, {act: statement})"""
    assert K * 16 + 4 < 2 ** 24  # every partial sum of products of magnitude <= 16, and the bias, is an fp32 integer
    g = _gen(M, N, K, seed, kind == "forward")
    a, b = R.ints(g, M, K), R.ints(g, N, K)
    if kind == "forward":
        bias = R.ints(g, N)
        z = a @ b.t() + bias
        return a.float(), b.float(), bias.float(), {"linear": z, "relu": z.clamp(min=0)}
    ht = R.ints(g, N, M)  # the stored output of the layer below; relu's mask is h > 0
    z = a @ b.t()
    return a.float(), b.float(), ht.float(), {"linear": z, "relu": z * (ht.t() > 0)}


def check_int_gemm(dev, kind, prec, M, N, K, act, outs, lay, seed=0):
    a, b, extra, want = int_case(kind, M, N, K, seed)
    if kind == "dgrad" and act == "linear" and (M + N + K) % 2:
        extra = None  # no saved activation: the network input
    got = run_gemm(dev, kind, prec, a, b, extra, act, outs, lay)
    assert set(got) == set(outs)
    w32 = want[act].float()
    assert torch.equal(w32.long(), want[act])
    for k, t in got.items():
        ref = w32 if k == "f32" else R.rne(w32.t() if k == "tt" else w32, _cd(prec))
        assert t.dtype == ref.dtype and torch.equal(t, ref.contiguous()), (kind, k, (t.float() - ref.float()).abs().max())
    return got


def gemm_calls(backend_name, prec, shape):
    """(kind, outputs, activation, layout) of every call at one shape of the edge table.
    The MI355X: forward and dgrad with every non-empty choice of outputs, each at both layouts (ALIGNED: the vector loads
    and the wide stores; FALLBACKS: every scalar path), relu and linear alternating.
    The interpreter, for its time: the three small corners as the MI355X; any other shape the forward and the dgrad with all
    three outputs, ALIGNED, relu, and (up to 512 rows) the forward once more with one other choice of outputs, the next of
    the six for each shape down the table, linear, FALLBACKS and ALIGNED in turns of six shapes.
    test_paths_agree_bit_for_bit runs every choice and every layout on both at (129, 65, 33)."""
    if backend_name == "hip" or (shape in CORNERS and shape != (257, 257, 33)):
        return [(kind, outs, ("relu", "linear")[(j + k) % 2], lay) for kind in ("forward", "dgrad")
                for j, outs in enumerate(COMBOS) for k, lay in enumerate((ALIGNED, FALLBACKS))]
    calls = [("forward", ALL3, "relu", ALIGNED), ("dgrad", ALL3, "relu", ALIGNED)]
    if shape[0] <= 512:
        n = GEMM_SHAPES[prec].index(shape)
        calls.append(("forward", COMBOS[1 + n % 6], "linear", (FALLBACKS, ALIGNED)[n // 6 % 2]))  # (the layout changes every six)
    return calls


@pytest.mark.parametrize("prec,M,N,K", GEMM_CASES)
def test_gemm_is_exact_on_integers(backend, prec, M, N, K):
    """the edge table, forward and dgrad (gemm_calls says which calls)"""
    for kind, outs, act, lay in gemm_calls(backend.name, prec, (M, N, K)):
        check_int_gemm(backend.device, kind, prec, M, N, K, act, outs, lay)


@pytest.mark.parametrize("backend,prec,out_f,in_f,batch,dbs", cases(WGRAD_ROWS), indirect=["backend"])
def test_wgrad_is_exact_on_integers(backend, prec, out_f, in_f, batch, dbs):
    assert batch * 16 < 2 ** 24
    g = _gen(out_f, in_f, batch)
    dzt, xt = R.ints(g, out_f, batch), R.ints(g, in_f, batch)
    for with_db, lay in WGRAD_CALLS[dbs]:
        dw, db, _ = run_wgrad(backend.device, prec, dzt.float(), xt.float(), with_db, lay)
        assert torch.equal(dw, (dzt @ xt.t()).float())
        assert db is None or torch.equal(db, dzt.sum(1).float())


def test_wgrad_batches_cover_every_split_class(backend):
    """1 split, a count that is no multiple of 8, exactly 8, and a count padded to a multiple of 8 (whose empty tail
    splits wrote zeros above): seen through the workspace query, not restated"""
    for prec in (L.PREC_F32, L.PREC_BF16):
        seen = [ops.fc_wgrad_workspace_bytes(40, 24, b, prec) // (4 * (40 * 24 + 40)) for b in WGRAD_BATCHES[prec]]
        print(f"SPLITS prec {prec} batches {WGRAD_BATCHES[prec]} -> {seen}")
        assert 1 in seen and 8 in seen and any(1 < s < 8 for s in seen)
        # k_per_split is a multiple of BK and the splits cover the batch, so it is at least kmin; where the splits before the
        # last already cover the batch at kmin, the last ones are empty
        kmin = {b: _ceil(_ceil(b, n), BK[prec]) * BK[prec] for b, n in zip(WGRAD_BATCHES[prec], seen)}
        assert any(n > 8 and n % 8 == 0 and (n - 1) * kmin[b] >= b for b, n in zip(WGRAD_BATCHES[prec], seen)), "no empty tail split"
        assert [s for b, s in zip(WGRAD_BATCHES[prec], seen) if b in WGRAD_SPLIT_CLASSES[prec]][1] == 8


@pytest.mark.gpu
def test_dma_kernel_is_exact_on_integers():
    """the 256 x 256 LDS-DMA kernel at the floor of its shape test plus one row and one column of tail (bf16, MI355X only:
    the interpreter runs this kernel in test_fc_ops.py)"""
    assert torch.cuda.is_available()
    L.lib()
    for kind in ("forward", "dgrad"):
        check_int_gemm("cuda", kind, L.PREC_BF16, 2049, 193, 1024, "relu", ALL3, Layout())


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("N", [5, 33])
@pytest.mark.parametrize("step", [-1, 0, 1, "2+1"])
def test_one_hot_operands_hand_the_other_through(backend, prec, N, step):
    """x = I_K: y32 is w^T bit for bit, for a real w; the same for dgrad and wgrad.  A wrong element names the k index or
    the row / column that went astray"""
    K = 2 * BK[prec] + 1 if step == "2+1" else BK[prec] + step
    dev, eye = backend.device, torch.eye(K)
    w = R.rne(torch.randn(N, K, generator=_gen(N, K)), _cd(prec)).float()
    got = run_gemm(dev, "forward", prec, eye, w, torch.zeros(N), "linear", ALL3, Layout.of(K))
    assert R.same_bits(got["f32"], w.t().contiguous()) and R.same_bits(got["tt"].float(), w)
    got = run_gemm(dev, "dgrad", prec, eye, w, None, "linear", ALL3, Layout.of(K + 1))
    assert R.same_bits(got["f32"], w.t().contiguous()) and R.same_bits(got["t"].float(), w.t().contiguous())
    dw, db, _ = run_wgrad(dev, prec, eye, w, True, Layout.of(K))  # out = batch = K, in = N
    assert R.same_bits(dw, w.t().contiguous()) and torch.equal(db, torch.ones(K))
    dw, db, _ = run_wgrad(dev, prec, w, eye, True, Layout.of(K + 2))  # out = N, in = batch = K
    assert R.same_bits(dw, w) and (db.double() - w.double().sum(1)).abs().max() <= float(R.wgrad_bound(w.abs().sum(1), K).max())


def _align_layouts():
    base = Layout()
    alts = [Layout(a_off=1), Layout(b_off=1), Layout(a_vec=False), Layout(b_vec=False), Layout(a_off=1, b_off=1, a_vec=False, b_vec=False),
            Layout(ldy_even=False), Layout(ldyt4=False), Layout(y32_off=1), Layout(ldy_even=False, ldyt4=False, y32_off=1)]
    return base, alts


@pytest.mark.parametrize("prec", PRECS)
def test_paths_agree_bit_for_bit(backend, prec):
    """the alignment table at (129, 65, 33), integers first (every layout exact, every choice of outputs), then real
    operands: vector against scalar loads, pair against scalar stores, the 8-byte transposed store against its scalar
    fallback, the swapped epilogue (bf16, no transposed copy) with its 16- and 8-byte row stores against the unswapped one"""
    dev, (M, N, K) = backend.device, ALIGN_SHAPE
    base, alts = _align_layouts()
    for kind in ("forward", "dgrad"):
        for j, (lay, outs) in enumerate(itertools.product([base] + alts, COMBOS)):
            if backend.name == "emu" and kind == "forward" and lay is not base:
                continue  # (the interpreter holds the forward's other layouts to the base's bits below, on real operands)
            if lay is base or outs == ALL3 or (outs == ("t", "f32") and lay in alts[5:]):  # (the swapped epilogue: no transposed copy)
                check_int_gemm(dev, kind, prec, M, N, K, "relu" if j % 2 else "linear", outs, lay)
        g = _gen(M, N, K, prec)
        a, b = (R.rne(torch.randn(r, K, generator=g), _cd(prec)).float() for r in (M, N))
        extra = torch.randn(N, generator=g) if kind == "forward" else R.rne(torch.rand(N, M, generator=g), _cd(prec)).float()
        ref = {outs: run_gemm(dev, kind, prec, a, b, extra, "tanh", outs, base) for outs in COMBOS}
        for outs in COMBOS:  # with and without the transposed copy, an output alone or with the others
            for k in outs:
                assert R.same_bits(ref[outs][k], ref[ALL3][k]), (kind, outs, k)
        for lay in alts if kind == "forward" or backend.name == "hip" else alts[5:7]:  # (one load path for both entry points)
            for outs in (ALL3, ("t", "f32"))[:2 if lay in alts[5:] else 1]:
                got = run_gemm(dev, kind, prec, a, b, extra, "tanh", outs, lay)
                for k in outs:
                    assert R.same_bits(got[k], ref[ALL3][k]), (kind, lay, outs, k)
    g = _gen(40, 24, prec)
    batch = WGRAD_SPLIT_CLASSES[prec][2]
    dzt, xt = (R.rne(torch.randn(r, batch, generator=g), _cd(prec)).float() for r in (40, 24))
    dw0, db0, _ = run_wgrad(dev, prec, dzt, xt, True, base)
    for lay in (alts[0], alts[3], alts[4]):
        dw, db, _ = run_wgrad(dev, prec, dzt, xt, True, lay)
        assert R.same_bits(dw, dw0) and R.same_bits(db, db0), lay
    assert R.same_bits(run_wgrad(dev, prec, dzt, xt, False, base)[0], dw0)


@pytest.mark.parametrize("prec", PRECS)
def test_two_runs_give_the_same_bits_and_a_row_stands_alone(backend, prec):
    dev, (M, N, K) = backend.device, (129, 33, 17)
    g = _gen(M, N, K, prec, 9)
    a, b, bias = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g), torch.randn(N, generator=g)
    a, b = R.rne(a, _cd(prec)).float(), R.rne(b, _cd(prec)).float()
    ht = R.rne(torch.rand(N, M, generator=g), _cd(prec)).float()
    one, two = (run_gemm(dev, "forward", prec, a, b, bias, "sigmoid") for _ in range(2))
    d1, d2 = (run_gemm(dev, "dgrad", prec, a, b, ht, "sigmoid") for _ in range(2))
    assert all(R.same_bits(one[k], two[k]) and R.same_bits(d1[k], d2[k]) for k in ALL3)
    batch = WGRAD_SPLIT_CLASSES[prec][2]  # the padded split count
    dzt, xt = (R.rne(torch.randn(r, batch, generator=g), _cd(prec)).float() for r in (40, 24))
    w1, w2 = (run_wgrad(dev, prec, dzt, xt) for _ in range(2))
    assert R.same_bits(w1[0], w2[0]) and R.same_bits(w1[1], w2[1])
    for r in (0, 67, 128):  # changing row r of x changes row r of the outputs and nothing else
        a2 = a.clone()
        a2[r] = R.rne(torch.randn(K, generator=g), _cd(prec)).float()
        other = run_gemm(dev, "forward", prec, a2, b, bias, "sigmoid")
        keep = [i for i in range(M) if i != r]
        assert R.same_bits(other["f32"][keep], one["f32"][keep]) and R.same_bits(other["t"][keep], one["t"][keep])
        assert R.same_bits(other["tt"][:, keep], one["tt"][:, keep]) and not R.same_bits(other["f32"][r], one["f32"][r])
        alone = run_gemm(dev, "forward", prec, a2[r:r + 1], b, bias, "sigmoid")
        assert R.same_bits(alone["f32"], other["f32"][r:r + 1]) and R.same_bits(alone["tt"], other["tt"][:, r:r + 1])


# ---- 2. float64 statements, a bound per element -------------------------------------------------------------------------
CHAIN_SHAPES = {p: CORNERS + [(257, 129, 65)] + [(b, 24, 40) for b in WGRAD_SPLIT_CLASSES[p]] for p in (L.PREC_F32, L.PREC_BF16)}
# the MI355X and, up to 129 rows, the interpreter: all six activations.  The interpreter above 129 rows (up to a second a
# call): the one activation named here, each of the six at some shape
EMU_LARGE_CHAIN_ACT = {(L.PREC_F32, 257, 257, 33): "softplus", (L.PREC_F32, 257, 129, 65): "tanh", (L.PREC_F32, 300, 24, 40): "sigmoid",
                       (L.PREC_BF16, 257, 257, 33): "leaky_relu", (L.PREC_BF16, 257, 129, 65): "softplus",
                       (L.PREC_BF16, 448, 24, 40): "relu", (L.PREC_BF16, 512, 24, 40): "linear", (L.PREC_BF16, 1200, 24, 40): "sigmoid"}
CHAIN_ROWS = [(b, p, *s, act) for b in BACKENDS for p, shapes in CHAIN_SHAPES.items() for s in shapes for act in R.ACTS
              if b == "hip" or s[0] <= 129 or EMU_LARGE_CHAIN_ACT[(p, *s)] == act]
# the largest A_act that profiles/NOTES_r31.md records: a torch whose own fp32 activations err by more than twice that is no yardstick
A_ACT_RECORDED = {"tanh": 4.183, "sigmoid": 7.813, "softplus": 10.262}
AB_SHAPES = [(1, 1), (3, 257), (2100, 1001)]  # the last: more than 8192 blocks of 256, the grid-stride loop


@functools.lru_cache(maxsize=None)
def chain_case(prec, M, N, K):
    """one layer as the engine chains it: forward x [M, K] . w [N, K]^T + b, then the layer above's dgrad dz2 [M, K] .
    wt2 [N, K]^T masked by this layer's stored output, then its wgrad dz2^T . yt^T.  Operands as stored (bf16 mode: after
    the cast), rows and columns of the planted classes"""
    g, cd = _gen(M, N, K, prec, 3), _cd(prec)
    x, xrows = R.planted(g, M, K, R.ROW_CLASSES, K)
    w, wrows = R.planted(g, N, K, R.COL_CLASSES, 1)
    dz2, _ = R.planted(g, M, K, R.ROW_CLASSES, K + 2)
    wt2, _ = R.planted(g, N, K, R.COL_CLASSES, 2)
    dz2 = dz2 * torch.tensor([(1.0, 1e2, 1e-2, 0.0)[(k + 1) % 4] for k in range(K)])  # dw's rows get a scale of their own
    st = lambda t: R.rne(t, cd).float()  # noqa: E731
    p = dict(x=st(x), w=st(R.paired(w) * 0.3), bias=torch.randn(N, generator=g), dz2=st(dz2), wt2=st(R.paired(wt2) * 0.3),
             xrows=xrows, wrows=wrows)
    p["z64"], p["S1"] = R.gemm_statement(p["x"], p["w"], p["bias"])
    p["P2"], p["S2"] = R.gemm_statement(p["dz2"], p["wt2"])
    return p


def torch_layer(p, act):
    """torch's own fp32 layer and autograd backward on the stored operands -> z, h, dz (at the pre-activation), dw2, db2"""
    z = Fn.linear(p["x"], p["w"], p["bias"]).requires_grad_()
    h = R.act32(z, act)
    h.retain_grad()
    w2 = p["wt2"].t().contiguous().requires_grad_()  # [K, N]
    b2 = torch.zeros(w2.shape[0], requires_grad=True)
    Fn.linear(h, w2, b2).backward(p["dz2"])
    return z.detach(), h.detach(), z.grad, w2.grad, b2.grad


@functools.lru_cache(maxsize=None)
def activation_pool(act):
    """the fp32 pre-activations of every chained case, and the outputs rg_act_backward is tested on"""
    zs = [Fn.linear(p["x"], p["w"], p["bias"]).flatten() for prec, shapes in CHAIN_SHAPES.items()
          for p in (chain_case(prec, *s) for s in shapes)]
    return torch.cat(zs), torch.cat([act_backward_case(r, c, act)[1].flatten() for r, c in AB_SHAPES[:2]])


@functools.lru_cache(maxsize=None)
def measured_A_act():
    """4 x the largest error of torch's fp32 activation against float64, and of its fp32 backward through the output
    against act' of that output in float64, in units of u |statement| (R.through_output_scale for the backward)"""
    A = {}
    for act in R.SMOOTH:
        z, y = activation_pool(act)
        h = R.act32(z, act)
        ref = R.act64(z, act)
        over = lambda err: (err - R.TINY).clamp(min=0)  # noqa: E731  (below 2^-126 a result may be flushed: the bound's last term)
        worst = float((over((h.double() - ref).abs()) / (R.U * ref.abs().clamp(min=R.TINY))).max())
        for out in (h, y):
            one = torch.ones_like(out)
            g32, g64 = R.dact32_from_output(one, out, act).double(), R.dact64(out, act)
            scale = R.through_output_scale(g64, one.double(), out, act).clamp(min=R.TINY)
            worst = max(worst, float((over((g32 - g64).abs()) / (R.U * scale)).max()))
        zg = z.clone().requires_grad_()  # and the backward autograd itself takes (softplus: through the input)
        R.act32(zg, act).sum().backward()
        g64 = R.dact64(h, act)
        scale = R.through_output_scale(g64, torch.ones_like(g64), h, act).clamp(min=R.TINY)
        worst = max(worst, float((over((zg.grad.double() - g64).abs()) / (R.U * scale)).max()))
        A[act] = 4.0 * worst
        print(f"A_ACT {act} {A[act]:.3f}")
        assert A[act] <= 2 * A_ACT_RECORDED[act], (act, A[act])
    return A


def _hold(what, got, ref, bound, strata=None):
    """assert |got - ref| <= bound element by element -> the worst ratio (printed per stratum of rows)"""
    err = (got.double() - ref).abs()
    assert not bool(err.isnan().any()), what
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    for name, rows in (strata or {"all": None}).items():
        r = ratio if rows is None else ratio[rows]
        if r.numel():
            print(f"RATIO {what} {name} {float(r.max()):.3f}")
    bad = (err > bound).nonzero()
    assert bad.numel() == 0, (what, bad[0].tolist(), float(err[tuple(bad[0])]), float(bound[tuple(bad[0])]), float(ratio.max()))
    return float(ratio.max())


def hold_layer(what, p, act, K, M, y=None, y32=None, yt=None, h=None, dx=None, dx32=None, dxt=None, dw=None, db=None, bf16=False):
    """every output given against its float64 statement; h = the stored output the backward was run on"""
    A = measured_A_act()
    ref = R.act64(p["z64"], act)
    for name, t, tr, b16 in (("y32", y32, False, False), ("y", y, False, bf16), ("yt", yt, True, bf16)):
        if t is not None:
            _hold(f"{what} forward {name}", t.t() if tr else t, ref, R.forward_bound(ref, p["S1"], K, act, A, b16), p["xrows"])
    if h is None:
        return
    g = R.dact64(h, act)
    rd = p["P2"] * g
    for name, t, tr, b16 in (("dx32", dx32, False, False), ("dx", dx, False, bf16), ("dxt", dxt, True, bf16)):
        if t is not None:
            _hold(f"{what} dgrad {name}", t.t() if tr else t, rd, R.dgrad_bound(rd, p["P2"], p["S2"], h, g, K, act, A, b16), p["xrows"])
    if dw is not None:
        rw, Sw = R.gemm_statement(p["dz2"].t(), h.t())
        _hold(f"{what} wgrad dw", dw, rw, R.wgrad_bound(Sw, M))
        _hold(f"{what} wgrad db", db, p["dz2"].double().sum(0), R.wgrad_bound(p["dz2"].double().abs().sum(0), M))


def test_torch_fp32_meets_every_fc_bound():
    """no kernel runs: torch's fp32 linear, activation and autograd backward on the stored operands stay inside every
    bound the kernels are held to, at every shape and activation of this section, and so does its backward through the
    output at the cases of rg_act_backward"""
    A = measured_A_act()
    for prec, shapes in CHAIN_SHAPES.items():
        for (M, N, K), act in itertools.product(shapes, R.ACTS):
            p = chain_case(prec, M, N, K)
            _, h, dz, dw2, db2 = torch_layer(p, act)
            hold_layer(f"torch-fp32 {prec} {M} {N} {K} {act}", p, act, K, M, y32=h, h=h, dx32=dz, dw=dw2, db=db2)
    for (rows, cols), act in itertools.product(AB_SHAPES[:2], R.ACTS):
        dy, y = act_backward_case(rows, cols, act)
        ref = dy.double() * R.dact64(y, act)
        _hold(f"torch-fp32 act_backward {act}", R.dact32_from_output(dy, y, act), ref, R.act_backward_bound(ref, dy, y, act, A))


@pytest.mark.parametrize("backend,prec,M,N,K,act", cases(CHAIN_ROWS), indirect=["backend"])
def test_layer_chain_against_float64(backend, prec, M, N, K, act):
    """forward, dgrad and wgrad as a layer uses them: yt of the forward is the ht of the dgrad and the xt of the wgrad
    (CHAIN_ROWS says which shapes and activations run where)"""
    dev, p, bf16 = backend.device, chain_case(prec, M, N, K), prec == L.PREC_BF16
    lay = Layout.of(M + N + K + R.ACTS.index(act))
    f = run_gemm(dev, "forward", prec, p["x"], p["w"], p["bias"], act, ALL3, lay)
    h = f["tt"].float().t()  # as stored
    d = run_gemm(dev, "dgrad", prec, p["dz2"], p["wt2"], f["tt"].float(), act, ALL3, lay)
    dw, db, _ = run_wgrad(dev, prec, p["dz2"].t().contiguous(), f["tt"].float(), True, lay)
    hold_layer(f"{backend.name} {prec} {M} {N} {K} {act}", p, act, K, M, y=f["t"], y32=f["f32"], yt=f["tt"], h=h, dx=d["t"],
               dx32=d["f32"], dxt=d["tt"], dw=dw, db=db, bf16=bf16)
    assert R.same_bits(f["t"], f["tt"].t().contiguous())  # one value, stored twice
    assert R.same_bits(f["t"], R.rne(f["f32"], _cd(prec))) and R.same_bits(d["t"], R.rne(d["f32"], _cd(prec)))


# ---- 3. the two small entry points --------------------------------------------------------------------------------------
TC_SIZES = (1, 31, 32, 33, 65)


@pytest.mark.parametrize("src_dt,dst_dt", [(F32, F32), (F32, BF16), (BF16, BF16), (BF16, F32)], ids=["f32-f32", "f32-bf16", "bf16-bf16", "bf16-f32"])
def test_transpose_cast_is_torchs_cast_and_transpose(backend, src_dt, dst_dt):
    dev = backend.device
    for j, (rows, cols) in enumerate(itertools.product(TC_SIZES, TC_SIZES)):
        src = torch.randn(rows, cols, generator=_gen(rows, cols)) * 10.0 ** (j % 7 - 3)
        S = Box(dev, rows, cols, src_dt, cols + 1 + j % 3, j % 2, src=src)
        want = S.src.float().to(dst_dt)
        for which in (("dst",), ("dst_t",), ("dst", "dst_t")):
            D = Box(dev, rows, cols, dst_dt, cols + 2 + j % 2, (j + 1) % 2, R.SENTINEL) if "dst" in which else None
            T = Box(dev, cols, rows, dst_dt, rows + 1 + j % 4, j % 2, R.SENTINEL) if "dst_t" in which else None
            ops.transpose_cast(S.v, None if D is None else D.v, None if T is None else T.v)
            _settle([S], [b for b in (D, T) if b is not None])
            assert D is None or R.same_bits(D.cpu(), want)
            assert T is None or R.same_bits(T.cpu(), want.t().contiguous())


@functools.lru_cache(maxsize=None)
def act_backward_case(rows, cols, act):
    """dy and an output y of `act`, with 0, +-1 and tiny positives planted: relu's boundary, tanh's saturation, the tail
    of softplus (where 1 - exp(-y) is 0 in fp32 and the derivative is y)"""
    g = _gen(rows, cols, R.ACTS.index(act))
    dy = torch.randn(rows, cols, generator=g)
    y = R.act32(torch.randn(rows, cols, generator=g) * 3, act).flatten()
    plant = torch.tensor([0.0, 1.0, -1.0, 1e-3, 6e-8, 1e-12, 1e-30, float(2.0 ** -126)])
    idx = torch.arange(len(plant)) * max(1, y.numel() // len(plant) - 1) % y.numel()
    y[idx] = plant[:len(idx)]
    return dy, y.reshape(rows, cols)


def _act_backward(dev, rows, cols, act):
    dy, y = act_backward_case(rows, cols, act)
    DY, Y = Box(dev, rows, cols, F32, cols + 3, 1, src=dy), Box(dev, rows, cols, F32, cols + 1, 0, src=y)
    DZ = Box(dev, rows, cols, F32, cols + 2, 1, R.SENTINEL)
    ops.act_backward(DY.v, Y.v, L.ACT[act], DZ.v)
    _settle([DY, Y], [DZ])
    ref = dy.double() * R.dact64(y, act)
    _hold(f"act_backward {rows}x{cols} {act}", DZ.cpu(), ref, R.act_backward_bound(ref, dy, y, act, measured_A_act()))


@pytest.mark.parametrize("act", R.ACTS)
def test_act_backward_against_float64(backend, act):
    for rows, cols in AB_SHAPES[:2]:
        _act_backward(backend.device, rows, cols, act)


@pytest.mark.gpu
@pytest.mark.parametrize("act", R.ACTS)
def test_act_backward_beyond_the_grid_cap(act):
    """2100 x 1001 > 8192 blocks x 256 threads: the grid-stride loop (MI355X only: the interpreter needs 2 s a case)"""
    assert torch.cuda.is_available()
    L.lib()
    _act_backward("cuda", *AB_SHAPES[2], act)


# ---- 4. refusals and empty calls, by code -------------------------------------------------------------------------------
def test_refusals_and_empty_calls_by_code(backend):
    dev = backend.device
    lib, s = L.lib(), L.stream_ptr()
    buf = torch.full((4096,), R.SENTINEL, device=dev)
    sent = buf.clone()
    p = buf.data_ptr()

    def fwd(x=p, w=p, bias=p, y=p, y32=p, yt=p, batch=2, out_f=3, in_f=4, act=1, prec=L.PREC_F32):
        return lib.rg_fc_forward(x, in_f, w, in_f, bias, y, y32, out_f, yt, batch, batch, out_f, in_f, act, prec, s)

    def dgrad(dz=p, wt=p, ht=p, dx=p, dx32=p, dxt=p, batch=2, in_f=3, out_f=4, act=1, prec=L.PREC_F32):
        return lib.rg_fc_dgrad(dz, out_f, wt, out_f, ht, batch, act, dx, dx32, in_f, dxt, batch, batch, in_f, out_f, prec, s)

    def wgrad(dzt=p, xt=p, dw=p, db=p, ws=p + 2048, wsb=None, out_f=3, in_f=4, batch=2, prec=L.PREC_F32):
        wsb = lib.rg_fc_wgrad_workspace_bytes(out_f, in_f, batch, prec) if wsb is None else wsb
        return lib.rg_fc_wgrad(dzt, batch, xt, batch, dw, db, ws, wsb, out_f, in_f, batch, prec, s)

    def actb(dy=p, y=p, dz=p, rows=2, cols=3, act=3):
        return lib.rg_act_backward(dy, cols, y, cols, act, dz, cols, rows, cols, s)

    def tcast(src=p, dst=p, dst_t=p, rows=2, cols=3, sdt=L.DT_F32, ddt=L.DT_F32):
        return lib.rg_transpose_cast(src, sdt, cols, rows, cols, dst, cols, dst_t, rows, ddt, s)

    # what is refused returns before anything is written; what is empty returns RG_OK and writes nothing either
    for k in ("x", "w"):
        assert fwd(**{k: None}) == L.EINVAL, k
    for k in ("dz", "wt"):
        assert dgrad(**{k: None}) == L.EINVAL, k
    for k in ("dzt", "xt", "dw"):
        assert wgrad(**{k: None}) == L.EINVAL, k
    for k in ("dy", "y", "dz"):
        assert actb(**{k: None}) == L.EINVAL, k
    assert tcast(src=None) == L.EINVAL
    for call, dims in ((fwd, ("out_f", "in_f")), (dgrad, ("out_f", "in_f")), (wgrad, ("out_f", "in_f"))):
        assert call(batch=-1) == L.EINVAL
        for d in dims:
            assert call(**{d: 0}) == L.EINVAL and call(**{d: -1}) == L.EINVAL, d
        for bad in (L.PREC_BF16X3, 7, -1):  # (the split-bf16 mode is the fused stack's alone)
            assert call(prec=bad) == L.EUNSUPPORTED, bad
    assert wgrad(batch=0) == L.EINVAL  # a weight gradient over no rows is refused, not empty
    assert actb(rows=-1) == L.EINVAL and actb(cols=-1) == L.EINVAL and tcast(rows=-1) == L.EINVAL and tcast(cols=-1) == L.EINVAL
    assert tcast(sdt=5) == L.EUNSUPPORTED and tcast(ddt=5) == L.EUNSUPPORTED
    assert fwd(act=-1) == L.EINVAL and fwd(act=L.ACT["softplus"] + 1) == L.EINVAL
    # rg_fc_dgrad refuses an activation it has no derivative for when there is a saved output to mask by ...
    assert dgrad(act=-1) == L.EINVAL and dgrad(act=L.ACT["softplus"] + 1) == L.EINVAL
    assert fwd(batch=0) == 0 and dgrad(batch=0) == 0 and actb(rows=0) == 0 and actb(cols=0) == 0
    assert tcast(rows=0) == 0 and tcast(cols=0) == 0
    need = lib.rg_fc_wgrad_workspace_bytes(3, 4, 2, L.PREC_F32)
    assert need == 4 * (3 * 4 + 3) and lib.rg_fc_wgrad_workspace_bytes(3, 4, 0, L.PREC_F32) == need
    for o, i in ((0, 4), (3, 0), (-1, 4), (3, -1)):  # the query of a shape rg_fc_wgrad refuses: no bytes (it used to divide by zero tiles)
        assert lib.rg_fc_wgrad_workspace_bytes(o, i, 2, L.PREC_F32) == 0
    assert wgrad(ws=None) == L.EWORKSPACE and wgrad(wsb=need - 1) == L.EWORKSPACE and wgrad(wsb=0) == L.EWORKSPACE
    if dev != "cpu":
        torch.cuda.synchronize()
    assert R.same_bits(buf, sent), "a refused or empty call wrote"
    # ... and takes any code without one (no mask is applied), as before
    assert dgrad(ht=None, act=99) == 0 and fwd() == 0 and dgrad() == 0 and wgrad() == 0 and actb() == 0 and tcast() == 0
    x = torch.zeros(2, 4, device=dev)
    with pytest.raises(L.ReagentHipError, match=r"rg_fc_dgrad failed.*code -1"):
        ops.fc_dgrad(x, torch.zeros(3, 4, device=dev), torch.zeros(3, 2, device=dev), 6, L.PREC_F32, dx32=torch.zeros(2, 3, device=dev))
    with pytest.raises(L.ReagentHipError, match=r"rg_fc_wgrad failed.*code -4"):
        ops.fc_wgrad(x.t().contiguous(), x.t().contiguous(), torch.zeros(4, 4, device=dev), None, torch.zeros(1, device=dev), L.PREC_F32)
