"""rg_fc_wgrad_rows (reagent_amd/csrc/fc_rows.hip), the weight gradient from row-major operands, held to the statements of
tests/fc_refs.py on the interpreter and on the MI355X, and lstm_stack.wgrad_rows' routing to it.

Exact: integer operands of magnitude <= 4 (rows * 16 < 2^24: every partial sum is an fp32 integer in any order) must give
the int64 product.  Float64: |got - ref| <= (2 rows + 4) u S + 2^-126 per element (fc_refs.wgrad_bound).  Nothing else is a
tolerance.  The row counts come from the workspace query: SLAB = the most rows it asks no workspace for (one split, dw and
db written by the one launch), CAP(out, in) = the split count it settles at, so SLAB * CAP + 5 rows are more than a slab a
split with a ragged last one.  Every operand is a view into a NaN-filled parent, every output one into a sentinel-filled
parent (fc_refs.Box)."""
import functools

import pytest
import torch

import fc_refs as R
import reagent_amd._lib as L
from fc_refs import F32, Box
from reagent_amd import ops
from reagent_amd.models import encoder_ops, lstm_stack

SHAPES = [(1, 1), (3, 5), (32, 32), (33, 129), (128, 128), (130, 257), (512, 512)]


@functools.lru_cache(maxsize=None)
def splits(out_f, in_f, rows):
    n, rest = divmod(ops.fc_wgrad_rows_workspace_bytes(out_f, in_f, rows), 4 * (out_f * in_f + out_f))
    assert rest == 0
    return max(n, 1)


@functools.lru_cache(maxsize=None)
def slab():
    return next(n for n in range(1, 4096) if splits(1, 1, n + 1) > 1)


def row_count(kind, out_f, in_f):
    return {"slab": slab(), "slab+1": slab() + 1, "long": slab() * splits(out_f, in_f, 1 << 24) + 5}.get(kind, kind)


def rows_cases():
    """(backend, out, in, rows kind, db, unaligned): every shape at two ragged splits; every row edge and the one-split
    launch at the two-tile (33, 129); one split over 16 tiles; several slabs a split at one tile and at many.  The MI355X
    runs the long count at the widest shapes too (the interpreter needs seconds for them)"""
    rows = [(o, i, "slab+1", k % 3 != 0, k % 2 == 1) for k, (o, i) in enumerate(SHAPES)]
    rows += [(33, 129, n, k % 2 == 0, k % 3 == 0) for k, n in enumerate((1, 2, 31, 33, "slab"))]
    rows += [(512, 512, "slab", True, True), (3, 5, "long", True, True), (130, 257, "long", False, False)]
    hip = rows + [(128, 128, "long", True, False), (512, 512, "long", True, True)]
    return [pytest.param(b, *c, id="-".join(str(v) for v in (b,) + c), marks=[pytest.mark.gpu] if b == "hip" else [])
            for b, cs in (("emu", rows), ("hip", hip)) for c in cs]


def run(dev, dz, x, with_db=True, unaligned=False):
    """rg_fc_wgrad_rows of dz [rows, out] and x [rows, in] -> dw, db (or None)"""
    (rows, out_f), in_f = dz.shape, x.shape[1]
    A = Box(dev, rows, out_f, F32, R.pitch_for(out_f, 4, not unaligned), int(unaligned), src=dz)
    B = Box(dev, rows, in_f, F32, R.pitch_for(in_f, 4, not unaligned), int(unaligned), src=x)
    DW = Box(dev, out_f, in_f, F32, in_f, 0, R.SENTINEL)  # dw is contiguous by contract
    DB = Box(dev, 1, out_f, F32, out_f + 3, 1, R.SENTINEL) if with_db else None
    nbytes = ops.fc_wgrad_rows_workspace_bytes(out_f, in_f, rows)
    wbuf, ws = R.workspace(dev, nbytes)
    ops.fc_wgrad_rows(A.v, B.v, DW.v, None if DB is None else DB.v[0], ws if nbytes else None)
    assert R.same_bits(wbuf[ws.numel():], torch.full((16,), R.SENTINEL)), "the workspace beyond its queried bytes was written"
    for b in (A, B):
        assert b.outside_intact() and b.unchanged(), "an operand or its NaN surroundings were written"
    for b in [DW] + ([DB] if with_db else []):
        assert b.outside_intact() and b.written(), "an output element is unwritten or NaN, or its surroundings were written"
    return DW.cpu(), (DB.cpu()[0] if with_db else None)


@pytest.mark.parametrize("backend,out_f,in_f,kind,with_db,unaligned", rows_cases(), indirect=["backend"])
def test_wgrad_rows_is_exact_on_integers(backend, out_f, in_f, kind, with_db, unaligned):
    rows = row_count(kind, out_f, in_f)
    assert rows * 16 < 2 ** 24 and (splits(out_f, in_f, rows) == 1) == (rows <= slab())
    assert kind != "long" or (splits(out_f, in_f, rows) >= 2 and rows > slab() * splits(out_f, in_f, rows) and rows % slab())
    g = torch.Generator().manual_seed(out_f * 4099 + in_f * 17 + rows)
    dz, x = R.ints(g, rows, out_f), R.ints(g, rows, in_f)
    dw, db = run(backend.device, dz.float(), x.float(), with_db, unaligned)
    assert torch.equal(dw, (dz.t() @ x).float())
    assert db is None or torch.equal(db, dz.sum(0).float())


@pytest.mark.parametrize("out_f,in_f,kind", [(3, 5, "long"), (33, 129, 31), (128, 128, "slab"), (130, 257, "slab+1"), (512, 512, "slab+1")])
def test_wgrad_rows_against_float64(backend, out_f, in_f, kind):
    """planted row classes, pitches above the widths, bases off a 16-byte boundary, NaN in every padding; and two runs
    give the same bits"""
    rows = row_count(kind, out_f, in_f)
    g = torch.Generator().manual_seed(out_f * 4099 + in_f * 17 + rows + 1)
    dz, _ = R.planted(g, rows, out_f, R.ROW_CLASSES, out_f)
    x, _ = R.planted(g, rows, in_f, R.ROW_CLASSES, in_f + 2)
    dw, db = run(backend.device, dz, x, True, True)
    again = run(backend.device, dz, x, True, True)
    assert R.same_bits(dw, again[0]) and R.same_bits(db, again[1])
    ref, S = R.gemm_statement(dz.t(), x.t())
    for what, got, want, mag in (("dw", dw, ref, S), ("db", db, dz.double().sum(0), dz.double().abs().sum(0))):
        err, bound = (got.double() - want).abs(), R.wgrad_bound(mag, rows)
        print(f"RATIO {what} {out_f} {in_f} {rows} {float((err / bound).max()):.3f}")
        assert bool(got.isfinite().all()) and bool((err <= bound).all()), what


def test_wgrad_rows_refusals_by_code(backend):
    dev, lib, s = backend.device, L.lib(), L.stream_ptr()
    buf = torch.full((4096,), R.SENTINEL, device=dev)
    sent, p, rows = buf.clone(), buf.data_ptr(), slab() + 1
    need = lib.rg_fc_wgrad_rows_workspace_bytes(3, 4, rows)
    assert need == 2 * 4 * (3 * 4 + 3) and lib.rg_fc_wgrad_rows_workspace_bytes(3, 4, slab()) == 0

    def call(dz=p, x=p, dw=p, db=p, ws=p, wsb=need, out_f=3, in_f=4, rows=rows, ld_dz=None, ldx=None):
        return lib.rg_fc_wgrad_rows(dz, out_f if ld_dz is None else ld_dz, x, in_f if ldx is None else ldx, dw, db, ws, wsb,
                                    out_f, in_f, rows, s)

    for k in ("dz", "x", "dw"):
        assert call(**{k: None}) == L.EINVAL, k
    for k in ("out_f", "in_f", "rows"):
        assert call(**{k: 0}) == L.EINVAL and call(**{k: -1}) == L.EINVAL, k
    assert call(out_f=513) == L.EINVAL and call(in_f=513) == L.EINVAL and call(ld_dz=2) == L.EINVAL and call(ldx=3) == L.EINVAL
    assert call(ws=None) == L.EWORKSPACE and call(wsb=need - 1) == L.EWORKSPACE and call(wsb=0) == L.EWORKSPACE
    for o, i, n in ((0, 4, rows), (3, 0, rows), (3, 4, 0), (-1, 4, rows), (3, -1, rows), (3, 4, -1), (513, 4, rows), (3, 513, rows)):
        assert lib.rg_fc_wgrad_rows_workspace_bytes(o, i, n) == 0, (o, i, n)
    if dev != "cpu":
        torch.cuda.synchronize()
    assert R.same_bits(buf, sent), "a refused call wrote"


def test_routing_at_the_threshold(backend):
    """at WGRAD_ROWS_MIN rows lstm_stack.wgrad_rows is one rg_fc_wgrad_rows, one row below it the transposed path, bit for
    bit; encoder_ops.linear_backward on a row slice of a packed parameter writes that slice alone"""
    dev, n, E = backend.device, lstm_stack.WGRAD_ROWS_MIN, 8
    g = torch.Generator().manual_seed(33)
    dz, x = torch.randn(n, E, generator=g).to(dev), torch.randn(n, E, generator=g).to(dev)
    new = lambda: (torch.full((E, E), R.SENTINEL, device=dev), torch.full((E,), R.SENTINEL, device=dev))  # noqa: E731
    for rows in (n, n - 1):
        (dw, db), (dw2, db2) = new(), new()
        lstm_stack.wgrad_rows(dz[:rows], x[:rows], dw, db)
        if rows == n:
            nbytes = ops.fc_wgrad_rows_workspace_bytes(E, E, rows)
            ops.fc_wgrad_rows(dz, x, dw2, db2, torch.empty(nbytes // 4, device=dev))
        else:
            lstm_stack.wgrad(lstm_stack.transposed(dz[:rows]), lstm_stack.transposed(x[:rows]), dw2, db2, rows)
        assert R.same_bits(dw, dw2) and R.same_bits(db, db2), rows
    w = torch.zeros(3 * E, E, device=dev)
    dw, db = torch.full((3 * E, E), R.SENTINEL, device=dev), torch.full((3 * E,), R.SENTINEL, device=dev)
    assert encoder_ops.linear_backward(encoder_ops.TransposedCache(), dz, x, "in_proj", w, dw, db, rows=slice(E, 2 * E), need_dx=False) is None
    ref, S = R.gemm_statement(dz.cpu().t(), x.cpu().t())
    assert bool(((dw[E:2 * E].cpu().double() - ref).abs() <= R.wgrad_bound(S, n)).all())
    assert bool(((db[E:2 * E].cpu().double() - dz.cpu().double().sum(0)).abs() <= R.wgrad_bound(dz.cpu().double().abs().sum(0), n)).all())
    keep = [r for r in range(3 * E) if not E <= r < 2 * E]
    assert bool((dw[keep] == R.SENTINEL).all()) and bool((db[keep] == R.SENTINEL).all())
