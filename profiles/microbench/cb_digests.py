"""SHA-256 of every output buffer of the contextual-bandit kernels on seeded inputs: a change that must keep their bits
(a refactor of cb.hip, cb_disjoint.hip, cb_deep.hip, cb_eval.hip or of the headers they share) is run before and after,
and every line must agree.
python profiles/microbench/cb_digests.py          the device (RG_LIB selects another build of the library)
python profiles/microbench/cb_digests.py --emu    the SIMT interpreter of tests/emu, on the host

  rg_linucb_accumulate   plain rows and [B, A, d] + action rows (one index below 0, one past A), weighted, two batches in a row
  rg_dlinucb_accumulate  three arms, the middle one empty, weighted, two batches in a row
  rg_linucb_score        three arms with arm_presence (one row with no arm present)
  rg_dlinucb_score       the same rows against three matrices, with arm_presence
  rg_drlinucb_head       train mode: sigmoid output, cross-entropy, weights, dv
  rg_cb_eval_ingest      clipped importance weights, arm_presence, two batches in a row
at (B, d) = (257, 33) and (1000, 130): more than one slice in both plans at the second, ragged tiles at both."""
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
EMU = "--emu" in sys.argv
if EMU:
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import emu_backend

    emu_backend.install()
from reagent_amd import ops  # noqa: E402

dev = torch.device("cpu" if EMU else "cuda")
ARMS = 3


def show(what, *tensors):
    for i, t in enumerate(tensors):
        h = hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()
        print(f"{what}[{i}] {tuple(t.shape)} {h}", flush=True)


def run(B, d):
    tag = f"B={B} d={d}"
    g = torch.Generator().manual_seed(1000 * B + d)
    rand = lambda *s: torch.randn(*s, generator=g).to(dev)  # noqa: E731
    weights = lambda n: (0.5 + torch.rand(n, generator=g)).to(dev)  # noqa: E731

    # --- joint accumulate: plain rows, then action rows, two batches each on one state
    for kind in ("plain", "action"):
        state = [torch.zeros(d, d, device=dev), torch.zeros(d, device=dev), torch.full((1,), 1e-5, device=dev),
                 torch.zeros(1, dtype=torch.int64, device=dev)]
        ws = ops.linucb_workspace(B, d, dev)
        for _ in range(2):
            y, w = rand(B), weights(B)
            if kind == "plain":
                ops.linucb_accumulate(rand(B, d), y, w, *state, ws)
            else:
                action = torch.randint(ARMS, (B,), generator=g)
                action[0], action[B - 1] = -2, ARMS + 1
                ops.linucb_accumulate(rand(B, ARMS, d), y, w, *state, ws, action=action.to(dev))
        show(f"{tag} linucb_accumulate {kind}", *state)

    # --- disjoint accumulate: arms of B - B // 3, 0 and B // 3 rows
    offsets = torch.tensor([0, B - B // 3, B - B // 3, B], dtype=torch.int64).to(dev)
    dstate = [torch.zeros(ARMS, d, d, device=dev), torch.zeros(ARMS, d, device=dev),
              torch.zeros(ARMS, dtype=torch.int64, device=dev)]
    dws = ops.dlinucb_workspace(B - B // 3, ARMS, d, dev)
    for _ in range(2):
        ops.dlinucb_accumulate(rand(B, d), rand(B), weights(B), offsets, B - B // 3, *dstate, dws)
    show(f"{tag} dlinucb_accumulate", *dstate)

    # --- the two scorers on the same rows
    x = rand(B, ARMS, d)
    G = rand(ARMS, d, d)
    M = (G @ G.transpose(1, 2) / d + torch.eye(d, device=dev)).contiguous()
    coefs = rand(ARMS, d)
    presence = (torch.rand(B, ARMS, generator=g) < 0.7)
    presence[1] = False
    presence = presence.to(dev)
    N = B * ARMS
    out = torch.zeros(3, N, device=dev)
    nan = torch.zeros(ops.linucb_score_partials(N) + 1, dtype=torch.int32, device=dev)
    best = torch.zeros(B, dtype=torch.int64, device=dev)
    ops.linucb_score(x.view(N, d), coefs[0], M[0], torch.full((1,), 37.5, device=dev), 1.5, out[0], out[1], out[2],
                     nan[1:], nan[:1], arms=ARMS, arm_presence=presence.view(-1), best_arm=best)
    show(f"{tag} linucb_score", out, nan, best)
    dout = torch.zeros(3, B, ARMS, device=dev)
    dbest = torch.zeros(B, dtype=torch.int64, device=dev)
    ops.dlinucb_score(x[:, 0].contiguous(), coefs, M, 1.5, dout[2], mean=dout[0], sigma=dout[1], arm_presence=presence,
                      best_arm=dbest)
    show(f"{tag} dlinucb_score", dout, dbest)

    # --- the deep-represent head, train mode
    h = d
    mlp, v = rand(B, h), rand(h + 1) / h ** 0.5
    label, w = torch.rand(B, generator=g).to(dev), weights(B)
    P = ops.drlinucb_head_partials(B, h)
    z, lin, pred, row_loss = (torch.zeros(B, h + 1, device=dev), torch.zeros(B, device=dev), torch.zeros(B, device=dev),
                              torch.zeros(B, device=dev))
    dmlp, lp, dvp = torch.zeros(B, h, device=dev), torch.zeros(P, device=dev), torch.zeros(P * (h + 1), device=dev)
    loss, dv = torch.zeros(1, device=dev), torch.zeros(h + 1, device=dev)
    ops.drlinucb_head(mlp, v, 4, z, lin, pred, label=label, weight=w, loss_type=2, row_loss=row_loss, dmlp_out=dmlp,
                      loss_partials=lp, dv_partials=dvp, loss=loss, dv=dv)
    show(f"{tag} drlinucb_head", z, lin, pred, row_loss, dmlp, lp, dvp, loss, dv)

    # --- offline evaluation
    sums = [torch.zeros(1, device=dev) for _ in range(8)]
    since = torch.zeros(1, device=dev)
    iw, eff = torch.zeros(B, device=dev), torch.zeros(B, device=dev)
    partials = ops.cb_eval_partials(B, dev)
    for _ in range(2):
        action = torch.randint(ARMS, (B,), generator=g).to(dev)
        model_action = torch.randint(ARMS, (B,), generator=g).to(dev)
        logp = torch.log(0.05 + 0.9 * torch.rand(B, generator=g)).to(dev)
        ops.cb_eval_ingest(action, model_action, rand(B), weights(B), logp, presence, ARMS, 8.0, iw, eff, partials, sums, since)
    show(f"{tag} cb_eval_ingest", iw, eff, partials, torch.cat(sums), since)


for shape in ((257, 33), (1000, 130)):
    run(*shape)
