"""Helper of tests/test_gpu_ce_rows_golden.py and tools/make_ce_rows_golden.py (not a test): the case list of the row
cross-entropy fixture tests/golden/ce_rows.npz and the code that runs one case on the device.

A case is (id, form, params). Inputs come from tests/golden/gen.py's seeded streams, so the fixture holds outputs
only. ``run`` returns {name: uint32 / int32 array}: every float output as its 32-bit patterns. loss_rows, lse,
logp_rows and the gradients at V = 7 and 257 are kept whole; at V = 8100 a gradient row is kept as two integers,
the wrapping sum and the xor of its patterns.

B = T = 3 throughout. V = 7: most of the 256 threads hold no element (the -inf rescale); 257: thread 0 holds two;
8100: the size of the fp64 tests. Per form:
  bt      capmi_ce_fwd_bwd: bt NULL / [3, 2, 0], gscale NULL / set, lse NULL / set: every pair of their values in
          one of the four gradient cases, dl_time_major 0 and 1 twice each; two cases without dlogits
  ignore  capmi_count_targets + capmi_ce_ignore_fwd_bwd: tgt_off 0 / 2, row (0, 1) ignored, row (2, 0)'s target = V
  pg      capmi_pg_ce_fwd_bwd: capmi/scst.py's two call sites (tgt_off, t_first, L) = (0, 1, T) and (1, 0, T + 1),
          lens = [0, full, 1], adv[1] < 0
  inf     one case per form at V = 7 with a -inf logit in the live row (1, 1), whose thread then holds nothing else;
          one at V = 257 (ignore form, no gradient) where thread 0 meets -inf first and a finite logit second
  fin     capmi_loss_finalize (with and without reg_part) and capmi_loss_finalize_dev at n = 1, 9, 1025"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "ce_rows.npz")
SEED = 97
B, T = 3, 3
VS = (7, 257, 8100)
WHOLE_V = 257  # gradients of wider rows are stored as (sum, xor)
BT = (3, 2, 0)
GSCALE = 0.37
ADV = (0.75, -1.25, 0.5)
PG_SITES = ((0, 1, T), (1, 0, T + 1))  # (tgt_off, t_first, L)
FIN_N = (1, 9, 1025)


def cases():
    out = []
    for V in VS:
        for bt, gs, lse, dl, tm in ((0, 0, 0, 1, 0), (0, 1, 1, 1, 1), (1, 0, 1, 1, 1), (1, 1, 0, 1, 0),
                                    (1, 0, 0, 0, 0), (0, 1, 1, 0, 1)):
            out.append((f"bt.V{V}.bt{bt}.gs{gs}.lse{lse}.dl{dl}.tm{tm}", "bt",
                        dict(V=V, bt=bt, gs=gs, lse=lse, dl=dl, tm=tm, inf=None)))
        for off, dl, tm in ((0, 1, 0), (2, 1, 1), (0, 0, 1), (2, 0, 0)):
            out.append((f"ignore.V{V}.off{off}.dl{dl}.tm{tm}", "ignore", dict(V=V, off=off, dl=dl, tm=tm, inf=None)))
        for site, dl, tm in ((0, 1, 1), (1, 1, 0), (0, 0, 0), (1, 0, 1)):
            out.append((f"pg.V{V}.site{site}.dl{dl}.tm{tm}", "pg", dict(V=V, site=site, dl=dl, tm=tm, inf=None)))
    out.append(("inf.bt.V7", "bt", dict(V=7, bt=1, gs=1, lse=1, dl=1, tm=0, inf=2)))
    out.append(("inf.ignore.V7", "ignore", dict(V=7, off=0, dl=1, tm=0, inf=2)))
    out.append(("inf.pg.V7", "pg", dict(V=7, site=1, dl=1, tm=0, inf=2)))
    out.append(("inf.ignore.V257", "ignore", dict(V=257, off=0, dl=0, tm=0, inf=0)))
    for n in FIN_N:
        out.append((f"fin.n{n}", "fin", dict(n=n)))
    return out


def _gen():
    g = os.path.join(HERE, "golden")
    if g not in sys.path:
        sys.path.insert(0, g)
    import gen
    return gen


def logits(V, inf):
    x = _gen().uniform(SEED, f"logits{V}", (B, T, V), -4.0, 4.0)
    if inf is not None:
        x[1, 1, inf] = -np.inf
    return x


def caps(V, L, name):
    """(B, L) int64 targets in [1, V)."""
    c = _gen().uniform(SEED, f"caps.{name}.{V}.{L}", (B, L), 1.0, float(V))
    return np.minimum(c.astype(np.int64), V - 1)


def _bits(t):
    import torch
    return t.detach().cpu().contiguous().view(torch.int32).numpy().view(np.uint32)


def _grad(dl, V):
    u = _bits(dl).reshape(B * T, V)
    if V <= WHOLE_V:
        return u
    return np.stack([u.sum(axis=1, dtype=np.uint32), np.bitwise_xor.reduce(u, axis=1)], axis=1)


def run(case, K, dev="cuda"):
    """The case's launches on ``dev`` through capmi.kernels ``K``; every output starts as NaN."""
    import torch
    _, form, p = case

    def f32(a):
        return torch.tensor(np.asarray(a, dtype=np.float32), device=dev)

    def nan(*shape):
        return torch.full(shape, float("nan"), device=dev)

    out = {}
    if form == "fin":
        n = p["n"]
        rows = f32(_gen().uniform(SEED, f"fin.rows{n}", (n,), -1.0, 3.0))
        reg = f32(_gen().uniform(SEED, f"fin.reg{n}", (n,), 0.0, 0.01))
        for name, r in (("loss", None), ("loss_reg", reg)):
            o = nan(1)
            K.loss_finalize(rows, n, n, r, o)
            out[name] = _bits(o)
        o = nan(1)
        K.loss_finalize_dev(rows, n, f32([1.0 / n]), o)
        out["loss_dev"] = _bits(o)
        return out

    V = p["V"]
    x = torch.from_numpy(logits(V, p["inf"])).to(dev)
    dl = nan(B * T, V) if p["dl"] else None
    loss = nan(B * T)
    if form == "bt":
        L = T + 1
        c = torch.from_numpy(caps(V, L, "bt")).to(dev)
        bt = torch.tensor(BT, dtype=torch.int32, device=dev) if p["bt"] else None
        lse = nan(B * T) if p["lse"] else None
        K.ce_fwd_bwd(x, c, B, T, L, V, bt, sum(BT) if p["bt"] else B * T, loss, lse, dl, bool(p["tm"]),
                     f32([GSCALE]) if p["gs"] else None)
        if lse is not None:
            out["lse"] = _bits(lse)
    elif form == "ignore":
        off = p["off"]
        L = T + off
        cn = caps(V, L, "ignore")
        cn[0, 1 + off] = 0  # ignore_index
        cn[2, 0 + off] = V  # outside [0, V): never followed
        c = torch.from_numpy(cn).to(dev)
        count, inv = torch.full((1,), -1, dtype=torch.int32, device=dev), nan(1)
        K.count_targets(c, B, T, L, off, 0, count, inv)
        K.ce_ignore_fwd_bwd(x, c, B, T, L, V, off, 0, inv, loss, dl, bool(p["tm"]))
        out["count"] = count.cpu().numpy()
        out["inv_count"] = _bits(inv)
    else:
        off, t_first, L = PG_SITES[p["site"]]
        c = torch.from_numpy(caps(V, L, "pg")).to(dev)
        lens_h = [0, T - t_first, 1]
        lens = torch.tensor(lens_h, dtype=torch.int32, device=dev)
        logp = nan(B * T)
        K.pg_ce_fwd_bwd(x, c, B, T, L, V, off, lens, t_first, f32(ADV), f32([1.0 / sum(lens_h)]), logp, loss, dl,
                        bool(p["tm"]))
        out["logp"] = _bits(logp)
    out["loss"] = _bits(loss)
    if dl is not None:
        out["dlogits"] = _grad(dl, V)
    torch.cuda.synchronize()
    return out
