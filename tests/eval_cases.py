"""Shared pieces of the validation-pass tests (test_eval_cpu.py, test_gpu_eval.py): an fp64 numpy
restatement of the contracts of capmi_eval_rows / capmi_eval_captions (include/capmi.h), constructed
logits whose ties are exact float equalities, and the fp64 oracle of one caption evaluated alone."""
import numpy as np
import torch

GAP = 1e-5  # a decode row whose oracle top-2 logit gap is below this may be left out of token comparisons


def clamp_lens(lens, B, T):
    return [T] * B if lens is None else [min(max(int(n), 0), T) for n in lens]


def rows_ref(logits, caps, lens):
    """logits (B, T, V), caps (B, L) int, lens: B ints or None -> loss (B, T) fp64, pred, rank (B, T) int."""
    x = np.asarray(logits, np.float64)
    B, T, V = x.shape
    loss = np.zeros((B, T), np.float64)
    pred = np.full((B, T), -1, np.int64)
    rank = np.full((B, T), -1, np.int64)
    for b, n in enumerate(clamp_lens(lens, B, T)):
        for t in range(n):
            r = x[b, t]
            tgt = int(caps[b][t + 1])
            pred[b, t] = int(np.argmax(r))  # numpy: the first index attaining the maximum
            if tgt < 0 or tgt >= V:
                loss[b, t], rank[b, t] = np.inf, V
                continue
            m = r.max()
            loss[b, t] = m + np.log(np.exp(r - m).sum()) - r[tgt]
            rank[b, t] = int((r > r[tgt]).sum() + (r[:tgt] == r[tgt]).sum())
    return loss, pred, rank


def captions_ref(loss_rows, rank, alphas, lens, alpha_c=1.0):
    """loss_rows, rank (B, T); alphas (B, T, P) -> dict of (B,) arrays: ce, reg, loss (fp64), top1, top5."""
    lr = np.asarray(loss_rows, np.float64)
    a = np.asarray(alphas, np.float64)
    rk = np.asarray(rank)
    B, T = lr.shape
    out = {k: np.zeros(B, np.float64) for k in ("ce", "reg", "loss")}
    out["top1"], out["top5"] = np.zeros(B, np.int64), np.zeros(B, np.int64)
    for b, n in enumerate(clamp_lens(lens, B, T)):
        if n == 0:
            continue
        out["ce"][b] = lr[b, :n].sum() / n
        out["reg"][b] = ((alpha_c - a[b, :n].sum(axis=0)) ** 2).sum() / a.shape[2]
        out["loss"][b] = out["ce"][b] + out["reg"][b]
        out["top1"][b] = int((rk[b, :n] == 0).sum())
        out["top5"][b] = int(((rk[b, :n] >= 0) & (rk[b, :n] < 5)).sum())
    return out


# ---------------------------------------------------------------------------------------------------
# constructed logits: every value is a multiple of 1/4 in [-8, 1], so equal values are equal floats and
# pred / rank are decided by the index rule alone. Background -8 .. -0.25 (many ties), planted 0.5 / 1.0.
# ---------------------------------------------------------------------------------------------------
# (indices that share the row maximum), by what separates them in the kernel's thread -> column maps
# (scalar path: column v belongs to thread v % 256; float4 path: thread (v / 4) % 256)
SCALAR_PATTERNS = [
    (7, 263),          # one thread's stride (v, v + 256)
    (3, 10),           # two lanes of one wavefront
    (64, 1),           # two wavefronts (v = 1 and v = 64)
    (1026, 513, 0),    # three-way, index 0 wins
]
VEC_PATTERNS = [
    (1029, 5),         # one thread's stride (v, v + 1024)
    (300, 44, 45),     # neighbours inside one load, and another wavefront
    (256, 2),          # two wavefronts
    (8099, 4100, 3),   # the row's last column, three-way
]


def tie_pattern(r, V):
    return (VEC_PATTERNS if V % 4 == 0 else SCALAR_PATTERNS)[r % 4]


def constructed(B, T, V, seed, L=None):
    """(logits (B, T, V) fp32, caps (B, L) int64) with planted ties. Row r = b*T + t takes tie_pattern(r, V) (the
    indices that fit in V) for its maximum; odd rows also tie the target (0.5) with a lower and a higher index."""
    rng = np.random.default_rng([seed, B, T, V])
    L = T + 1 if L is None else L
    x = (rng.integers(-32, 0, size=(B, T, V)) * 0.25).astype(np.float32)
    caps = rng.integers(0, V, size=(B, L)).astype(np.int64)
    for b in range(B):
        for t in range(T):
            r = b * T + t
            top = [v for v in tie_pattern(r, V) if v < V]
            x[b, t, np.array(top, np.int64)] = 1.0
            if r % 2 == 1 and V >= 16:
                free = [v for v in range(V) if v not in top]
                lo, tgt, hi = sorted(rng.choice(len(free), size=3, replace=False))
                caps[b, t + 1] = free[tgt]
                x[b, t, [free[lo], free[tgt], free[hi]]] = 0.5
    return x, caps


ROW_SHAPES = [(B, T, V) for V in (1, 50, 257, 1027) for T in (1, 3) for B in (1, 3)] + [(1, 2, 8100), (3, 3, 260)]


def ragged_lens(B, T):
    """A full, a length-1 and a length-0 caption (B = 3); the full one alone at B = 1."""
    return [T, 1, 0][:B]


# ---------------------------------------------------------------------------------------------------
# the oracle for one caption alone at its true length (what the reference's batch-1 loop evaluates)
# ---------------------------------------------------------------------------------------------------
def oracle_caption(p, feats, cap, dtype=torch.float64):
    """p: name -> tensor (gen.decoder_params); feats (1, 14, 14, E); cap: 1-D int64 tensor START..END.
    Returns dict: loss (oracle.decoder_ref.attention_loss), logits (T, V) and alphas (T, P) numpy fp64,
    pred / rank (T,), gap (T,) = top-1 minus top-2 logit, margin (T,) = the least |x[tgt] - x[v]|, v != tgt."""
    from oracle import decoder_ref as R
    q = {k: v.to(dtype) for k, v in p.items()}
    caps = cap.view(1, -1)
    rp, rc, dl, ra = R.decoder_forward(q, feats.to(dtype), caps, [caps.shape[1]])
    loss = float(R.attention_loss(rp, rc, dl, ra))
    x = rp[0].double().numpy()
    _, pred, rank = rows_ref(x[None], caps.numpy(), dl)
    top2 = np.sort(x, axis=1)[:, -2:]
    tgt = caps[0, 1:].numpy()
    d = np.abs(x - x[np.arange(x.shape[0]), tgt][:, None])
    d[np.arange(x.shape[0]), tgt] = np.inf
    return dict(loss=loss, logits=x, alphas=ra[0].double().numpy(), pred=pred[0], rank=rank[0],
                gap=top2[:, 1] - top2[:, 0], margin=d.min(axis=1), decode_length=dl[0])


E2E = dict(A=32, D=32, M=16, V=50, lengths=[5, 8, 3, 6, 4, 8, 7], batch_size=4)


def e2e_inputs(seed):
    """7 captions of lengths 3..8 in non-sorted order with one feature map each: [(feats (14,14,E), cap)]."""
    import gen
    from helpers import t
    lengths = E2E["lengths"]
    caps = gen.captions(seed, len(lengths), max(lengths), E2E["V"], lengths=lengths)
    return [(t(gen.encoder_features(seed + i, 1))[0], t(caps[i, :n].copy())) for i, n in enumerate(lengths)]


def strip(tokens, V):
    """START / END / PAD of the synthetic vocabulary layout (pad 0, start V-3, end V-2) removed."""
    return [int(w) for w in tokens if int(w) not in (0, V - 3, V - 2)]
