"""Helper of the grouped attention-backward tests (not a test): the case lists, seeded input builders and fp64
references that tests/test_gpu_att_group.py (the kernels of csrc/att_group.hip) and
tests/test_scst_attention_cpu.py (the references themselves) share.

Row layout: image i owns rows i*n .. i*n+n-1. The references are those of tests/decoder_kernel_cases.py (ctx_bwd,
score_bwd, encgrad_ref) applied to features replicated per row; ``*_direct`` restate the same sums by indexing
the image of a row (r // n) without replicating anything, and the CPU test holds the two against each other.
Rules are that file's: ``within`` for accumulations, ``roundings`` for pointwise outputs, and the fp64 ReLU mask
of the fp32 inputs agrees with the kernel's in every element."""
import torch

import decoder_kernel_cases as DC
from decoder_kernel_cases import F64, _u, gen, roundings, slab_parts, within

# (B, n, P, A, E, S): one row; P = 13 one full slot chunk with n = 2 of the 4-arm; n = 5 of the 8-arm with P = 29
# (a tail chunk of 3 slots, waves 0..2 one each), E = 1028 one float4 in a second trip of the lane stride and S = 5
# (slab_sum's 4-wide arm over the S - 1 = 4 later slabs); n = 16 the 16-arm full with 128 KiB of LDS (E = 2048) and
# A = 260 one float4 column in a fifth column block; n = 4 the 4-arm full at the production P = 196, S = 3.
GROUP_BWD_CASES = [(1, 1, 1, 4, 4, 1), (3, 2, 13, 68, 260, 2), (2, 5, 29, 512, 1028, 5), (2, 16, 49, 260, 2048, 1),
                   (3, 4, 196, 68, 260, 3)]
GROUP_BWD_IDENTITY_CASE = GROUP_BWD_CASES[2]

# (T, B, n, P, A): A / 4 = 1 (1024 slot groups), 12 (85 groups, threads 1020..1023 idle), 128 (8 groups), 256 (4
# groups, 7 slots a thread); P = 28, 29: one full block, and a second of one slot; (26, 1, 16, 29, 512): 416 (t, j)
# pairs in 26 chunks of 16, the largest staged case; (2, 2, 3, 29, 1024): chunks of 8 pairs, the last one of 6 ending
# inside a timestep.
GROUP_ENCGRAD_CASES = [(1, 2, 1, 1, 4), (3, 3, 2, 28, 48), (3, 2, 5, 29, 512), (26, 1, 16, 29, 512), (2, 2, 3, 29, 1024)]
EPCH = 28  # slots per workgroup of capmi_att_group_enc_grad


def enc_grad_chunk(T, n, A):
    """(t, j) pairs staged at a time, and the dynamic LDS bytes asked for (csrc/att_group.hip)."""
    ch = max(1, min(T * n, 64, 8192 // A))
    return ch, (ch * A + ch * EPCH + 1024 * 4) * 4


def rep(x, n):
    return x.repeat_interleave(n, 0)


# ------------------------------------------------------------------------------------------ one timestep
def group_bwd_inputs(case):
    B, n, P, A, E, S = case
    R = B * n
    g = gen("group_bwd", case)
    alpha, _ = DC._alpha_dreg(g, R, P, 0)  # row stride 3 P
    return dict(parts=slab_parts(g, S, (R, E), S + 1.0), enc=_u(g, (B, P, E)), gate=torch.sigmoid(_u(g, (R, E), 4.0)),
                awe=_u(g, (R, E)), alpha=alpha, att_enc=_u(g, (B, P, A)), att_dec=_u(g, (R, A)), wf=_u(g, (A,)))


def group_bwd_ref(p, n, dt=F64):
    """{dgp, de, dad: (ref, mag)} of all R rows: ctx_bwd then score_bwd on the replicated features, every row live."""
    R = p["gate"].shape[0]
    out = DC.ctx_bwd(p["parts"], p["gate"], p["awe"], rep(p["enc"], n), dt)
    dalpha, mag_dalpha = out["dalpha"]
    sb = DC.score_bwd(dalpha, mag_dalpha, None, p["alpha"], rep(p["att_enc"], n), p["att_dec"], p["wf"], R, dt)
    return dict(dgp=out["dgp"], dalpha=out["dalpha"], de=sb["de"], dad=sb["dad"])


def group_bwd_direct(p, n, dt=F64):
    """The same quantities with the image of row r taken as r // n (nothing replicated)."""
    parts, enc, alpha = p["parts"], p["enc"].to(dt), p["alpha"].to(dt)
    R, B = parts.shape[1], enc.shape[0]
    img = torch.arange(R, device=enc.device) // n
    d = parts[0].to(dt)
    for s in range(1, parts.shape[0]):
        d = d + parts[s].to(dt)
    g = p["gate"].to(dt)
    dgp = d * p["awe"].to(dt) * g * (1 - g)
    dalpha = torch.stack([enc[int(img[r])] @ (d[r] * g[r]) for r in range(R)])
    de = alpha * (dalpha - (alpha * dalpha).sum(1, keepdim=True))
    x, ad = p["att_enc"].double(), p["att_dec"].double()
    dad = torch.stack([p["wf"].to(dt) * ((x[int(img[r])] + ad[r] > 0) * de[r][:, None]).sum(0) for r in range(R)])
    assert B * n == R
    return dict(dgp=dgp, dalpha=dalpha, de=de, dad=dad)


def group_bwd_compare(got, ref, S, what):
    """dgp is pointwise: the S - 1 slab adds, 1 - gate and three products."""
    roundings(got["dgp"], *ref["dgp"], S + 3, f"{what} dgp")
    for k in ("dalpha", "de", "dad"):
        if k in got:
            within(got[k], *ref[k], f"{what} {k}")


# ------------------------------------------------------------------------------------------ hoisted over t and j
def group_encgrad_inputs(case):
    T, B, n, P, A = case
    g = gen("group_encgrad", case)
    return dict(de=_u(g, (T, B * n, P)), att_enc=_u(g, (B, P, A)), att_dec=_u(g, (T, B * n, A)), wf=_u(g, (A,)))


def group_encgrad_ref(p, n, dt=F64):
    """encgrad_ref on the replicated att_enc; the per-row d(att_enc) and its magnitude summed over each group."""
    B, P, A = p["att_enc"].shape
    r = DC.encgrad_ref(dict(de=p["de"], att_enc=rep(p["att_enc"], n), att_dec=p["att_dec"], wf=p["wf"]), dt)
    val, mag = r["datt_enc"]
    return dict(datt_enc=(val.view(B, n, P, A).sum(1), mag.view(B, n, P, A).sum(1)), wf_grad=r["wf_grad"],
                bf_grad=r["bf_grad"])


def group_encgrad_direct(p, n, dt=F64):
    """datt_enc[i][p][a] = wf[a] sum_t sum_j de[t][i n + j][p] [att_enc[i][p][a] + att_dec[t][i n + j][a] > 0] and
    the full_att gradients, looping over (t, j) in the kernel's order."""
    de, x, ad, wf = p["de"].to(dt), p["att_enc"], p["att_dec"], p["wf"].to(dt)
    T, R, P = de.shape
    B, _, A = x.shape
    datt = torch.zeros(B, P, A, dtype=dt, device=x.device)
    wfg = torch.zeros(A, dtype=dt, device=x.device)
    for t in range(T):
        for j in range(n):
            rows = torch.arange(B, device=x.device) * n + j
            s = x.double() + ad[t, rows].double()[:, None, :]   # (B, P, A), fp64: the mask of the fp32 inputs
            d = de[t, rows][:, :, None]
            datt += (s > 0) * d
            wfg += (torch.relu(x.to(dt) + ad[t, rows].to(dt)[:, None, :]) * d).sum((0, 1))
    return dict(datt_enc=datt * wf, wf_grad=wfg, bf_grad=de.sum())


def group_encgrad_compare(got, ref, what):
    for k in got:
        within(got[k], *ref[k], f"{what} {k}")
