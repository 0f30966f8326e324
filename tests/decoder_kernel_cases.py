"""Helper of the decoder non-GEMM kernel tests (not a test): the case lists, the seeded input builders, the
fp64 references and the comparison rules that tests/test_gpu_decoder_kernels.py (the kernels of
csrc/decoder.hip, the two fused attention kernels of csrc/decoder_step.hip and csrc/optim.hip) and
tests/test_decoder_kernel_cases_cpu.py (the references and rules themselves) share.

Every reference takes the fp32 tensors that are handed to the kernel, upcasts them to ``dt`` = fp64 and
computes there, on whatever device the tensors live. Called with ``dt`` = fp32 the same function is the CPU
emulation of the kernel (sequential slab sums, plain fp32 torch otherwise), and with ``bug=...`` the
emulation of one plausible kernel bug; ReLU masks and magnitudes are always formed in fp64.

Rules: ``exact``, ``within``, ``one_rounding`` of encoder_kernel_cases, and

  roundings   |got - ref| <= k * ulp * mag, no absolute floor: k fp32 operations on the path to the output,
              each a rounding of a value no larger than mag. A transcendental (expf, logf, tanhf, __expf)
              counts as 4 roundings of its result, and exp(x) as |x| more (the rounding of its argument).

``within`` (4e-6 = 67 ulp of the summed term magnitudes, + 1e-6) is the project's rule for an fp32
accumulation (tests/test_gpu_gemm.py::check) and is used for every O(1) sum here; the magnitude of an output
computed from rounded intermediates is the first-order propagation of theirs (|d out / d in| * mag_in summed).
Where an output is a difference that cancels, mag is the sum of the magnitudes of what is subtracted.

ReLU kinks excuse nothing: every backward kernel masks by the sign of the one fp32 add att_enc + att_dec of
final fp32 inputs, and the sign of a rounded sum of two floats is the sign of the exact sum, so the
reference's fp64 mask must agree in every element."""
import math
import zlib

import torch

from encoder_kernel_cases import RATIOS, _ratio, _u, case_id, exact, fma32, one_rounding, within  # noqa: F401

F64 = torch.float64
ULP = 2.0 ** -24
NAN = float("nan")


def roundings(got, ref, mag, k, what, ulp=ULP):
    return _ratio(got, ref, k * ulp * mag.double(), what, f"roundings k={k}")


def all_zero(x, what):
    """Exactly zero (either sign: w * +0 is -0 for a negative w)."""
    assert bool((x == 0).all()), f"{what}: {int((x != 0).sum())} elements are not zero"


def gen(tag, case):
    return torch.Generator().manual_seed(zlib.crc32(f"{tag}:{case_id(case)}".encode()))


def padded(t, ld):
    """t (rows, cols) as the leading columns of a NaN-filled (rows, ld) buffer: a view whose row stride is ld."""
    base = torch.full((t.shape[0], ld), NAN, dtype=t.dtype)
    base[:, :t.shape[1]] = t
    return base[:, :t.shape[1]]


def slab_parts(g, S, shape, scale=1.0, pad=8):
    """S split-K partial slabs (S, *shape), each drawn in scale / (S + 1) * [-1, 1] so that a bias drawn the
    same way plus all of them stays within [-scale, scale]; the slab stride is numel + pad, the pad NaN."""
    if S == 0:
        return None
    n = math.prod(shape)
    return padded(_u(g, (S, n), scale / (S + 1)), n + pad).unflatten(1, shape)


def slab_total(parts, init, dt=F64, drop_last=False):
    """init + parts[0] + parts[1] + ... added in slab order in dt (slab_sum's order), and the summed
    magnitudes. ``drop_last``: the bug of the last slab never added."""
    S = 0 if parts is None else parts.shape[0]
    ref = parts[0] if init is None else init
    acc, mag = torch.zeros_like(ref, dtype=dt), torch.zeros_like(ref, dtype=F64)
    if init is not None:
        acc, mag = acc + init.to(dt), mag + init.double().abs()
    for s in range(S - 1 if drop_last else S):
        acc, mag = acc + parts[s].to(dt), mag + parts[s].double().abs()
    return acc, mag


# ------------------------------------------------------------------------------------------ planned paths
PCH_T, PCH, DIN_PB = 13, 28, 8  # rows per workgroup of att_score_fwd / att_ctx_bwd, att_enc_grad, att_enc_dinput


def slab_arms(S):
    """(trips of the 8-wide loop, 4-wide arm taken, trips of the 1-wide loop) of slab_sum (csrc/common.h)."""
    return S // 8, S % 8 >= 4, S % 8 - 4 * (S % 8 >= 4)


def chunks(P, per):
    """(workgroups along P, rows of the last one)"""
    n = (P + per - 1) // per
    return n, P - (n - 1) * per


def enc_grad_plan(A):
    """(A / 4, p-groups, idle threads) of att_enc_grad_kernel; A / 4 = 256 is its one-group arm."""
    A4 = A // 4
    ngrp = max(1, 256 // A4)
    return A4, ngrp, 256 - ngrp * A4


def enc_grad_lds(T, A):
    """dynamic LDS bytes capmi_att_enc_grad asks for"""
    return (T * A + T * PCH + 256 * 4) * 4


# ============================================================================================ part A
# ------------------------------------------------------------------------------------------ mean_rows
MEAN_CASES = [(2, 1, 4), (3, 5, 260), (2, 49, 2048)]  # (B, P, E)


def mean_inputs(case):
    B, P, E = case
    return dict(enc=_u(gen("mean", case), (B, P, E)))


def mean_ref(p, dt=F64):
    e = p["enc"]
    return dict(mean=(e.to(dt).mean(1), e.double().abs().mean(1)))


def mean_compare(got, ref, what):
    within(got["mean"], *ref["mean"], f"{what} mean")


# ------------------------------------------------------------------------------------------ scores
def _scaled_wf(att_enc, ad, wf, limit=1.5):
    """wf rescaled so that the scores relu(att_enc + ad) . wf stay within [-limit, limit] (then bf within 0.5)"""
    e = (torch.relu(att_enc.double() + ad.double()[:, None, :]) * wf.double()).sum(-1)
    return (wf.double() * (limit / max(float(e.abs().max()), 1e-3))).float()


def kink_mask(att_enc, att_dec):
    """[att_enc + att_dec > 0] from the fp64 sum of the fp32 inputs; att_dec (B, A) or (T, B, A)"""
    ad = att_dec.double()
    return att_enc.double() + (ad[:, None, :] if ad.dim() == 2 else ad[:, :, None, :]) > 0


def scores(att_enc, ad, mag_ad, wf, bf, dt):
    """e[b][p] = relu(att_enc[b][p] + ad[b]) . wf + bf and its magnitude: each term |x + ad| |wf| plus the
    att_dec sum's own magnitude where the ReLU passes (its rounding reaches e through the mask)."""
    s = att_enc.to(dt) + ad.to(dt)[:, None, :]
    e = (torch.relu(s) * wf.to(dt)).sum(-1)
    s64 = att_enc.double() + ad.double()[:, None, :]
    mag = ((s64.abs() + mag_ad[:, None, :]) * (s64 > 0) * wf.double().abs()).sum(-1)
    if bf is not None:
        e, mag = e + bf.to(dt), mag + bf.double().abs()
    return e, mag


# (B, P, A, S, bias_da, bf, att_dec_out): P = 13 one full chunk, 14 and 29 a tail chunk of 1 and 3 rows (29: wave
# 0 owns rows 26, wave 1 27, wave 2 28); A = 260 a second trip of the 256-float lane stride for lane 0 alone;
# S = 1, 3, 4, 8, 13: slab_sum's 1-wide, 4-wide, 8-wide arms alone and all three together
SCORE_CASES = [(2, 1, 4, 1, 0, 0, 0), (3, 13, 260, 3, 1, 1, 1), (2, 14, 512, 4, 1, 0, 1), (3, 29, 260, 8, 0, 1, 0),
               (2, 29, 512, 13, 1, 1, 1)]


def score_inputs(case):
    B, P, A, S, bias, bf, _ = case
    g = gen("score", case)
    p = dict(att_enc=_u(g, (B, P, A)), parts=slab_parts(g, S, (B, A)),
             bias_da=_u(g, (A,), 1.0 / (S + 1)) if bias else None, bf=_u(g, (1,), 0.5) if bf else None)
    p["wf"] = _scaled_wf(p["att_enc"], slab_total(p["parts"], p["bias_da"])[0].float(), _u(g, (A,)))
    return p


def score_ref(p, dt=F64, bug=None):
    ad, mag_ad = slab_total(p["parts"], p["bias_da"], dt, drop_last=bug == "drop_last_slab")
    e, mag_e = scores(p["att_enc"], ad, mag_ad, p["wf"], p["bf"], dt)
    if bug == "drop_tail_rows":  # the last chunk of PCH_T rows never written (a zeroed buffer)
        e = e.clone()
        e[:, (e.shape[1] - 1) // PCH_T * PCH_T:] = 0
    return dict(e=(e, mag_e), att_dec=(ad, mag_ad))


def score_compare(got, ref, S, what):
    within(got["e"], *ref["e"], f"{what} e")
    if "att_dec" in got:  # k = S: the S adds of bias + partials (the first is exact without a bias)
        roundings(got["att_dec"], *ref["att_dec"], S, f"{what} att_dec_out")


# ------------------------------------------------------------------------------------------ softmax, context, gate
def softmax_ctx(e, mag_e, enc, bt, gate, mag_gate, dt, bug=None):
    """alpha = softmax(e) (rows b >= bt reported as zero), awe = sum_p alpha enc, x = gate * awe.
    mag_e: the magnitude of the scores where the kernel computed them itself (None: e is an input). A score
    error d reaches alpha as alpha_p (d_p - sum_q alpha_q d_q), at most 2 alpha_p max|d|, so alpha and
    everything after it carry the factor amp = 1 + 2 max_p mag_e."""
    B, P = e.shape
    ed = e.to(dt)
    ex = torch.exp(ed - ed.max(1, keepdim=True).values)
    alpha = ex / ex.sum(1, keepdim=True)
    a64 = torch.softmax(e.double(), 1)
    amp = torch.ones(B, 1, dtype=F64, device=e.device) if mag_e is None else 1 + 2 * mag_e.max(1, keepdim=True).values
    w = alpha[:, :, None] * enc.to(dt)
    if bug == "skip_pgroup3":  # rows 3, 7, 11, ... left out of the context sum
        w[:, 3::4] = 0
    awe, mag_awe = w.sum(1), amp * (a64[:, :, None] * enc.double().abs()).sum(1)
    live = (torch.arange(B, device=e.device) < bt)[:, None]
    out = dict(alpha=(alpha if bug == "bt_ignored" else alpha * live, amp * a64), awe=(awe, mag_awe))
    if gate is None:
        out["x"] = (awe, mag_awe)
    else:  # d(g awe) = g d awe + awe d g, |g| <= 1, |awe| <= mag_awe
        out["x"] = (gate.to(dt) * awe, mag_awe * (1 + mag_gate))
    return out


def gate_act(parts, bias, dt, drop_last=False):
    """sigmoid(bias + partials) and its magnitude: the pre-activation's (Lipschitz constant 1/4 < 1) + 1."""
    pre, mag = slab_total(parts, bias, dt, drop_last)
    return torch.sigmoid(pre), mag + 1


# (B, P, E, bt, S, gate_out, x_out, awe_out); S = 0: no gate. P = 257 a second trip of the 256-thread softmax
# loops for thread 0; P = 5 leaves p-group 0 two rows and the rest one; E = 260 one float4 column in a second
# column block. alpha_out is always strided by 3 P, x_out by E + 12.
SOFTCTX_CASES = [(2, 1, 4, 0, 0, 0, 1, 1), (3, 5, 260, 2, 4, 1, 1, 1), (2, 257, 2048, 2, 13, 1, 1, 0),
                 (3, 5, 2048, 3, 1, 0, 1, 1), (3, 257, 260, 2, 0, 0, 0, 1)]


def softctx_inputs(case):
    B, P, E, bt, S, _, _, _ = case
    g = gen("softctx", case)
    return dict(e=_u(g, (B, P), 2.0), enc=_u(g, (B, P, E)), gate_parts=slab_parts(g, S, (B, E), 4.0),
                bias_fb=_u(g, (E,), 4.0 / (S + 1)) if S else None)


def softctx_ref(p, bt, dt=F64, bug=None):
    gate = mag_gate = None
    if p["gate_parts"] is not None:
        gate, mag_gate = gate_act(p["gate_parts"], p["bias_fb"], dt, bug == "drop_last_slab")
    out = softmax_ctx(p["e"], None, p["enc"], bt, gate, mag_gate, dt, bug)
    if gate is not None:
        out["gate"] = (gate, mag_gate)
    return out


def softctx_compare(got, ref, bt, what):
    for k in got:
        within(got[k], *ref[k], f"{what} {k}")
    if "alpha" in got:
        all_zero(got["alpha"][bt:], f"{what} alpha rows b >= bt")


# (B, P, A, E, S_a, S_g, bt, ad_out, gate_out, awe_out, alpha_out): S_a = 0 takes att_dec final, S_g = 0 the gate
# final. P = 8, 9: one row per wave, and wave 0 alone a second; 49, 56: the production size and the kernel's limit
# (7 score rows per wave, 14 context rows per thread). E = 516: one float4 column in a second 512-column block.
FWDF_CASES = [(2, 1, 4, 4, 0, 0, 0, 0, 0, 0, 1), (3, 8, 260, 516, 3, 4, 2, 1, 1, 1, 1), (2, 9, 512, 2048, 8, 0, 2, 1, 0, 1, 1),
              (3, 49, 512, 2048, 3, 4, 3, 1, 1, 0, 1), (2, 56, 260, 516, 0, 0, 2, 1, 0, 1, 0), (3, 56, 4, 4, 3, 4, 0, 1, 1, 1, 1),
              (2, 49, 4, 516, 8, 0, 2, 0, 0, 1, 1), (3, 1, 512, 4, 0, 0, 3, 0, 0, 1, 1), (2, 9, 260, 2048, 3, 4, 0, 1, 0, 0, 1),
              (3, 8, 512, 516, 8, 0, 2, 1, 0, 1, 0)]


def fwdf_inputs(case):
    B, P, A, E, S_a, S_g = case[:6]
    g = gen("fwdf", case)
    p = dict(att_enc=_u(g, (B, P, A)), enc=_u(g, (B, P, E)), bf=_u(g, (1,), 0.5))
    if S_a:
        p["ad_parts"], p["bias_da"] = slab_parts(g, S_a, (B, A)), _u(g, (A,), 1.0 / (S_a + 1))
        ad = slab_total(p["ad_parts"], p["bias_da"])[0].float()
    else:
        p["ad"] = ad = _u(g, (B, A))
    p["wf"] = _scaled_wf(p["att_enc"], ad, _u(g, (A,)))
    if S_g:
        p["gate_parts"], p["bias_fb"] = slab_parts(g, S_g, (B, E), 4.0), _u(g, (E,), 4.0 / (S_g + 1))
    else:
        p["gate"] = torch.sigmoid(_u(g, (B, E), 4.0))
    return p


def fwdf_ref(p, bt, dt=F64, bug=None):
    if "ad" in p:
        ad, mag_ad = p["ad"].to(dt), torch.zeros_like(p["ad"], dtype=F64)  # final: no rounding of its own
    else:
        ad, mag_ad = slab_total(p["ad_parts"], p["bias_da"], dt, bug == "drop_last_slab")
    e, mag_e = scores(p["att_enc"], ad, mag_ad, p["wf"], p["bf"], dt)
    if "gate" in p:
        gate, mag_gate = p["gate"].to(dt), torch.zeros_like(p["gate"], dtype=F64)
    else:
        gate, mag_gate = gate_act(p["gate_parts"], p["bias_fb"], dt, bug == "drop_last_slab")
    out = softmax_ctx(e, mag_e, p["enc"], bt, gate, mag_gate, dt, bug)
    out["ad"] = (ad, mag_ad)
    out["gate"] = (gate, mag_gate)
    return out


def fwdf_compare(got, ref, p, bt, what):
    for k in got:
        if k == "ad":
            if "ad" in p:
                exact(got[k], p["ad"].to(got[k].device), f"{what} ad_out (a copy)")
            else:
                roundings(got[k], *ref[k], p["ad_parts"].shape[0], f"{what} ad_out")
        else:
            within(got[k], *ref[k], f"{what} {k}")
    if "alpha" in got:
        all_zero(got["alpha"][bt:], f"{what} alpha rows b >= bt")


# ------------------------------------------------------------------------------------------ attention backward
def ctx_bwd(parts, gate, awe, enc, dt, bug=None):
    """d = sum of the partials; dawe = d gate; dgp = d awe gate (1 - gate); dalpha[b][p] = dawe[b] . enc[b][p].
    1 - gate rounds to within an ulp of itself (exact for gate >= 1/2, a value in [1/2, 1] below)."""
    d, mag_d = slab_total(parts[1:] if parts.shape[0] > 1 else None, parts[0], dt, bug == "drop_last_slab")
    out = {}
    dawe, mag_dawe = d, mag_d
    if gate is not None:
        g = gate.to(dt)
        dawe, mag_dawe = d * g, mag_d * gate.double()
        out["dgp"] = (d * awe.to(dt) * g * (1 - g), mag_d * awe.double().abs() * gate.double() * (1 - gate.double()))
    out["dawe"] = (dawe, mag_dawe)
    w = enc.to(dt) * dawe[:, None, :]
    out["dalpha"] = (w.sum(-1), (enc.double().abs() * mag_dawe[:, None, :]).sum(-1))
    if bug == "drop_tail_rows":
        out["dalpha"][0][:, (enc.shape[1] - 1) // PCH_T * PCH_T:] = 0
    return out


def score_bwd(dalpha, mag_dalpha, dreg, alpha, att_enc, att_dec, wf, bt, dt, bug=None):
    """da = dalpha + dreg, s = sum_p alpha da, de = alpha (da - s) (zero for b >= bt),
    dad[b][a] = wf[a] sum_p de[b][p] [att_enc[b][p][a] + att_dec[b][a] > 0]. de cancels: its magnitude is
    alpha (mag_da + sum_p alpha mag_da)."""
    B, P = dalpha.shape
    al, da, mag_da = alpha.to(dt), dalpha.to(dt), mag_dalpha
    if dreg is not None:
        da, mag_da = da + dreg.to(dt), mag_da + dreg.double().abs()
    s = (al * da).sum(1, keepdim=True)
    live = (torch.arange(B, device=dalpha.device) < bt)[:, None]
    de = al * (da - s) * (1 if bug == "bt_ignored" else live)
    mag_de = alpha.double() * (mag_da + (alpha.double() * mag_da).sum(1, keepdim=True))
    mask = kink_mask(att_enc, att_dec)
    w = mask * de[:, :, None]
    if bug == "drop_tail_rows":  # rows 26..28 of P = 29 left out of the sum over p
        w[:, 26:] = 0
    dad = wf.to(dt) * w.sum(1)
    return dict(de=(de, mag_de), dad=(dad, wf.double().abs() * (mask * mag_de[:, :, None]).sum(1)))


# (B, P, E, S, gate mode, dawe_out): gate mode 0 none, 1 gate and dgp, 2 gate without dgp. E = 1028: one float4 in
# a second trip of the 1024-float staging loop. slab_sum runs over the S - 1 slabs after the first: 0, 1, 4, 8.
CTXB_CASES = [(2, 1, 4, 1, 0, 1), (3, 13, 1028, 2, 1, 1), (2, 14, 2048, 5, 2, 0), (3, 29, 1028, 9, 1, 0), (2, 29, 4, 2, 0, 0)]


def ctxb_inputs(case):
    B, P, E, S, gm, _ = case
    g = gen("ctxb", case)
    p = dict(parts=slab_parts(g, S, (B, E), S + 1.0), enc=_u(g, (B, P, E)), gate=None, awe=None)
    if gm:
        p["gate"], p["awe"] = torch.sigmoid(_u(g, (B, E), 4.0)), _u(g, (B, E))
    return p


def ctxb_ref(p, dt=F64, bug=None):
    return ctx_bwd(p["parts"], p["gate"], p["awe"], p["enc"], dt, bug)


def ctxb_compare(got, ref, what):
    for k in got:
        within(got[k], *ref[k], f"{what} {k}")


# (B, P, A, bt, dreg): A = 68: a second 64-column block of one float4; P = 17: p-group 0 two rows, the rest one;
# P = 257: a second trip of the 256-thread loops. alpha is strided by 3 P, dreg by P + 8.
SCOREB_CASES = [(2, 1, 4, 0, 0), (3, 17, 68, 1, 1), (2, 257, 512, 2, 1), (3, 257, 68, 3, 0), (3, 29, 68, 3, 1)]


def _alpha_dreg(g, B, P, dreg):
    alpha = padded(torch.softmax(_u(g, (B, P), 2.0).double(), 1).float(), 3 * P)
    return alpha, (padded(_u(g, (B, P), 0.05), P + 8) if dreg else None)


def scoreb_inputs(case):
    B, P, A, bt, dreg = case
    g = gen("scoreb", case)
    alpha, dr = _alpha_dreg(g, B, P, dreg)
    return dict(dalpha=_u(g, (B, P)), alpha=alpha, dreg=dr, att_enc=_u(g, (B, P, A)), att_dec=_u(g, (B, A)),
                wf=_u(g, (A,)))


def scoreb_ref(p, bt, dt=F64, bug=None):
    alpha = p["alpha"]
    if bug == "alpha_ld_is_P":  # the row stride taken as P: row b read at b * P of the strided buffer
        flat = alpha._base.reshape(-1)
        B, P = alpha.shape
        alpha = torch.nan_to_num(torch.stack([flat[b * P:(b + 1) * P] for b in range(B)]))
    return score_bwd(p["dalpha"], p["dalpha"].double().abs(), p["dreg"], alpha, p["att_enc"], p["att_dec"], p["wf"],
                     bt, dt, bug)


def scoreb_compare(got, ref, bt, what):
    within(got["de"], *ref["de"], f"{what} de")
    within(got["dad"], *ref["dad"], f"{what} dad")
    all_zero(got["de"][bt:], f"{what} de rows b >= bt")
    all_zero(got["dad"][bt:], f"{what} dad rows b >= bt")


# (B, P, A, E, S, gate mode, bt, dreg, dawe_out): S = 0 takes d(awe) final (no gate, no dawe_out). P = 16, 17, 33:
# one row per wave, wave 0 a second, wave 0 a second trip; 56 the fused forward's limit. E = 4100: one float4 in a
# second trip of the 4096-float staging loop. A = 260: a second 64-column pass with one column.
BWDF_CASES = [(2, 1, 4, 4, 0, 0, 0, 0, 0), (3, 16, 260, 2048, 1, 1, 1, 1, 1), (2, 17, 260, 4100, 5, 1, 2, 1, 1),
              (3, 33, 512, 2048, 5, 2, 3, 0, 0), (2, 56, 260, 2048, 5, 1, 2, 1, 1), (3, 56, 4, 4, 1, 0, 1, 1, 1),
              (2, 33, 512, 4100, 0, 0, 2, 1, 0)]
BWDF_IDENTITY_CASES = [BWDF_CASES[2], BWDF_CASES[4]]  # P = 17 and 56, A = 260, gate with dgp, S = 5


def bwdf_inputs(case):
    B, P, A, E, S, gm, bt, dreg, _ = case
    g = gen("bwdf", case)
    alpha, dr = _alpha_dreg(g, B, P, dreg)
    p = dict(parts=slab_parts(g, max(S, 1), (B, E), max(S, 1) + 1.0), enc=_u(g, (B, P, E)), gate=None, awe=None,
             alpha=alpha, dreg=dr, att_enc=_u(g, (B, P, A)), att_dec=_u(g, (B, A)), wf=_u(g, (A,)))
    if gm:
        p["gate"], p["awe"] = torch.sigmoid(_u(g, (B, E), 4.0)), _u(g, (B, E))
    return p


def bwdf_ref(p, bt, dt=F64, bug=None):
    out = ctx_bwd(p["parts"], p["gate"], p["awe"], p["enc"], dt, bug)
    dalpha, mag_dalpha = out.pop("dalpha")
    out.update(score_bwd(dalpha, mag_dalpha, p["dreg"], p["alpha"], p["att_enc"], p["att_dec"], p["wf"], bt, dt, bug))
    return out


def bwdf_compare(got, ref, bt, what):
    for k in got:
        within(got[k], *ref[k], f"{what} {k}")
    all_zero(got["de"][bt:], f"{what} de rows b >= bt")
    all_zero(got["dad"][bt:], f"{what} dad rows b >= bt")


# (B, P, T, E, dmean): P = 8, 9: one full block of 8 rows, and a second with one; E = 1028: two z-blocks. alpha is
# (B, T, P) with the batch stride T P + 4.
DINPUT_CASES = [(2, 1, 1, 4, 0), (3, 8, 4, 1028, 1), (2, 9, 4, 4, 1), (3, 29, 1, 1028, 0), (2, 29, 4, 1028, 1)]


def dinput_inputs(case):
    B, P, T, E, dm = case
    g = gen("dinput", case)
    alpha = torch.softmax(_u(g, (B, T, P), 2.0).double(), 2).float()
    return dict(alpha=padded(alpha.reshape(B, T * P), T * P + 4).unflatten(1, (T, P)), dawe=_u(g, (T, B, E)),
                dmean=_u(g, (B, E)) if dm else None)


def dinput_ref(p, dt=F64, bug=None):
    """denc[b][p][e] = sum_t alpha[b][t][p] dawe[t][b][e] + dmean[b][e] / P"""
    al, dw = p["alpha"], p["dawe"]
    P = al.shape[2]
    denc = torch.einsum("btp,tbe->bpe", al.to(dt), dw.to(dt))
    mag = torch.einsum("btp,tbe->bpe", al.double(), dw.double().abs())
    if p["dmean"] is not None:
        dm = p["dmean"].to(dt)[:, None, :]
        denc, mag = denc + (dm if bug == "dmean_not_divided" else dm / P), mag + p["dmean"].double().abs()[:, None, :] / P
    return dict(denc=(denc, mag))


def dinput_compare(got, ref, what):
    within(got["denc"], *ref["denc"], f"{what} denc")


# (B, P, T, A): A / 4 = 1 (256 p-groups), 12 (21 p-groups, threads 252..255 idle), 128 (2 p-groups), 256 (the
# one-group arm); P = 28, 29: one full block, and a second of one row. The last case asks for 88.4 KiB of dynamic
# LDS: the branch that raises the kernel's limit above 64 KiB.
ENCGRAD_CASES = [(2, 1, 1, 4), (3, 28, 3, 48), (2, 29, 3, 512), (2, 29, 1, 1024), (3, 29, 3, 48), (1, 29, 40, 512)]
ENCGRAD_BIG_LDS = ENCGRAD_CASES[-1]


def encgrad_inputs(case):
    B, P, T, A = case
    g = gen("encgrad", case)
    return dict(de=_u(g, (T, B, P)), att_enc=_u(g, (B, P, A)), att_dec=_u(g, (T, B, A)), wf=_u(g, (A,)))


def encgrad_ref(p, dt=F64, bug=None):
    """datt_enc[b][p][a] = wf[a] sum_t de[t][b][p] [s > 0], wf_grad[a] = sum_tbp de relu(s), bf_grad = sum de,
    s = att_enc[b][p][a] + att_dec[t][b][a]"""
    de, x, ad, wf = p["de"], p["att_enc"], p["att_dec"], p["wf"]
    mask = kink_mask(x, ad)  # (T, B, P, A)
    d = de.to(dt)[..., None]
    s = torch.relu(x.to(dt) + ad.to(dt)[:, :, None, :])
    s64 = torch.relu(x.double() + ad.double()[:, :, None, :])
    rows = slice(0, 26 if bug == "drop_tail_rows" else None)
    return dict(datt_enc=(wf.to(dt) * (mask * d).sum(0), wf.double().abs() * (mask * de.double().abs()[..., None]).sum(0)),
                wf_grad=((d * s)[:, :, rows].sum((0, 1, 2)), (de.double().abs()[..., None] * s64).sum((0, 1, 2))),
                bf_grad=(de.to(dt)[:, :, rows].sum(), de.double().abs().sum()))


def encgrad_compare(got, ref, what):
    for k in got:
        within(got[k], *ref[k], f"{what} {k}")


# ============================================================================================ part B
# ------------------------------------------------------------------------------------------ LSTM cell
# (B, D, S, S2, xemb): D = 1, 5, 48: not a multiple of the 64-lane workgroup; (70, 48): 53 workgroups, the last
# half full; slab_sum arms: S = 1, 0, 13 and S2 = 1, 3, 4
LSTM_FWD_CASES = [(1, 1, 1, 1, 0), (3, 5, 0, 3, 1), (2, 64, 13, 4, 1), (70, 48, 1, 1, 1), (70, 48, 13, 4, 0), (3, 5, 13, 4, 0),
                  (2, 64, 0, 3, 0)]


def lstm_fwd_inputs(case):
    B, D, S, S2, xe = case
    g = gen("lstm_fwd", case)
    n = S + S2 + 1  # every term within 4 / n: the pre-activations stay within [-4, 4]
    return dict(parts=slab_parts(g, S, (B, 4 * D), 4.0 * (S + 1) / n), xemb=_u(g, (B, 4 * D), 4.0 / n) if xe else None,
                hh_parts=slab_parts(g, S2, (B, 4 * D), 4.0 * (S2 + 1) / n), c_prev=_u(g, (B, D)))


def lstm_fwd_ref(p, dt=F64, bug=None):
    """gates (i, f, g, o) = xemb + partials + hh partials; c = f c_prev + i g; h = o tanh(c); act = the four
    activations. Magnitudes by first-order propagation: an activation's is the pre-activation's + 1 (Lipschitz
    constant <= 1), c's |c_prev| mag_f + mag_i + mag_g + |c_prev| + 1, h's mag_o + mag_c."""
    B, D = p["c_prev"].shape
    v, mag_v = slab_total(p["parts"], p["xemb"], dt) if (p["parts"] is not None or p["xemb"] is not None) else (None, None)
    pre, mag = slab_total(p["hh_parts"], v, dt, bug == "drop_last_slab")
    if mag_v is not None:
        mag = mag - v.double().abs() + mag_v
    pre, mag = pre.view(B, 4, D), mag.view(B, 4, D) + 1
    if bug == "swap_f_g":
        pre = pre[:, [0, 2, 1, 3]]
    ig, fg, cg, og = torch.sigmoid(pre[:, 0]), torch.sigmoid(pre[:, 1]), torch.tanh(pre[:, 2]), torch.sigmoid(pre[:, 3])
    cp = p["c_prev"].to(dt)
    c = fg * cp + ig * cg
    mag_c = p["c_prev"].double().abs() * (mag[:, 1] + 1) + mag[:, 0] + mag[:, 2] + 1
    return dict(act=(torch.stack([ig, fg, cg, og], 1).reshape(B, 4 * D), mag.reshape(B, 4 * D)), c=(c, mag_c),
                h=(og * torch.tanh(c), mag[:, 3] + mag_c))


def lstm_fwd_compare(got, ref, what):
    for k in got:
        within(got[k], *ref[k], f"{what} {k}")


# (B, D, bt, dhd, dc_in, S)
LSTM_BWD_CASES = [(1, 1, 0, 1, 1, 1), (3, 5, 1, 0, 1, 5), (2, 64, 2, 1, 0, 0), (70, 48, 70, 1, 1, 5), (70, 48, 1, 0, 0, 1),
                  (3, 5, 3, 1, 1, 0)]


def lstm_bwd_inputs(case):
    B, D, bt, dhd, dci, S = case
    g = gen("lstm_bwd", case)
    f = lstm_fwd_ref(lstm_fwd_inputs((B, D, 1, 1, 1)))
    return dict(act=f["act"][0].float(), c_cur=f["c"][0].float(), c_prev=lstm_fwd_inputs((B, D, 1, 1, 1))["c_prev"],
                dh_parts=slab_parts(g, S, (B, D)), dhd=_u(g, (B, D)) if dhd else None, dc_in=_u(g, (B, D)) if dci else None)


def lstm_bwd_ref(p, bt, dt=F64, bug=None):
    """The LSTMCell backward from the saved activations: dh = dhd + partials; d_o = dh tanh(c) o (1 - o);
    dc = dc_in + dh o (1 - tanh(c)^2); d_i = dc g i (1 - i); d_f = dc c_prev f (1 - f); d_g = dc i (1 - g^2);
    dc_out = dc f. Rows b >= bt are zero. 1 - x of a value in [0, 1] rounds within an ulp of itself and
    1 - x^2 within a few ulp of 1, so those factors enter the magnitudes as they are, or as 1."""
    B, D = p["c_prev"].shape
    if p["dh_parts"] is None and p["dhd"] is None:
        dh, mag_dh = torch.zeros(B, D, dtype=dt, device=p["act"].device), torch.zeros(B, D, dtype=F64, device=p["act"].device)
    else:
        dh, mag_dh = slab_total(p["dh_parts"], p["dhd"], dt, bug == "drop_last_slab")
    a, a64 = p["act"].to(dt).view(B, 4, D), p["act"].double().view(B, 4, D)
    ig, fg, cg, og = (a[:, j] for j in ([0, 2, 1, 3] if bug == "swap_f_g" else range(4)))
    i64, f64, g64, o64 = (a64[:, j] for j in range(4))
    tc, cp = torch.tanh(p["c_cur"].to(dt)), p["c_prev"].to(dt)
    dc = dh * og * (1 - tc * tc)
    mag_dc = mag_dh * o64
    if p["dc_in"] is not None:
        dc, mag_dc = p["dc_in"].to(dt) + dc, mag_dc + p["dc_in"].double().abs()
    live = (torch.arange(B, device=a.device) < bt)[:, None]
    if bug == "bt_ignored":
        live = torch.ones_like(live)
    dg = torch.stack([dc * cg * ig * (1 - ig), dc * cp * fg * (1 - fg), dc * ig * (1 - cg * cg), dh * tc * og * (1 - og)], 1)
    mag = torch.stack([mag_dc * g64.abs() * i64, mag_dc * p["c_prev"].double().abs() * f64, mag_dc * i64, mag_dh * o64], 1)
    return dict(dgates=((dg * live[:, None]).reshape(B, 4 * D), mag.reshape(B, 4 * D)), dc_out=(dc * fg * live, mag_dc * f64))


def lstm_bwd_compare(got, ref, bt, what):
    for k in got:
        within(got[k], *ref[k], f"{what} {k}")
        all_zero(got[k][bt:], f"{what} {k} rows b >= bt")


# ------------------------------------------------------------------------------------------ cross entropy
CE_B, CE_T, CE_L = 3, 4, 7  # the caption stride differs from T + 1
CE_BT = [3, 3, 2, 1]
# (V, bt, time-major dlogits, gscale, lse, dlogits): V = 256, 257: one trip of the 256-thread loops, and a second
# for thread 0; 8100 the production vocabulary (32 trips)
CE_CASES = [(1, 0, 0, 0, 1, 1), (7, 1, 1, 1, 1, 1), (256, 0, 1, 0, 0, 1), (257, 1, 0, 1, 1, 0), (8100, 1, 1, 1, 1, 1),
            (8100, 0, 0, 0, 1, 1), (7, 1, 0, 0, 0, 0)]
CE_GSCALE = 0.37


def ce_inputs(case):
    V, bt, tm, gs, _, _ = case
    g = gen("ce", case)
    caps = torch.randint(0, V, (CE_B, CE_L), generator=g)
    caps[0, 1], caps[1, 2] = 0, V - 1  # targets 0 and V - 1 both occur (rows (0, 0) and (1, 1): active under CE_BT)
    return dict(logits=_u(g, (CE_B, CE_T, V), 4.0), caps=caps, bt=torch.tensor(CE_BT, dtype=torch.int32) if bt else None,
                gscale=torch.tensor([CE_GSCALE]) if gs else None, nrows=sum(CE_BT) if bt else CE_B * CE_T, tm=tm)


def ce_k(V, lse_abs, arg_abs):
    """fp32 operations on the path to dlogits. The row sum s: one term's sub + expf + its argument (<= 8) = 13, the
    online chain's rescale and add per trip 2 ceil(V / 256), the final rescale s * expf(m - gm) 14, wave_sum 6 and
    block_sum 4: s is relative to k_s = 37 + 2 ceil(V / 256). lse = gm + logf(s): k_s + 4 |log s| + |lse|, taken
    as k_s + 5 |lse| (absolute, in ulp of 1). Then expf(x - lse): the sub rounds |x - lse|, expf 4; - onehot 1;
    * g 1; g = gscale / nrows 2."""
    return 37 + 2 * ((V + 255) // 256) + math.ceil(5 * lse_abs) + math.ceil(arg_abs) + 8


def ce_ref(p, dt=F64, bug=None):
    x, caps = p["logits"].to(dt), p["caps"].to(p["logits"].device)
    B, T, V = x.shape
    off = 0 if bug == "target_at_t" else 1
    tgt = caps[:, off:T + off]
    lse = torch.logsumexp(x, -1)
    xt = x.gather(2, tgt[..., None])[..., 0]
    dev = x.device
    live = torch.ones(B, T, dtype=torch.bool, device=dev) if p["bt"] is None else \
        torch.arange(B, device=dev)[:, None] < p["bt"].to(dev)[None, :]
    onehot = torch.zeros_like(x).scatter_(2, tgt[..., None], 1.0)
    g = (float(p["gscale"]) if p["gscale"] is not None else 1.0) / p["nrows"]
    prob = torch.exp(x - lse[..., None])
    dl, mag_dl = (prob - onehot) * g * live[..., None], (prob.double() + onehot.double()) * g
    if bool(p["tm"]) != (bug == "batch_major"):
        dl = dl.transpose(0, 1)
    if p["tm"]:
        mag_dl = mag_dl.transpose(0, 1)
    k = ce_k(V, float(lse.abs().max()), float((x - lse[..., None]).abs().max()))
    return dict(loss=((lse - xt) * live, lse.double().abs() + xt.double().abs()), lse=(lse * live, lse.double().abs() + 1),
                dlogits=(dl.reshape(B * T, V), mag_dl.reshape(B * T, V)), live=live, k=k)


def ce_compare(got, ref, what):
    live = ref["live"]
    within(got["loss"], *ref["loss"], f"{what} loss_rows")
    all_zero(got["loss"][~live], f"{what} loss of inactive rows")
    if "lse" in got:
        within(got["lse"], *ref["lse"], f"{what} lse")
        all_zero(got["lse"][~live], f"{what} lse of inactive rows")
    if "dlogits" in got:
        roundings(got["dlogits"], *ref["dlogits"], ref["k"], f"{what} dlogits")
        all_zero(got["dlogits"][ref["dlogits"][0] == 0], f"{what} dlogits of inactive rows")


# ------------------------------------------------------------------------------------------ alpha regulariser, loss
ALPHA_C = 1.0
REG_CASES = [(1, 1, 1, 1), (3, 4, 29, 1), (5, 3, 196, 1), (3, 4, 29, 0)]  # (B, T, P, dreg); 5 * 196 = 3 * 256 + 212


def reg_inputs(case):
    B, T, P, _ = case
    return dict(alphas=torch.softmax(_u(gen("reg", case), (B, T, P), 2.0).double(), 2).float())


def reg_ref(p, dt=F64, bug=None):
    """d = alpha_c - sum_t alpha; reg = mean(d^2); dreg = -2 d / (B P). k for dreg: the T adds of the sum, the
    subtraction, 1 / n, and the product by it (-2 is exact): T + 3, of |alpha_c| + sum_t alpha."""
    al = p["alphas"]
    B, T, P = al.shape
    d = ALPHA_C - al.to(dt).sum(1)
    mag_d = ALPHA_C + al.double().sum(1)
    n = P if bug == "scaled_by_1_over_P" else B * P
    return dict(reg=((d * d).mean(), (mag_d * mag_d).mean()), dreg=(-2 * d / n, 2 * mag_d / (B * P)), k=T + 3)


def reg_compare(got, ref, what):
    within(got["reg"], *ref["reg"], f"{what} reg")
    if "dreg" in got:
        roundings(got["dreg"], *ref["dreg"], ref["k"], f"{what} dreg")


LOSSFIN_CASES = [(1, 0), (1023, 1), (1025, 49), (2500, 49), (2500, 0)]  # (n, nreg): 1024 threads, one row short / over


def lossfin_inputs(case):
    n, nreg = case
    g = gen("lossfin", case)
    return dict(rows=torch.rand(n, generator=g) * 8, reg=torch.rand(nreg, generator=g) if nreg else None, nrows=max(1, n - n // 7))


def lossfin_ref(p, dt=F64):
    s = p["rows"].to(dt).sum() / p["nrows"]
    mag = p["rows"].double().sum() / p["nrows"]
    if p["reg"] is not None:
        s, mag = s + p["reg"].to(dt).sum(), mag + p["reg"].double().sum()
    return dict(loss=(s, mag))


# ------------------------------------------------------------------------------------------ data movers
EMB_V, EMB_B, EMB_L, EMB_T = 11, 3, 5, 4
GATHER_CASES = [("f32", 1), ("f32", 300), ("f64", 1), ("f64", 300)]  # (table dtype, M); ld_out = M + 8, T < L


def gather_inputs(case):
    dtype, M = case
    g = gen("gather", case)
    emb = torch.rand(EMB_V, M, generator=g, dtype=F64) * 2 - 1
    return dict(emb=emb if dtype == "f64" else emb.float(), caps=torch.randint(0, EMB_V, (EMB_B, EMB_L), generator=g))


def gather_ref(p):
    """out[t][b] = emb[caps[b][t]], t < T, as fp32"""
    caps = p["caps"].to(p["emb"].device)
    return p["emb"].float()[caps[:, :EMB_T].t()]


DENSE_CASES = [(3, 5, 4, 4), (2, 6, 300, 3)]  # (B, Le, M, T); ld_out = M + 8


def dense_inputs(case):
    B, Le, M, T = case
    return dict(emb=_u(gen("dense", case), (B, Le, M)))


def dense_ref(p, T):
    return p["emb"][:, :T].transpose(0, 1).contiguous()


MASK_T, MASK_B, MASK_COLS, MASK_BT = 3, 3, 5, [3, 2, 0]


def mask_ref(x):
    """x (T, B, cols), any strides: rows b >= bt[t] zeroed"""
    out = x.clone()
    for t, n in enumerate(MASK_BT):
        out[t, n:] = 0
    return out


DROPOUT_N = 1 << 16


# ============================================================================================ part C
# ------------------------------------------------------------------------------------------ Adam
ADAM = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, clip=5.0)
ADAM_N = [1, 255, 257, 8192 * 256 + 3]  # the last: three elements take a second trip of the grid-stride loop
ADAM_CASES = [(d, n) for d in ("f32", "f64") for n in ADAM_N]
ADAM_STEPS = 3
# fp operations on the path (the reference keeps 1 - beta1, beta2, 1 - beta2, eps in double: a rounding each)
ADAM_K = dict(m=4,   # w1, g - m, w1 *, m +
              v=6,   # b2, v * b2, w2, w2 * g, * g, +
              p=14)  # v's 6 halved by the sqrt 3, sqrt 1, / bc2 1, eps and + eps 2; m's 4; m / denom, * step, p + 3


def adam_dtype(case):
    return torch.float32 if case[0] == "f32" else F64


def adam_inputs(case, device="cpu"):
    """p, m, v >= 0 and ADAM_STEPS gradients. The gradients are drawn in [-6, 6] (a sixth is clamped) and start
    with exactly +-clip, the values just inside, and 10 x clip outside (as far as n allows). |p| is drawn in
    [1/4, 1]: the update's numerator m + w1 (g - m) cancels, so its roundings are relative to |m| + w1 (|g| + |m|)
    and not to |update|; against |p| >= 1/4 they are below 0.01 ulp (step_size / denom is about 1e-3), which makes
    k ulp (|p| + |update|) a true bound for these inputs."""
    T, n = adam_dtype(case), case[1]
    g = torch.Generator().manual_seed(zlib.crc32(case_id(case).encode()))
    r = lambda: torch.rand(n, generator=g, dtype=F64)  # noqa: E731
    p = dict(p=((r() * 0.75 + 0.25) * torch.where(r() < 0.5, -1.0, 1.0)).to(T), m=((r() * 2 - 1) * 0.5).to(T),
             v=(r() * 0.25).to(T))
    clip = torch.tensor(ADAM["clip"], dtype=T)
    inside = torch.nextafter(clip, torch.zeros((), dtype=T))
    special = torch.stack([clip, -clip, inside, -inside, 10 * clip, -10 * clip])
    p["g"] = []
    for s in range(ADAM_STEPS):
        gr = ((r() * 2 - 1) * 6).to(T)
        k = min(n, 6)
        gr[:k] = special.roll(s)[:k]
        p["g"].append(gr.to(device))
    return {k: v.to(device) if torch.is_tensor(v) else v for k, v in p.items()}


def adam_bc(step, shift=0):
    """(bc1, bc2_sqrt) as the host computes them for step number ``step``"""
    t = step - shift
    return 1.0 - ADAM["beta1"] ** t, math.sqrt(1.0 - ADAM["beta2"] ** t)


def adam_ref(p, g, m, v, step, T, bug=None):
    """One step in fp64 from the state handed to the kernel, as csrc/optim.hip's header states it: clamp, lerp,
    addcmul, addcdiv with step_size = lr / bc1 and bc2_sqrt rounded to T. Returns {name: (ref, mag)}."""
    h = ADAM
    bc1, bc2s = adam_bc(step, 1 if bug == "bias_correction_of_t_minus_1" else 0)
    rnd = lambda x: float(torch.tensor(x, dtype=F64).to(T))  # noqa: E731
    step_size, bc2s = rnd(h["lr"] / bc1), rnd(bc2s)
    gd, md, vd, pd = g.double(), m.double(), v.double(), p.double()
    if bug != "no_clamp":
        gd = gd.clamp(-h["clip"], h["clip"])
    m1 = md + (1 - h["beta1"]) * (gd - md)
    v1 = vd * h["beta2"] + (1 - h["beta2"]) * gd * gd
    upd = step_size * m1 / (v1.sqrt() / bc2s + h["eps"])
    return dict(m=(m1, md.abs() + (1 - h["beta1"]) * (gd.abs() + md.abs())), v=(v1, v1), p=(pd - upd, pd.abs() + upd.abs()))


def adam_compare(got, ref, T, what):
    ulp = ULP if T == torch.float32 else 2.0 ** -53
    for k in ("m", "v", "p"):
        roundings(got[k], *ref[k], ADAM_K[k], f"{what} {k}", ulp=ulp)


# ------------------------------------------------------------------------------------------ embedding scatter-add
SC_B, SC_T, SC_L, SC_M, SC_V = 3, 4, 6, 5, 9
SC_BT = [3, 3, 2, 1]
# (destination dtype, captions, ragged bt): "mixed": token 1 once, token 2 twice, token 3 in every other active
# slot; "same": token 4 in all B T slots. ld_dx = M + 4, T < L.
SCATTER_CASES = [("f32", "mixed", 1), ("f32", "same", 0), ("f64", "mixed", 1), ("f64", "same", 0), ("f32", "same", 1)]


def scatter_inputs(case):
    dtype, kind, bt = case
    g = gen("scatter", case)
    caps = torch.full((SC_B, SC_L), 4 if kind == "same" else 3, dtype=torch.int64)
    if kind == "mixed":
        caps[0, 0], caps[1, 0], caps[0, 1] = 1, 2, 2
    caps[:, SC_T:] = 7  # past T: never read
    T = torch.float32 if dtype == "f32" else F64
    return dict(dx=padded(_u(g, (SC_T * SC_B, SC_M)), SC_M + 4).unflatten(0, (SC_T, SC_B)), caps=caps,
                bt=torch.tensor(SC_BT, dtype=torch.int32) if bt else None,
                demb=(torch.rand(SC_V, SC_M, generator=g, dtype=F64) * 2 - 1).to(T))


def scatter_ref(p, dt=F64, bug=None):
    """demb[caps[b][t]] += dx[t][b] over the active (t, b); returns (ref, mag, multiplicity per row)"""
    dev = p["dx"].device
    demb = p["demb"].to(dt).clone()
    mag, mult = p["demb"].double().abs().clone(), torch.zeros(SC_V, dtype=torch.int64, device=dev)
    for t in range(SC_T):
        for b in range(SC_B if p["bt"] is None else int(p["bt"][t])):
            tok = int(p["caps"][b, t])
            d = p["dx"][t, b]
            demb[tok] = d.to(dt) if bug == "overwrite" else demb[tok] + d.to(dt)
            mag[tok] += d.double().abs()
            mult[tok] += 1
    return demb, mag, mult


def scatter_compare(got, ref, init, what):
    want, mag, mult = ref
    for tok in range(SC_V):
        k = int(mult[tok])
        if k == 0:
            exact(got[tok], init[tok].to(got.device), f"{what} untouched row {tok}")
        else:  # k atomic adds in any order
            roundings(got[tok], want[tok], mag[tok], k, f"{what} x{k}", ulp=ULP if got.dtype == torch.float32 else 2.0 ** -53)
