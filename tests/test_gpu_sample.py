"""GPU: sampled decoding (capmi.sample; csrc/sample.hip) -- capmi_sample_step against the fp64 contract of
tests/sample_cases.py::pick_ref (random rows, edge rows, bookkeeping, the drawn distribution), whole rollouts of
both decoders by forced replay on the CPU, the greedy rollout against beam search with one beam, and the public
surface.

Bounds. A token is compared exactly where pick_ref's margin (the distance of u from the neighbouring CDF steps)
is at least 1e-5: a sequential fp32 CDF deviates from fp64 by at most 3.7e-7 on the random cases, so 1e-5 is
about 30 times that. logp at temperature 1 (and for the greedy pick) takes the bound of
test_gpu_beam_batched.py::test_beam_select_matches_fp64, assert_close(1e-6, 1e-6). At any other temperature the
only extra rounding is the division, so the bound is 4 times the largest error of the fp32 restatement on the
CPU (sample_cases.logp_fp32, a sequential sum) against fp64 on the same inputs, taken over every row of the
same (V, temperature, top_k) -- all three R of the kernel cases, every draw of a rollout. Measured on the kernel
cases: the restatement errs by 2.3e-7 (V = 37, temperature 0.7) to 7.6e-7 (V = 1000, temperature 0.7), so the
bounds lie between 9.2e-7 and 3.0e-6; |logp| there is up to about 12, where one fp32 ulp is 9.5e-7.

Rollouts. The toy decoders give END about the probability of any other word, so with no END bias one to five of
the twelve rows of a run draw END within 13 steps at temperature 1 on every table of uniforms tried. The run in
which nothing may finish therefore lowers END's bias by 30 (weight e^-30) instead of leaving it at 0; the run
in which rows finish early raises it by 3."""
import functools
import types

import pytest
import torch
import torch.nn.functional as F

import baseline_cases as BLC
import beam_cases as BC
import gen
import sample_cases as SC
from helpers import assert_close, t

pytestmark = pytest.mark.gpu
DEV = "cuda"
I32 = dict(dtype=torch.int32, device=DEV)
MARGIN = 1e-5
LOGIT_RTOL, LOGIT_ATOL = 1e-4, 1e-5  # tests/test_gpu_decoder.py, decoder logits
ALPHA_ATOL = 1e-5                    # tests/test_gpu_beam_batched.py, alphas
CANARY = -7


def _step(logits, u, temperature, top_k, end_idx, alive=None, step=0):
    """One capmi_sample_step launch. Returns (tokens, logp, prev, alive, rows_live) on the host; rows that the
    kernel does not write keep CANARY in tokens / logp / prev."""
    from capmi import kernels as K
    R, V = logits.shape
    alive = torch.ones(R, **I32) if alive is None else torch.tensor(alive, **I32)
    rows_live = torch.tensor([int(alive.sum())], **I32)
    tokens = torch.full((R,), CANARY, **I32)
    logp = torch.full((R,), float(CANARY), device=DEV)
    prev = torch.full((R,), CANARY, dtype=torch.int64, device=DEV)
    K.sample_step(logits.to(DEV).contiguous(), R, V, u.to(DEV), temperature, top_k, end_idx, step, alive, prev, tokens,
                  logp, rows_live)
    torch.cuda.synchronize()
    return tokens.cpu(), logp.cpu(), prev.cpu(), alive.cpu(), int(rows_live.item())


def _refs(logits, u, temperature, top_k):
    return [SC.pick_ref(logits[r], float(u[r]), temperature, top_k) for r in range(logits.size(0))]


# ---------------------------------------------------------------------------------------------
# 1. the kernel against fp64 on random rows
# ---------------------------------------------------------------------------------------------
VS, RS = (37, 1000, 8100), (1, 5, 96)
SETTINGS = ((1.0, 0), (0.7, 0), (1.0, 10), (1.3, 64))


@functools.lru_cache(maxsize=None)
def _inputs(V, R):
    g = torch.Generator().manual_seed(9100 + V + R)
    logits = 3.0 * torch.randn(R, V, generator=g)
    return logits, torch.rand(R, generator=g)


@functools.lru_cache(maxsize=None)
def _case_refs(V, R, temperature, top_k):
    logits, u = _inputs(V, R)
    return _refs(logits, u, temperature, top_k)


@functools.lru_cache(maxsize=None)
def _restatement_error(V, temperature, top_k):
    """max |fp32 restatement - fp64| of logp over every row of the three R cases of this (V, setting)"""
    worst = 0.0
    for R in RS:
        logits, _ = _inputs(V, R)
        for r, (tok, lp, _) in enumerate(_case_refs(V, R, temperature, top_k)):
            worst = max(worst, abs(SC.logp_fp32(logits[r], tok, temperature, top_k) - lp))
    return worst


def _assert_logp(got, want, temperature, restatement_error, what):
    got, want = torch.tensor(got, dtype=torch.float64), torch.tensor(want, dtype=torch.float64)
    if not got.numel():
        return
    err = float((got - want).abs().max())
    if temperature in (0.0, 1.0):
        print(f"{what}: max |logp - fp64| {err:.3g} (bound 1e-6 + 1e-6 |logp|)")
        assert_close(got, want, 1e-6, 1e-6, what)
    else:
        print(f"{what}: max |logp - fp64| {err:.3g}; fp32 restatement {restatement_error:.3g}, bound 4x")
        assert err <= 4 * restatement_error, (what, err, restatement_error)


@pytest.mark.parametrize("temperature,top_k", SETTINGS)
@pytest.mark.parametrize("R", RS)
@pytest.mark.parametrize("V", VS)
def test_sample_step_matches_fp64(V, R, temperature, top_k):
    logits, u = _inputs(V, R)
    ref = _case_refs(V, R, temperature, top_k)
    clear = [r for r in range(R) if ref[r][2] >= MARGIN]
    # the test's own precondition: no row skipped for R <= 5, at most 5 of 96
    assert len(clear) == R if R <= 5 else R - len(clear) <= 5, [ref[r][2] for r in range(R)]
    tokens, logp, prev, alive, rows_live = _step(logits, u, temperature, top_k, V - 1)
    assert ((tokens >= 0) & (tokens < V)).all()
    assert tokens[clear].tolist() == [ref[r][0] for r in clear]
    agree = [r for r in range(R) if int(tokens[r]) == ref[r][0]]
    print(f"V {V} R {R} T {temperature} top_k {top_k}: {R - len(clear)} rows under the margin, "
          f"{len(agree)} of {R} tokens agree")
    _assert_logp(logp[agree].tolist(), [ref[r][1] for r in agree], temperature,
                 _restatement_error(V, temperature, top_k), "kernel logp")
    assert prev.tolist() == tokens.tolist()
    ended = tokens == V - 1
    assert alive.tolist() == (~ended).int().tolist() and rows_live == R - int(ended.sum())


def test_sample_step_long_rows_are_read_through_l2():
    """V above what a workgroup keeps in LDS (14336): the same code on the global row."""
    V, R = 20000, 3
    g = torch.Generator().manual_seed(9203)  # chosen on the CPU: margins of 9.9e-4 and 1.2e-3
    logits, u = 3.0 * torch.randn(R, V, generator=g), torch.rand(R, generator=g)
    for temperature, top_k in ((1.0, 0), (1.0, 64), (0.0, 0)):
        ref = _refs(logits, u, temperature, top_k)
        assert min(x[2] for x in ref) >= MARGIN
        tokens, logp, _, _, _ = _step(logits, u, temperature, top_k, V - 1)
        assert tokens.tolist() == [x[0] for x in ref]
        err = max(abs(SC.logp_fp32(logits[r], ref[r][0], temperature or 1.0, top_k) - ref[r][1]) for r in range(R))
        _assert_logp(logp.tolist(), [x[1] for x in ref], temperature, err, "long rows")


# ---------------------------------------------------------------------------------------------
# 2. edges
# ---------------------------------------------------------------------------------------------
NINF = float("-inf")
U_TOP = 1.0 - 2.0 ** -24


def _rand_logits(V, R, seed):
    return 3.0 * torch.randn(R, V, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("V", [50, 8100])
def test_u_at_both_ends(V):
    logits = _rand_logits(V, 6, 500 + V)
    logits[0::2, :3] = NINF          # the first entry with weight is not entry 0
    logits[1::2, V - 4:] = NINF      # the last entry with weight is not entry V-1
    for temperature, top_k in ((1.0, 0), (0.7, 0), (1.0, 10), (1.3, V - 1)):
        keep = [SC.kept_mask(logits[r], top_k) & (logits[r] > NINF) for r in range(6)]
        tokens, logp, _, _, _ = _step(logits, torch.zeros(6), temperature, top_k, -1)
        # u = 0: exactly the first kept entry with weight
        assert tokens.tolist() == [int(k.nonzero()[0]) for k in keep]
        assert tokens.tolist() == [x[0] for x in _refs(logits, torch.zeros(6), temperature, top_k)]
        assert torch.isfinite(logp).all()
        tokens, logp, _, _, _ = _step(logits, torch.full((6,), U_TOP), temperature, top_k, -1)
        for r in range(6):  # a kept index with positive weight, never outside the row
            assert 0 <= int(tokens[r]) < V and bool(keep[r][int(tokens[r])]), (r, int(tokens[r]))
        assert torch.isfinite(logp).all()


@pytest.mark.parametrize("V", [50, 8100])
def test_single_finite_logit_and_inf_neighbours(V):
    us = torch.tensor([0.0, 0.5, U_TOP, 0.0, 0.5, U_TOP])
    logits = torch.full((6, V), NINF)
    logits[:3, 0] = 1.5
    logits[3:, V - 1] = -2.5
    for temperature, top_k in ((1.0, 0), (0.7, 5), (0.0, 0)):
        tokens, logp, _, _, _ = _step(logits, us, temperature, top_k, -1)
        assert tokens.tolist() == [0, 0, 0, V - 1, V - 1, V - 1] and logp.tolist() == [0.0] * 6
    # -inf on both sides of a dominant argmax
    logits = _rand_logits(V, 4, 600 + V)
    for r, a in enumerate((1, V // 2, V - 2, 17)):
        logits[r, a] = 20.0
        logits[r, a - 1] = logits[r, a + 1] = NINF
    u = torch.full((4,), 0.5)
    for temperature, top_k in ((1.0, 0), (1.0, 3), (0.0, 0)):
        ref = _refs(logits, u, temperature, top_k)
        tokens, logp, _, _, _ = _step(logits, u, temperature, top_k, -1)
        assert tokens.tolist() == [1, V // 2, V - 2, 17] == [x[0] for x in ref]
        assert_close(logp, torch.tensor([x[1] for x in ref]), 1e-6, 1e-6, "logp beside -inf")


@pytest.mark.parametrize("V", [50, 8100])
def test_top_k_limits(V):
    R = 8
    logits = _rand_logits(V, R, 700 + V)
    u = torch.rand(R, generator=torch.Generator().manual_seed(701))
    u[0], u[1] = 0.0, U_TOP
    # top_k = 1 is the argmax for any u, with probability 1
    tokens, logp, _, _, _ = _step(logits, u, 0.9, 1, -1)
    assert tokens.tolist() == logits.argmax(1).tolist() and logp.tolist() == [0.0] * R
    # top_k >= V is top_k = 0, bit for bit
    base = _step(logits, u, 0.8, 0, -1)
    for top_k in (V, V + 5, 2 ** 31 - 1):
        got = _step(logits, u, 0.8, top_k, -1)
        assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1])


@pytest.mark.parametrize("V", [50, 8100])
def test_ties_across_the_top_k_threshold_keep_the_lower_index(V):
    """Column `hi` holds the largest value, columns a < b < c the same second value. top_k = 2 keeps {hi, a},
    top_k = 3 {hi, a, b}; u is chosen so that any other reading of the tie draws another token."""
    a, b, c, hi = 3, V // 2, V - 2, V // 3
    row = torch.full((V,), -2.0)
    row[[a, b, c]] = 5.0
    row[hi] = 6.0
    logits = row.repeat(4, 1)
    # weights 1 (hi) and e^-1 = 0.3679 each: top_k 2 -> cdf over {a, hi} = 0.269, 1; top_k 3 -> over {a, hi, b}
    # = 0.212, 0.788, 1. Wrong kept sets: {hi, b} / {hi, c} never give a; {a, hi, c} never gives b.
    u = torch.tensor([0.1, 0.9, 0.1, 0.9])
    tokens, logp, _, _, _ = _step(logits[:2], u[:2], 1.0, 2, -1)
    assert tokens.tolist() == [a, hi] == [x[0] for x in _refs(logits[:2], u[:2], 1.0, 2)]
    tokens3, logp3, _, _, _ = _step(logits[2:], u[2:], 1.0, 3, -1)
    ref3 = _refs(logits[2:], u[2:], 1.0, 3)
    assert tokens3.tolist() == [a, b] == [x[0] for x in ref3]
    assert_close(logp3, torch.tensor([x[1] for x in ref3]), 1e-6, 1e-6, "logp with ties")
    # -0.0 and 0.0 are one value: the tie still goes by index
    z = torch.full((2, V), -3.0)
    z[:, a], z[:, b], z[:, hi] = 0.0, -0.0, 1.0
    z[1, a], z[1, b] = -0.0, 0.0
    tz, _, _, _, _ = _step(z, torch.tensor([0.05, 0.05]), 1.0, 2, -1)
    assert tz.tolist() == [a, a]


@pytest.mark.parametrize("V", [50, 8100])
def test_greedy_and_cold_temperature(V):
    logits = _rand_logits(V, 3, 800 + V)
    logits[0, 7] = logits[0, V - 9] = 15.0   # an exact tie at the maximum
    logits[1, V - 1] = logits[1, 0] = 15.0
    u = torch.tensor([0.99, 0.5, 0.0])
    tokens, logp, _, _, _ = _step(logits, u, 0.0, 3, -1)
    assert tokens.tolist() == [7, 0, int(logits[2].argmax())]
    want = F.log_softmax(logits.double(), 1)[torch.arange(3), tokens.long()]
    assert_close(logp, want, 0.0, 1e-6, "greedy logp")
    # temperature 0.05 over logits spanning +-30: every other weight underflows or is tiny
    cold = 60.0 * torch.rand(2, V, generator=torch.Generator().manual_seed(801)) - 31.0
    cold[0, V // 2], cold[1, 1] = 30.0, 30.0
    cold[0, 0], cold[1, V - 1] = -30.0, -30.0
    tokens, logp, _, _, _ = _step(cold, torch.tensor([0.5, 0.5]), 0.05, 0, -1)
    assert tokens.tolist() == [V // 2, 1] and torch.isfinite(logp).all() and (logp <= 0).all()
    assert_close(logp, torch.tensor([x[1] for x in _refs(cold, torch.tensor([0.5, 0.5]), 0.05, 0)]), 0.0, 1e-6,
                 "cold logp")


# ---------------------------------------------------------------------------------------------
# 3. bookkeeping
# ---------------------------------------------------------------------------------------------
def test_dead_rows_are_not_touched_and_end_is_recorded():
    V, END = 50, 48
    logits = _rand_logits(V, 5, 900)
    logits[:, END] = -20.0
    logits[2, END] = 20.0  # row 2 must draw END
    tokens, logp, prev, alive, rows_live = _step(logits, torch.full((5,), 0.3), 1.0, 1, END, alive=[1, 0, 1, 0, 1],
                                                 step=4)
    assert tokens.tolist() == [int(logits[0].argmax()), CANARY, END, CANARY, int(logits[4].argmax())]
    assert logp.tolist() == [0.0, float(CANARY), 0.0, float(CANARY), 0.0]
    assert prev.tolist() == tokens.tolist()
    assert alive.tolist() == [1, 0, 0, 0, 1]
    assert rows_live == 3 - 1


# ---------------------------------------------------------------------------------------------
# 4. the drawn distribution
# ---------------------------------------------------------------------------------------------
CHI2_999 = {2: 13.816, 6: 22.458}  # 0.999 quantiles of chi-square


@pytest.mark.parametrize("temperature,top_k", [(1.0, 0), (0.5, 0), (1.0, 3)])
def test_counts_follow_the_distribution(temperature, top_k):
    R, row = 20000, torch.tensor([0.5, -1.0, 2.0, 0.0, 1.5, -0.3, 1.0])
    u = torch.rand(R, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1234))
    tokens, _, _, _, _ = _step(row.repeat(R, 1), u, temperature, top_k, -1)
    keep = SC.kept_mask(row, top_k)
    w = torch.where(keep, torch.exp(row.double() / temperature), torch.zeros(7, dtype=torch.float64))
    expected = R * w / w.sum()
    counts = torch.bincount(tokens.long(), minlength=7).double()
    assert (counts[~keep] == 0).all() and float(expected[keep].min()) >= 5
    chi2 = float(((counts - expected) ** 2 / expected)[keep].sum())
    dof = int(keep.sum()) - 1
    print(f"T {temperature} top_k {top_k}: chi-square {chi2:.3f} on {dof} degrees of freedom "
          f"(0.999 quantile {CHI2_999[dof]}); counts {counts.tolist()}")
    assert chi2 < CHI2_999[dof]


# ---------------------------------------------------------------------------------------------
# 5. / 6. rollouts by forced replay
# ---------------------------------------------------------------------------------------------
ROLL_SETTINGS = ((1.0, 0), (0.8, 5), (0.0, 0))
B_ROLL, N_ROLL, MAX_STEPS = 3, 4, 12


def _check_rollout(out, sampler, u, temperature, top_k, start, end, replay, what):
    """(a) - (d) of a rollout. ``replay(i, tokens)`` -> CPU logits (len(tokens), V) along the row's own prefix."""
    T, n = MAX_STEPS + 1, N_ROLL
    kept = sampler.last_logits.cpu()
    assert kept.shape[:2] == (T, B_ROLL * n)
    draws = skipped = 0
    got_lp, want_lp, restated = [], [], 0.0
    for i in range(B_ROLL):
        for j in range(n):
            d, r = out[i][j], i * n + j
            toks = d["seq"][1:] if d["finished"] else d["seq"]
            assert not d["finished"] or d["seq"][0] == start
            # (d) a sequence stops at its first END, or runs all max_steps + 1 draws
            assert end not in toks[:-1] and d["finished"] == (toks[-1] == end)
            assert d["finished"] or len(toks) == T
            # (c)
            assert len(d["token_logp"]) == len(toks)
            assert abs(d["logp"] - sum(d["token_logp"])) <= 1e-6 * max(1.0, abs(d["logp"]))
            # (a) the logits of every step the row was alive at, along its own prefix
            assert_close(kept[:len(toks), r], replay(i, toks), LOGIT_RTOL, LOGIT_ATOL, f"{what} row {r} logits")
            # (b) every draw against the contract on the GPU's own logits
            for t_, tok in enumerate(toks):
                want, lp, margin = SC.pick_ref(kept[t_, r], float(u[t_, r]), temperature, top_k)
                draws += 1
                if margin < MARGIN:
                    skipped += 1
                    continue
                assert tok == want, (what, r, t_, tok, want, margin)
                got_lp.append(d["token_logp"][t_])
                want_lp.append(lp)
                if temperature not in (0.0, 1.0):
                    restated = max(restated, abs(SC.logp_fp32(kept[t_, r], want, temperature, top_k) - lp))
    assert skipped <= 0.05 * draws, (skipped, draws)
    _assert_logp(got_lp, want_lp, temperature, restated, f"{what} token_logp")
    print(f"{what}: {draws} draws, {skipped} under the margin, lengths "
          f"{[len(d['token_logp']) for per in out for d in per]}")


@pytest.mark.parametrize("temperature,top_k", ROLL_SETTINGS)
@pytest.mark.parametrize("end_bias", [3.0, -30.0])
@pytest.mark.parametrize("A,D,M,V", [(32, 32, 16, 50), (64, 32, 16, 120)])
def test_attention_rollouts_by_forced_replay(A, D, M, V, end_bias, temperature, top_k):
    from capmi.sample import BatchedSampler
    start, end = V - 3, V - 2
    dec, p = BC.tuned_decoder(A, D, M, V, 62, 2.0, end_bias, end, DEV)
    feats = BC.features((62, 162, 262))
    u = torch.rand(MAX_STEPS + 1, B_ROLL * N_ROLL, generator=torch.Generator().manual_seed(4000 + V))
    s = BatchedSampler(dec, N_ROLL, temperature, top_k)
    out = s.sample(feats.to(DEV), start, end, max_steps=MAX_STEPS, uniforms=u, return_alphas=True, keep_logits=True)
    assert len(out) == B_ROLL and all(len(per) == N_ROLL for per in out)
    replays = {}

    def replay(i, toks):
        replays[(i, tuple(toks))] = SC.attention_replay(p, feats[i:i + 1], start, toks)
        return replays[(i, tuple(toks))][0]

    what = f"attention V {V} end_bias {end_bias} T {temperature} top_k {top_k}"
    _check_rollout(out, s, u, temperature, top_k, start, end, replay, what)
    done = [d["finished"] for per in out for d in per]
    if end_bias > 0:  # what the two runs are there for
        assert sum(done) > len(done) // 2
    else:
        assert not any(done) and all(len(d["seq"]) == MAX_STEPS + 1 for per in out for d in per)
    # (e) alphas: a row of ones, then the attention of every step of the row
    for i in range(B_ROLL):
        for d in out[i]:
            toks = d["seq"][1:] if d["finished"] else d["seq"]
            al = torch.tensor(d["alphas"])
            assert al.shape == (len(toks) + 1, 14, 14) and bool((al[0] == 1).all())
            assert_close(al[1:].reshape(len(toks), -1), replays[(i, tuple(toks))][1], 0.0, ALPHA_ATOL, what + " alphas")
    plain = s.sample(feats.to(DEV), start, end, max_steps=MAX_STEPS, uniforms=u)
    assert [[d["seq"] for d in per] for per in plain] == [[d["seq"] for d in per] for per in out]
    assert all(d["alphas"] == [] for per in plain for d in per) and s.last_logits is None


BL_M, BL_H, BL_V = 16, 24, 50


@pytest.mark.parametrize("temperature,top_k", ROLL_SETTINGS)
@pytest.mark.parametrize("end_bias", [3.0, -30.0])
def test_baseline_rollouts_by_forced_replay(end_bias, temperature, top_k):
    from capmi.sample import BaselineBatchedSampler
    start, end = BL_V - 3, BL_V - 2
    dec, p = BLC.decoder(BL_M, BL_H, BL_V, 48, DEV, fc_scale=20.0, end_bias=end_bias, end_idx=end)
    feats = torch.stack([t(gen.uniform(48 + i, "feats", (BL_M,), -1, 1)) for i in range(B_ROLL)])
    u = torch.rand(MAX_STEPS + 1, B_ROLL * N_ROLL, generator=torch.Generator().manual_seed(4100))
    s = BaselineBatchedSampler(dec, N_ROLL, temperature, top_k)
    out = s.sample(feats.to(DEV), start, end, max_steps=MAX_STEPS, uniforms=u, keep_logits=True)
    what = f"baseline end_bias {end_bias} T {temperature} top_k {top_k}"
    _check_rollout(out, s, u, temperature, top_k, start, end,
                   lambda i, toks: SC.baseline_replay(p, feats[i], start, toks), what)
    done = [d["finished"] for per in out for d in per]
    if end_bias > 0:
        assert sum(done) > len(done) // 2
    else:
        assert not any(done) and all(len(d["seq"]) == MAX_STEPS + 1 for per in out for d in per)
    assert all(d["alphas"] == [] for per in out for d in per)


# ---------------------------------------------------------------------------------------------
# 7. the greedy rollout is beam search with one beam
# ---------------------------------------------------------------------------------------------
def _same_as_one_beam(out, beams):
    finished = 0
    for per, (seq, _, ok, (_, scores)) in zip(out, beams):
        if not ok:
            continue
        finished += 1
        assert per[0]["finished"] and per[0]["seq"] == seq
        assert abs(per[0]["logp"] - scores[0]) <= 1e-5, (per[0]["logp"], scores[0])
    assert finished >= 2  # the comparison is not empty


def test_greedy_rollout_equals_beam_search_with_one_beam():
    from capmi.beam import BaselineBatchedBeamSearch, BatchedBeamSearch
    from capmi.sample import BaselineBatchedSampler, BatchedSampler
    V = 120
    dec, _ = BC.tuned_decoder(64, 48, 32, V, 62, 1.0, 2.0, V - 2, DEV)
    feats = BC.features((62, 162, 262, 362)).to(DEV)
    beams = BatchedBeamSearch(dec, 1).search(feats, V - 3, V - 2, max_steps=20, return_all=True, return_alphas=False)
    _same_as_one_beam(BatchedSampler(dec, 1, 0.0).sample(feats, V - 3, V - 2, max_steps=20), beams)
    bdec, _ = BLC.decoder(BL_M, BL_H, BL_V, 48, DEV, fc_scale=60.0, end_bias=2.0, end_idx=BL_V - 2)
    bfeats = torch.stack([t(gen.uniform(48 + i, "feats", (BL_M,), -1, 1)) for i in range(4)]).to(DEV)
    beams = BaselineBatchedBeamSearch(bdec, 1).search(bfeats, BL_V - 3, BL_V - 2, max_steps=20, return_all=True)
    _same_as_one_beam(BaselineBatchedSampler(bdec, 1, 0.0).sample(bfeats, BL_V - 3, BL_V - 2, max_steps=20), beams)


# ---------------------------------------------------------------------------------------------
# 8. surface
# ---------------------------------------------------------------------------------------------
def _strip(out):
    return [[(d["seq"], d["finished"]) for d in per] for per in out]


def test_surface_seed_batch_independence_and_syncs():
    from capmi.sample import BaselineBatchedSampler, BatchedSampler
    from gen_captions import baseline_caption_images_sample, caption_images_sample
    from vocabulary import synthetic_vocab
    V = 50
    args = types.SimpleNamespace(num_samples=3, temperature=0.9, top_k=8, seed=5)
    dec, _ = BC.tuned_decoder(32, 32, 16, V, 62, 2.0, 2.0, V - 2, DEV)
    feats = BC.features((62, 162, 262)).to(DEV)
    bdec, _ = BLC.decoder(BL_M, BL_H, BL_V, 48, DEV, fc_scale=20.0, end_bias=2.0, end_idx=BL_V - 2)
    bfeats = torch.stack([t(gen.uniform(48 + i, "feats", (BL_M,), -1, 1)) for i in range(3)]).to(DEV)
    cases = ((caption_images_sample, BatchedSampler, dec, feats), (baseline_caption_images_sample,
                                                                   BaselineBatchedSampler, bdec, bfeats))
    for fn, cls, d, x in cases:
        one = fn(DEV, args, x, lambda imgs: imgs, d, synthetic_vocab(V))
        two = fn(DEV, args, x, lambda imgs: imgs, d, synthetic_vocab(V))
        assert one == two  # the same seed: the same captions and log-probabilities
        assert len(one) == 3 and all(len(per) == 3 for per in one)
        assert all(set(s) == {"seq", "token_logp", "logp", "finished", "alphas"} for per in one for s in per)
        other = fn(DEV, types.SimpleNamespace(num_samples=3, temperature=0.9, top_k=8, seed=6), x, lambda imgs: imgs,
                   d, synthetic_vocab(V))
        assert _strip(other) != _strip(one)
        default = fn(DEV, types.SimpleNamespace(), x, lambda imgs: imgs, d, synthetic_vocab(V))
        assert [len(per) for per in default] == [1, 1, 1]
        # sample j of image i depends on its own features and its own column of uniforms alone
        n, T = 3, 21
        u = torch.rand(T, 3 * n, generator=torch.Generator().manual_seed(4200))
        s = cls(d, n, 0.9, 8)
        full = s.sample(x, V - 3, V - 2, max_steps=T - 1, uniforms=u, sync_every=4)
        st = s.last_stats
        assert 1 <= st["steps"] <= T and st["host_syncs"] <= st["steps"] // 4 + 1
        for i in range(3):
            alone = s.sample(x[i:i + 1], V - 3, V - 2, max_steps=T - 1, uniforms=u[:, i * n:(i + 1) * n])
            assert _strip(alone) == _strip(full[i:i + 1])
            for a, b in zip(alone[0], full[i]):
                assert_close(torch.tensor(a["token_logp"]), torch.tensor(b["token_logp"]), 0.0, 1e-5, "logp alone")


def test_limits():
    from capmi.sample import BatchedSampler
    dec, _ = BC.tuned_decoder(32, 32, 16, 50, 62, 1.0, 0.0, 48, DEV)
    feats = BC.features((62,)).to(DEV)
    with pytest.raises(ValueError):  # the uniforms table must be (max_steps + 1, R)
        BatchedSampler(dec, 2).sample(feats, 47, 48, max_steps=5, uniforms=torch.rand(5, 2))
    with pytest.raises(ValueError):  # keep_logits above 256 MB
        BatchedSampler(dec, 16).sample(feats.expand(8, -1, -1, -1), 47, 48, max_steps=12000, keep_logits=True)
    dec.use_bert = True
    with pytest.raises(NotImplementedError):
        BatchedSampler(dec, 2).sample(feats, 47, 48)
