"""CPU: the host side of self-critical training (capmi.scst): the fp64 reward against the reference scorer's
fixture, the device tables' contents on a hand case, argument checks of the four C entries before any launch, the
exports, and train.py's flags."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import scst_cases as SC

EINVAL, ERANGE = 1001, 1003
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("capmi_rollout_pack", "capmi_cider_reward", "capmi_scst_advantage", "capmi_pg_ce_fwd_bwd")


@pytest.fixture(scope="module")
def fixture():
    return SC.load_fixture()


@pytest.mark.parametrize("case", ["corpus", "single_image"])
@pytest.mark.parametrize("with_end", [False, True])
def test_host_reward_matches_the_reference_scorer(fixture, case, with_end):
    """Both sides evaluate the same formulas in fp64 and differ by summation order only: 1e-9 relative
    (tests/test_scoring_cpu.py's rule); a golden 0 is exactly 0."""
    from capmi.scst import CiderRefs, cider_rewards_host
    c, end = fixture[case], fixture["end_idx"]
    rows = SC.case_rows(c)
    refs = CiderRefs.build(SC.references(c), end_idx=end if with_end else None)
    got = cider_rewards_host(refs, [SC.emitted(r, end) for r in rows], [r["image"] for r in rows],
                             score_end=with_end, end_idx=end)
    assert len(got) == len(rows)
    for g, r in zip(got, rows):
        want = r["score_end" if with_end else "score"]
        assert isinstance(g, float) and abs(g - want) <= 1e-9 * abs(want), (r["image"], r["j"], g, want)


def test_fixture_covers_the_edge_cases(fixture):
    c, end = fixture["corpus"], fixture["end_idx"]
    rows = SC.case_rows(c)
    n_images = len(c["images"])
    assert 35 <= n_images <= 45 and len(fixture["single_image"]["images"]) == 1
    nrefs = [len(im["references"]) for im in c["images"]]
    assert min(nrefs) == 1 and max(nrefs) == 7
    assert any(len({tuple(r) for r in im["references"]}) < len(im["references"]) for im in c["images"])  # repeated
    lens = {len(r["hyp"]) for r in rows}
    assert {0, 1, 2, 3, 64} <= lens
    assert any(len(r["hyp"]) == 64 and not r["finished"] for r in rows)
    assert any(r["hyp"] in c["images"][r["image"]]["references"] and r["j"] < 3 for r in rows)  # an exact copy
    words = {w for im in c["images"] for r in im["references"] for w in r}
    assert {0, 65533} <= words and end not in words
    assert any(r["hyp"] and not set(r["hyp"]) & words for r in rows)  # n-grams found in no reference: df 0
    assert any(r["hyp"] and r["score"] == 0 and set(r["hyp"]) <= words for r in rows)  # no overlap with its image
    assert all(im["references"][k][0] == 1 or im["references"][k][0] == 0 for im in c["images"]
               for k in range(len(im["references"])))
    assert all(any(1 in r for r in im["references"]) for im in c["images"])  # a word of every image: idf 0
    assert any(max(np.bincount(r["hyp"]).tolist() or [0]) > 2 for r in rows if max(r["hyp"] or [0]) < 100)  # tf > 1
    assert any(r["score"] == 0 for r in rows) and any(r["score"] > 9 for r in rows)


def test_tables_on_a_hand_case():
    """Three images; df counts images, not references; idf = log(3) - log(df) computed in fp64, rounded once."""
    from capmi.scst import CiderRefs, key_order
    refs = CiderRefs.build([[[5, 6, 5], [5, 6]], [[5, 7]], [[8]]])
    key = {k: i for i, k in enumerate(refs.host["idf_keys"].tolist())}
    df = lambda *g: int(refs.df[key[SC.key_of(g)]])  # noqa: E731
    assert (df(5), df(6), df(7), df(8), df(5, 6), df(6, 5), df(5, 6, 5), df(5, 7)) == (2, 1, 1, 1, 1, 1, 1, 1)
    assert refs.n_keys == 8 and refs.n_images == 3 and refs.n_refs == 4 and refs.log_images == math.log(3.0)
    assert SC.key_of((5, 9)) not in key  # absent: df 0
    idf = refs.host["idf_vals"]
    assert idf.dtype == np.float32
    assert idf[key[SC.key_of((5,))]] == np.float32(math.log(3.0) - math.log(2.0))
    assert idf[key[SC.key_of((6,))]] == np.float32(math.log(3.0))
    ascending = lambda k: all(a < b for a, b in zip(k.tolist(), k.tolist()[1:]))  # noqa: E731
    assert ascending(refs.host["idf_keys"])
    assert key_order([SC.key_of((5,)), SC.key_of((5, 6)), SC.key_of((5, 6, 5)), SC.key_of((0, 0, 0, 0))]).tolist() \
        == [1, 2, 3, 4]
    h = refs.host
    assert h["img_off"].tolist() == [0, 2, 3, 4] and h["ref_bigrams"].tolist() == [2, 1, 1, 0]
    assert h["ref_off"].tolist() == [0, 5, 8, 11, 12]  # [5 6 5]: 5, 6, 56, 65, 565
    w_of = dict(zip(h["ref_keys"][:5].tolist(), h["ref_w"][:5]))
    assert w_of[SC.key_of((5,))] == np.float32(2) * idf[key[SC.key_of((5,))]]  # tf 2, one fp32 product
    assert all(ascending(h["ref_keys"][a:b]) for a, b in zip(h["ref_off"][:-1], h["ref_off"][1:]))
    w5, w6 = 2 * (math.log(3.0) - math.log(2.0)), math.log(3.0)
    assert abs(float(h["ref_norm"][0, 0]) - math.hypot(w5, w6)) < 1e-6
    assert h["ref_norm"][3].tolist()[1:] == [0.0, 0.0, 0.0]  # one word: no bigram
    assert refs.nbytes == sum(a.nbytes for a in h.values())
    single = CiderRefs.build([[[5, 6]]])
    assert single.log_images == 1.0 and single.host["idf_vals"].tolist() == [1.0, 1.0, 1.0]  # the scorers' quirk
    with_end = CiderRefs.build([[[5, 6]]], end_idx=2)
    assert with_end.references == [[[5, 6, 2]]] and with_end.host["ref_bigrams"].tolist() == [2]


def test_build_rejects_what_the_keys_cannot_hold():
    from capmi.scst import CiderRefs
    CiderRefs.build([[[1] * 63]], end_idx=2)
    CiderRefs.build([[[65533, 0]]])
    with pytest.raises(ValueError, match="63"):
        CiderRefs.build([[[1] * 64]])
    with pytest.raises(ValueError, match="65533"):
        CiderRefs.build([[[3, 65534]]])
    with pytest.raises(ValueError):
        CiderRefs.build([[[3, -1]]])
    with pytest.raises(ValueError):
        CiderRefs.build([[[3]], []])  # an image without a reference
    with pytest.raises(ValueError):
        CiderRefs.build([])


def test_new_entry_points_are_declared_exported_and_bound():
    import capmi
    from capmi import kernels as K
    with open(os.path.join(REPO, "include", "capmi.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for name in NEW:
        assert re.search(r"^int " + name + r"\(", text, flags=re.M), name
        assert hasattr(ctypes.CDLL(capmi.LIB_PATH), name)
        assert callable(getattr(K, name[len("capmi_"):])), name
    assert set(NEW) <= set(capmi.EXPORTS)
    assert capmi.ABI_VERSION == capmi.lib.capmi_abi_version() == 27


def _bad(fn, ok, **kw):
    a = list(ok)
    for pos, v in kw.items():
        a[int(pos[1:])] = v
    return fn(*a)


def test_entries_reject_bad_arguments_before_any_launch():
    """CAPMI_EINVAL / CAPMI_ERANGE: runs without a GPU."""
    import capmi
    lib = capmi.lib
    buf = (ctypes.c_float * 1024)()
    q = (ctypes.cast(buf, ctypes.c_void_p).value + 15) & ~15
    q2 = q + 2048
    # tokens T R start end pad lens caps count inv_count stream
    ok = [q, 4, 3, 1, 2, 0, q, q, q, q, None]
    pack = lambda **kw: _bad(lib.capmi_rollout_pack, ok, **kw)  # noqa: E731
    for bad in (dict(p0=None), dict(p6=None), dict(p7=None), dict(p9=None), dict(p1=0), dict(p2=0), dict(p3=-1),
                dict(p4=-1), dict(p5=-1)):
        assert pack(**bad) == EINVAL, bad
    assert pack(p1=1 << 16, p2=1 << 16) == ERANGE
    # tokens T R n lens img_key n_images V end score_end idf_keys idf_vals n_keys log_images ref_keys ref_w ref_off
    # ref_norm ref_bigrams img_off reward stream
    ok = [q, 12, 6, 3, q, q, 5, 100, 2, 1, q, q, 7, 1.5, q, q, q, q, q, q, q, None]
    rew = lambda **kw: _bad(lib.capmi_cider_reward, ok, **kw)  # noqa: E731
    for bad in (dict(p0=None), dict(p4=None), dict(p5=None), dict(p10=None), dict(p11=None), dict(p14=None),
                dict(p15=None), dict(p16=None), dict(p17=None), dict(p18=None), dict(p19=None), dict(p20=None),
                dict(p1=0), dict(p1=65), dict(p2=0), dict(p3=0), dict(p3=4), dict(p6=0), dict(p7=0), dict(p8=-1),
                dict(p12=-1), dict(p13=float("nan"))):
        assert rew(**bad) == EINVAL, bad
    assert rew(p7=65535) == ERANGE
    # reward greedy B n mode adv stats stream
    ok = [q, q, 3, 2, 0, q2, q2, None]
    adv = lambda **kw: _bad(lib.capmi_scst_advantage, ok, **kw)  # noqa: E731
    for bad in (dict(p0=None), dict(p5=None), dict(p6=None), dict(p2=0), dict(p3=0), dict(p4=2), dict(p4=-1),
                dict(p3=1), dict(p1=None, p4=1)):  # "mean" with n = 1; "greedy" without a greedy reward
        assert adv(**bad) == EINVAL, bad
    assert adv(p2=1 << 16, p3=1 << 16) == ERANGE
    # logits caps B T L V tgt_off lens t_first adv inv logp loss dlogits tm stream
    ok = [q, q, 2, 5, 6, 7, 1, q, 0, q, q, q2, q2, q2, 1, None]
    pg = lambda **kw: _bad(lib.capmi_pg_ce_fwd_bwd, ok, **kw)  # noqa: E731
    for bad in (dict(p0=None), dict(p1=None), dict(p7=None), dict(p9=None), dict(p11=None), dict(p12=None),
                dict(p2=0), dict(p3=0), dict(p5=0), dict(p6=-1), dict(p8=-1), dict(p4=5), dict(p10=None),
                dict(p13=q)):  # L < T + tgt_off; dlogits without inv_count; dlogits == logits
        assert pg(**bad) == EINVAL, bad
    assert pg(p2=1 << 16, p3=1 << 16, p4=1 << 17) == ERANGE


def test_parser_keeps_every_old_default_and_adds_the_flags():
    import train
    a = train.parse_args(["name", "--model", "baseline"])
    old = dict(attention_dim=512, decoder_dim=512, decoder_dropout=0.5, embed_size=512, epochs=1, batch_size=32,
               workers=1, encoder_lr=1e-4, decoder_lr=1e-4, grad_clip=5.0, alpha_c=1.0, fine_tune_encoder=False,
               fine_tune_embedding=False, checkpoint=None, print_freq=1, use_glove=False, max_caption_length=-1,
               use_bert=False, trusted_checkpoint=False, synthetic=False, synthetic_size=0, vocab_size=8100,
               bert_path=None, image_cache_gb=0)
    for k, v in old.items():
        assert getattr(a, k) == v, k
    new = dict(self_critical=False, sc_samples=5, sc_baseline="mean", sc_temperature=1.0, sc_top_k=0, sc_max_len=20)
    for k, v in new.items():
        assert getattr(a, k) == v, k
    assert set(vars(a)) == set(old) | set(new) | {"model_name", "model"}


def test_self_critical_needs_a_checkpoint_and_the_baseline_model():
    import train
    with pytest.raises(SystemExit) as e:
        train.main(["sc", "--model", "baseline", "--self_critical", "True", "--synthetic", "True"])
    assert "--checkpoint" in str(e.value)
    with pytest.raises(NotImplementedError):
        train.main(["sc", "--model", "attention", "--self_critical", "True", "--synthetic", "True",
                    "--checkpoint", "x.pth.tar"])
