"""CPU: the beam-loop helper of the batched beam-search tests (tests/beam_cases.py) is pinned to
oracle.beam_ref.beam_search on the three beam_search_* goldens; the batched beam entry points
(capmi_beam_att_fwd / capmi_beam_select / capmi_beam_advance, ABI 27) validate before any launch."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import beam_cases as BC
from helpers import t
import gen


@pytest.mark.parametrize("tag", ["small", "k5", "noend"])
def test_helper_is_the_oracle(golden, tag):
    from oracle.beam_ref import beam_search
    fx = golden(f"beam_search_{tag}")
    m = fx["meta"]
    p = BC.golden_params(fx)
    feats = t(gen.encoder_features(m["seed"], 1)).view(1, 14, 14, 2048)
    seq, alphas, ok, (done, scores) = beam_search(p, feats, m["k"], m["start"], m["end"], return_all=True)
    got = BC.beam_loop(p, feats, m["k"], m["start"], m["end"])
    assert got["ok"] == ok == bool(fx["ok"]) and got["seq"] == seq == fx["seq"].tolist()
    assert got["done_seqs"] == done and got["done_scores"] == scores
    assert np.array_equal(np.array(got["alphas"]), np.array(alphas))
    assert len(got["live_seqs"]) == len(got["live_scores"]) == m["k"] - len(done)
    assert got["margin"] > 0
    if tag == "noend":
        assert not done and got["steps"] == 51 and all(len(s) == 52 for s in got["live_seqs"])


def test_helper_fp64_agrees_where_the_margin_allows(golden):
    """The same loop in fp64 takes the same decisions on a golden whose margin is far above fp32 rounding."""
    fx = golden("beam_search_noend")
    m = fx["meta"]
    p = BC.golden_params(fx)
    feats = t(gen.encoder_features(m["seed"], 1)).view(1, 14, 14, 2048)
    a = BC.beam_loop(p, feats, m["k"], m["start"], m["end"], max_steps=14)
    b = BC.beam_loop(p, feats, m["k"], m["start"], m["end"], max_steps=14, dtype=torch.float64)
    assert a["margin"] >= 1e-3
    assert a["live_seqs"] == b["live_seqs"] and a["steps"] == b["steps"] == 15
    np.testing.assert_allclose(a["live_scores"], b["live_scores"], rtol=1e-5)


def _lib():
    import capmi
    return capmi.lib


def test_beam_entry_points_reject_null_arguments():
    """CAPMI_EINVAL (1001) before any launch: runs without a GPU."""
    lib = _lib()
    buf = (ctypes.c_float * 64)()
    q = ctypes.cast(buf, ctypes.c_void_p).value
    att = [q, q, q, 1, 0, None, q, None, None, 0, 0, None, q, 1, 2, 4, 4, 4, q, None, None, None, None, 0, None]
    for hole in (0, 1, 2, 6, 12, 18):
        a = list(att)
        a[hole] = None
        assert lib.capmi_beam_att_fwd(*a) == 1001, hole
    for k in (0, 17):
        a = list(att)
        a[14] = k
        assert lib.capmi_beam_att_fwd(*a) == 1001, k
    sel = [q, q, q, 0, 1, 2, 8, q, q, q, q, q, None]
    for hole in (0, 1, 2, 7, 8, 9, 10, 11):
        a = list(sel)
        a[hole] = None
        assert lib.capmi_beam_select(*a) == 1001, hole
    for k, V in ((0, 8), (17, 100), (4, 3)):
        a = list(sel)
        a[5], a[6] = k, V
        assert lib.capmi_beam_select(*a) == 1001, (k, V)
    adv = [q, q, q, q, 1, 2, 4, 1, 0] + [q, q, q + 32, q + 64] + [q] * 10 + [None]
    for hole in [0, 1, 2, 3] + list(range(9, 23)):
        a = list(adv)
        a[hole] = None
        assert lib.capmi_beam_advance(*a) == 1001, hole
    for k in (0, 17):
        a = list(adv)
        a[5] = k
        assert lib.capmi_beam_advance(*a) == 1001, k
    a = list(adv)
    a[11] = a[9]  # h_dst == h_src
    assert lib.capmi_beam_advance(*a) == 1001


def test_exports_still_match_header():
    import capmi
    hdr = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "capmi.h")
    with open(hdr) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = sorted(set(re.findall(r"^\s*(?:const\s+)?(?:\w+\s+)*\w+\*?\s+\*?(capmi_\w+)\s*\(", text, flags=re.M)))
    assert sorted(capmi.EXPORTS) == declared
    assert {"capmi_beam_att_fwd", "capmi_beam_select", "capmi_beam_advance"} <= set(declared)
    assert capmi.ABI_VERSION == 27 == capmi.lib.capmi_abi_version()


def test_beam_size_limits_and_bert():
    import types
    from capmi.beam import BatchedBeamSearch
    dec = types.SimpleNamespace(use_bert=True)
    for k in (0, 17):
        with pytest.raises(ValueError):
            BatchedBeamSearch(dec, k)
    with pytest.raises(NotImplementedError):
        BatchedBeamSearch(dec, 5).search(torch.zeros(1, 4, 8), 1, 2)
