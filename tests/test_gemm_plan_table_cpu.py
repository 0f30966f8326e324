"""CPU: the host GEMM planner (csrc/gemm_plan.hip) answers every query of tests/gemm_plan_queries.py as the pinned
table tests/golden/gemm_plan_table.npz says: rc, bm, bn, stream_k, generic and threads of capmi_gemm_sk_plan over
every flag value, tile, operand mode, the encoder's and decoder's shapes, the contract cases' layouts and the
epilogue / addressing variants that steer a branch. The table holds the answers of the planner as it stood before it
moved out of csrc/gemm.hip (generator and query list: tests/gemm_plan_queries.py)."""
import numpy as np
import pytest

import gemm_plan_queries as Q


def test_plan_table():
    from capmi._lib import GemmProblem, lib
    if lib.capmi_gemm_workspace_bytes() != Q.workspace_bytes(Q.CUS):
        pytest.skip(f"the table is the {Q.CUS}-CU answer; this device has another CU count")
    want = np.load(Q.TABLE)["rows"]
    qs = Q.queries(GemmProblem)
    assert len(qs) == len(want), f"{len(qs)} queries, {len(want)} pinned rows: regenerate the table with the list"
    got = Q.run(lib, qs)
    Q.check_not_hollow(qs, want)
    bad = np.nonzero((got != want).any(axis=1))[0]
    if len(bad):
        i = int(bad[0])
        label, a, b, tile, flags, _ = qs[i]
        raise AssertionError(f"{len(bad)} of {len(qs)} plan queries differ from the pinned table, first #{i}: {label} "
                             f"(amode {a}, bmode {b}, tile {tile}, flags {flags}): [rc, bm, bn, stream_k, generic, "
                             f"threads] = {got[i].tolist()}, pinned {want[i].tolist()}")
