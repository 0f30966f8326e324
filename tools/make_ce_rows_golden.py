"""Writes tests/golden/ce_rows.npz: the bit patterns the row cross-entropy entry points give on the cases of
tests/ce_rows_cases.py. Run on the MI355X against the library whose results are to be pinned:

    CAPMI_LIB=<that build's libcapmi.so> python tools/make_ce_rows_golden.py [out.npz]

The committed fixture was written by the library built from the commit before the three cross-entropy kernels
were merged into csrc/loss.hip. Regenerate it only together with a deliberate change of the row arithmetic."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "image-captioning-with-different-decoders_amd"), os.path.join(REPO, "tests")):
    sys.path.insert(0, p)


def main(argv):
    import ce_rows_cases as C
    from capmi import kernels as K
    from capmi._lib import LIB_PATH
    path = argv[0] if argv else C.GOLDEN
    arrays = {}
    for case in C.cases():
        for name, a in C.run(case, K).items():
            arrays[f"{case[0]}/{name}"] = a
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez_compressed(path, **arrays)
    print(f"{LIB_PATH}: {len(C.cases())} cases, {len(arrays)} arrays -> {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main(sys.argv[1:])
