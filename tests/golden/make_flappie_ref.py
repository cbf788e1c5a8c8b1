#!/usr/bin/env python3
"""Records what the compiled flappie decode path (oracle/_ref/flappie_decode.out, built by oracle/Makefile's `flappieref`)
returns on every case of tests/flappie_cases.py: its posteriors of the score cases (in full up to STORE_POST_MAX blocks,
as SHA-256 + E_flappie beyond), and its basecall -- path, score bits, change positions, bases -- of its own posteriors and
of the two posterior inputs.  Build container only:

    python tests/golden/make_flappie_ref.py            -> tests/golden/flappie_ref.npz"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
from oracle import oracle as O  # noqa: E402
import flappie_cases as C  # noqa: E402


def main():
    assert O.have_flappie_ref(), "build oracle/_ref first (make -C oracle flappieref)"
    rec = {}
    for name in C.ALL_CASES:
        one = C.record_case(name, O)
        rec.update(one)
        print(name, C.case_input(name).shape[0], "blocks,", len(one[name + "__bases"]), "bases,",
              "posteriors stored" if name + "__post" in one else "posteriors as SHA-256" if name + "__post_sha" in one else "posterior input",
              flush=True)
    np.savez_compressed(C.FIXTURE, **rec)
    print(C.FIXTURE, os.path.getsize(C.FIXTURE), "bytes")


if __name__ == "__main__":
    main()
