#!/usr/bin/env python3
"""Records what the compiled reference RS codec program (oracle/_ref/schifra_RS_16bit_fileio_<fec>.out, built by
oracle/Makefile) returns on the seeded draw of tests/test_rs_oracle.py::test_oracle_block_decoder_matches_reference_program:
exit code and output symbols of the encode and of the decode call of every trial.  Build container only:

    python tests/golden/make_rs_block_ref.py        -> tests/golden/rs_block_ref.npz"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
from oracle import rs_oracle as R  # noqa: E402
import test_rs_oracle as T  # noqa: E402


def main():
    rec = {}
    for fec in (2, 6, 20):
        assert R.have_ref(fec), "build oracle/_ref first (make -C oracle rsref)"
        for trial, full, rx, erl, _, _ in T.block_trials(fec):
            for kind, (rc, out) in (("enc", R.ref_codec(fec, full, encode=True)), ("dec", R.ref_codec(fec, rx, erasures=erl))):
                key = "f%d_t%d_%s" % (fec, trial, kind)
                rec[key + "_rc"] = np.int32(rc)
                rec[key + "_wrote"] = np.int32(out is not None)
                rec[key + "_out"] = np.zeros(0, "<u2") if out is None else out.astype("<u2")
    np.savez_compressed(os.path.join(HERE, "rs_block_ref.npz"), **rec)


if __name__ == "__main__":
    main()
