#!/usr/bin/env python3
"""Records what the compiled reference RS codec program (oracle/_ref/schifra_RS_16bit_fileio_<fec>.out, built by
oracle/Makefile) returns on the seeded draw of tests/test_rs_oracle.py::test_oracle_block_decoder_matches_reference_program:
exit code and output symbols of the encode and of the decode call of every trial, and on the draw at large redundancies
(test_oracle_block_codec_matches_reference_program_at_large_redundancy): exit code, SHA-256 of the output symbols and,
for short blocks, the symbols behind the padding.  Build container only:

    python tests/golden/make_rs_block_ref.py            -> tests/golden/rs_block_ref.npz, rs_block_ref_large.npz
    python tests/golden/make_rs_block_ref.py large      -> tests/golden/rs_block_ref_large.npz only"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
from oracle import rs_oracle as R  # noqa: E402
import test_rs_oracle as T  # noqa: E402


def small():
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


def large():
    rec = {}

    def put(key, record):
        for k, v in record.items():
            rec["%s_%s" % (key, k)] = v

    for fec in T.LARGE_FEC:
        assert R.have_ref(fec), "build oracle/_ref first (make -C oracle rsref)"
        codewords = {}

        def encoded(n_total):
            if n_total not in codewords:
                rc, out = R.ref_codec(fec, T.large_block_data(fec, n_total), encode=True)
                assert rc == 0 and out is not None
                put("L%d_n%d_enc" % (fec, n_total), T.large_record(rc, out, n_total))
                codewords[n_total] = out
            return codewords[n_total]

        for name, n_total, _, rx, erl in T.large_block_trials(fec, encoded):
            rc, out = R.ref_codec(fec, rx, erasures=erl)
            put("L%d_%s_dec" % (fec, name), T.large_record(rc, out, n_total))
            print(fec, name, n_total, "exit", rc, "wrote" if out is not None else "no file", flush=True)
    np.savez_compressed(os.path.join(HERE, "rs_block_ref_large.npz"), **rec)


if __name__ == "__main__":
    if sys.argv[1:] != ["large"]:
        small()
    large()
