"""SURVEY 8(f) row N4 on the CPU: the numpy oracle of the Reed-Solomon outer code (oracle/rs_oracle.py) against
  * tests/golden/rs_cases.json -- outputs of the reference's own MainEncoder / MainDecoder (Python + C++), and
  * the compiled reference codec program (oracle/_ref/schifra_RS_16bit_fileio_<fec>.out), block by block,
    including words the decoder must give up on -- its outputs on the test's seeded draw are recorded in
    tests/golden/rs_block_ref.npz (tests/golden/make_rs_block_ref.py), so that the test runs where the program is absent.
This is what pins the oracle; the GPU path is compared with the oracle in tests/test_gpu_rs.py."""
import json
import os

import numpy as np
import pytest

from oracle import rs_oracle as R

HERE = os.path.dirname(os.path.abspath(__file__))


def cases():
    return json.load(open(os.path.join(HERE, "golden", "rs_cases.json")))["cases"]


@pytest.mark.parametrize("i", range(10))
def test_oracle_matches_reference_main_encoder_decoder(i):
    c = cases()[i]
    reads = [bytes.fromhex(x) for x in c["reads"]]
    assert [e.hex() for e in R.MainEncoder(reads, c["redundancy"])] == c["encoded"]
    rx = [[j, bytes.fromhex(p)] for j, p in c["received"]]
    dec = R.MainDecoder(rx, c["redundancy"], c["total"])
    assert [d.hex() for d in dec] == c["decoded"]
    assert (dec == reads) == c["recovered"]


def test_golden_set_covers_failures():
    cs = cases()
    assert sum(not c["recovered"] for c in cs) >= 3 and sum(c["recovered"] for c in cs) >= 5
    # an undecodable column comes back as ASCII '0' bytes (RSCode_16bit_fileio.py:122-123)
    assert any(all(d[:4] == "3030" for d in c["decoded"]) for c in cs if not c["recovered"])


REF_BLOCKS = os.path.join(HERE, "golden", "rs_block_ref.npz")


def block_trials(fec):
    """the seeded draw of test_oracle_block_decoder_matches_reference_program: per trial the padded data block, the received
    word (erasures + errors, some in the padding) and the erased positions -> [(trial, full, rx, erl, S, E)]"""
    rng = np.random.default_rng(100 + fec)
    N = R.N
    out = []
    for trial in range(10):
        n_data = int(rng.integers(1, 30))
        n_total = n_data + fec
        pad = N - n_total
        full = np.concatenate([np.full(pad, R.PAD), rng.integers(0, 65536, size=n_data)])
        enc = R.encode_block(full, fec)
        S = min(int(rng.integers(0, fec + 2)) if trial % 3 else 0, n_total)
        E = int(rng.integers(0, fec // 2 + 3))
        er = sorted(rng.choice(n_total, size=S, replace=False).tolist())
        rx = enc.copy()
        rx[[pad + p for p in er]] = R.PAD
        anywhere = trial % 5 == 4                     # errors may also hit the padding that is not transmitted
        for p in rng.choice(N if anywhere else n_total, size=min(E, n_total), replace=False):
            rx[int(p) if anywhere else pad + int(p)] ^= int(rng.integers(1, 65536))
        out.append((trial, full, rx, [pad + p for p in er], S, E))
    return out


def recorded_ref_codec(rec, fec, trial, kind):
    """what the compiled reference program returned for this trial (tests/golden/make_rs_block_ref.py) -> (exit code, symbols | None)"""
    key = "f%d_t%d_%s" % (fec, trial, kind)
    out = rec[key + "_out"]
    return int(rec[key + "_rc"]), (out.astype(np.int64) if int(rec[key + "_wrote"]) else None)


@pytest.mark.parametrize("fec", [2, 6, 20])
def test_oracle_block_decoder_matches_reference_program(fec):
    """The block codec against the reference program's outputs on the same draw: the program itself where oracle/_ref has it
    (its outputs must also equal the recorded ones), the recorded outputs of tests/golden/rs_block_ref.npz everywhere."""
    rec = np.load(REF_BLOCKS)
    live = R.have_ref(fec)
    N = R.N
    seen = {True: 0, False: 0}

    def same(a, b):
        return a[0] == b[0] and (a[1] is None) == (b[1] is None) and (a[1] is None or np.array_equal(a[1], b[1]))

    for trial, full, rx, erl, S, E in block_trials(fec):
        enc = R.encode_block(full, fec)
        rc, ref_enc = recorded_ref_codec(rec, fec, trial, "enc")
        assert not live or same(R.ref_codec(fec, full, encode=True), (rc, ref_enc)), (fec, trial)
        assert rc == 0 and np.array_equal(ref_enc, enc)
        rc, ref_dec = recorded_ref_codec(rec, fec, trial, "dec")
        assert not live or same(R.ref_codec(fec, rx, erasures=erl), (rc, ref_dec)), (fec, trial)
        ok, blk = R.decode_block(rx, fec, erl)
        assert (rc == 0) == ok, (fec, trial, S, E)
        if ok:
            assert np.array_equal(blk[:N - fec], ref_dec), (fec, trial, S, E)
        seen[ok] += 1
    assert seen[True] >= 2 and seen[False] >= 1


def test_consensus_rule():
    """decode_RS_from_decoded_lists.py:37-51: most frequent payload per index; among equal counts the one that got there first"""
    a, b, c = b"aa", b"bb", b"cc"
    got = R.consensus([(3, a), (1, c), (3, b), (3, b), (3, a), (1, c), (7, a)])
    assert got == [[3, b], [1, c], [7, a]]
    assert R.consensus([(0, a), (0, b)]) == [[0, a]]
    assert R.consensus([(0, a), (0, b), (0, b), (0, a), (0, a)]) == [[0, a]]
