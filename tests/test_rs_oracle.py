"""SURVEY 8(f) row N4 on the CPU: the numpy oracle of the Reed-Solomon outer code (oracle/rs_oracle.py) against
  * tests/golden/rs_cases.json -- outputs of the reference's own MainEncoder / MainDecoder (Python + C++), and
  * the compiled reference codec program (oracle/_ref/schifra_RS_16bit_fileio_<fec>.out), block by block,
    including words the decoder must give up on -- its outputs on the test's seeded draw are recorded in
    tests/golden/rs_block_ref.npz (tests/golden/make_rs_block_ref.py), so that the test runs where the program is absent.
    At redundancies 300, 1713 and 4096 (beyond one 256-thread pass, beyond 48 KB of LDS and at the kernel's limit) the
    outputs are recorded as exit code + SHA-256 in tests/golden/rs_block_ref_large.npz (large_block_trials below).
This is what pins the oracle; the GPU path is compared with the oracle in tests/test_gpu_rs.py and tests/test_gpu_rs_large.py."""
import hashlib
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


# ---------------------------------------------------------------- large redundancy: fec 300, 1713, 4096
LARGE_FEC = (300, 1713, 4096)
LARGE_REF_BLOCKS = os.path.join(HERE, "golden", "rs_block_ref_large.npz")
LARGE_SHORT = {300: 1000, 1713: 3000, 4096: 6000}          # n_total of the short block (<= 8192: its data symbols are recorded)
LARGE_MIX_S = {300: 258, 1713: 1001, 4096: 3000}           # erasures of the mixed cases: > 256, same parity as fec


def large_block_cases(fec):
    """-> [(name, n_total, S erasures, E errors at non-erased positions, positions that must be among the errors, class)]
    class: "clean"; "capacity" (S + 2E == fec or fec - 1 for errors only at odd fec: must come back as sent);
    "refused" (S > fec); "beyond" (S + 2E > fec: given up on, or miscorrected -- the reference decides)."""
    short, s_mix = LARGE_SHORT[fec], LARGE_MIX_S[fec]
    e_mix = (fec - s_mix) // 2
    assert s_mix > 256 and s_mix + 2 * e_mix == fec
    return [
        ("clean", short, 0, 0, (), "clean"),
        ("errors_cap", R.N, 0, fec // 2, (0, 1, R.N - 1), "capacity"),             # unshortened: first two and last symbol hit
        ("erasures_cap", R.N - 1, fec, 0, (), "capacity"),
        ("erasures_cap_short", short, fec, 0, (), "capacity"),
        ("refused", short, fec + 1, 0, (), "refused"),
        ("mix_cap", R.N - 2, s_mix, e_mix, (0, R.N - 3), "capacity"),
        ("mix_over", short, s_mix + 1, e_mix, (), "beyond"),                     # S + 2E == fec + 1
        ("errors_over", R.N - 1, 0, fec // 2 + 1, (0, R.N - 2), "beyond"),
        ("far", short, 0, fec, (), "beyond"),                                      # twice the capacity
    ]


def large_block_data(fec, n_total):
    """the padded data block of (fec, n_total): ASCII '0' padding in front of seeded random data symbols"""
    rng = np.random.default_rng([201, fec, n_total])
    return np.concatenate([np.full(R.N - n_total, R.PAD, dtype=np.int64), rng.integers(0, 65536, size=n_total - fec)])


def large_block_trials(fec, encoded):
    """the seeded draw at a large redundancy.  encoded(n_total) -> the codeword of large_block_data(fec, n_total).
    Erased symbols are overwritten with the dummy symbol; the E errors are drawn among the symbols that are NOT erased, so
    that a case at capacity is at capacity.  Yields (name, n_total, class, received word, erased positions in the full block)."""
    for idx, (name, n_total, S, E, forced, cls) in enumerate(large_block_cases(fec)):
        rng = np.random.default_rng([200, fec, idx])
        pad = R.N - n_total
        rx = encoded(n_total).copy()
        er = np.sort(rng.choice(n_total, size=S, replace=False))
        rx[pad + er] = R.PAD
        free = np.setdiff1d(np.arange(n_total), er)
        must = np.array([p for p in forced if p in set(free.tolist())], dtype=np.int64)
        rest = np.setdiff1d(free, must)
        pos = np.concatenate([must, rng.choice(rest, size=E - len(must), replace=False)]) if E else must[:0]
        assert len(pos) == E and len(set(pos.tolist())) == E and not set(pos.tolist()) & set(er.tolist())
        rx[pad + pos] ^= rng.integers(1, 65536, size=E)
        yield name, n_total, cls, rx, (pad + er).tolist()


def symbols_sha256(symbols):
    return np.frombuffer(hashlib.sha256(np.asarray(symbols, dtype="<u2").tobytes()).digest(), dtype=np.uint8)


def large_record(rc, out, n_total):
    """what is kept of one run of the reference program: exit code, whether it wrote a file, the SHA-256 of the symbols it wrote and,
    for a block of at most 8192 transmitted symbols, the symbols behind the padding themselves"""
    wrote = out is not None
    keep = out[R.N - n_total:] if wrote and n_total <= 8192 else np.zeros(0)
    return dict(rc=np.int32(rc), wrote=np.int32(wrote), sha=symbols_sha256(out) if wrote else np.zeros(32, np.uint8),
                data=np.asarray(keep, dtype="<u2"))


def same_record(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("rc", "wrote", "sha", "data"))


def recorded_large(rec, key):
    return {k: rec["%s_%s" % (key, k)] for k in ("rc", "wrote", "sha", "data")}


@pytest.mark.parametrize("fec", LARGE_FEC)
def test_oracle_block_codec_matches_reference_program_at_large_redundancy(fec):
    """decode_block / encode_block against the reference program at fec 300 (two passes of a 256-thread loop), 1713 (first
    size beyond 48 KB of LDS in the kernel) and 4096 (the kernel's limit): clean, exactly at capacity (errors only, erasures
    only with S == fec, a mix with S > 256), refused (S == fec + 1), one past capacity, far beyond it; unshortened blocks of
    65535, 65534 and 65533 symbols and short ones.  The program itself where oracle/_ref has it (its outputs must also equal
    the recorded ones), the record of tests/golden/rs_block_ref_large.npz everywhere."""
    rec = np.load(LARGE_REF_BLOCKS)
    live = R.have_ref(fec)
    N = R.N
    codewords = {}

    def encoded(n_total):
        if n_total not in codewords:
            full = large_block_data(fec, n_total)
            enc = R.encode_block(full, fec)
            want = recorded_large(rec, "L%d_n%d_enc" % (fec, n_total))
            assert not live or same_record(large_record(*R.ref_codec(fec, full, encode=True), n_total), want), (fec, n_total)
            assert int(want["rc"]) == 0 and int(want["wrote"]) == 1
            assert same_record(large_record(0, enc, n_total), want), (fec, n_total)
            codewords[n_total] = enc
        return codewords[n_total]

    seen = set()
    for name, n_total, cls, rx, erl in large_block_trials(fec, encoded):
        want = recorded_large(rec, "L%d_%s_dec" % (fec, name))
        assert not live or same_record(large_record(*R.ref_codec(fec, rx, erasures=erl), n_total), want), (fec, name)
        ok, blk = R.decode_block(rx, fec, erl)
        assert (int(want["rc"]) == 0) == ok == bool(want["wrote"]), (fec, name)
        if ok:
            assert same_record(large_record(0, blk[:N - fec], n_total), want), (fec, name)
        sent = np.array_equal(blk[:N - fec], large_block_data(fec, n_total))
        if cls in ("clean", "capacity"):
            assert ok and sent, (fec, name)
        elif cls == "refused":
            assert not ok, (fec, name)
        else:
            assert not (ok and sent), (fec, name)        # beyond capacity: given up on, or a miscorrection
        seen.add(cls)
        seen.add(n_total)
    assert seen >= {"clean", "capacity", "refused", "beyond", N, N - 1, N - 2, LARGE_SHORT[fec]}


def test_consensus_rule():
    """decode_RS_from_decoded_lists.py:37-51: most frequent payload per index; among equal counts the one that got there first"""
    a, b, c = b"aa", b"bb", b"cc"
    got = R.consensus([(3, a), (1, c), (3, b), (3, b), (3, a), (1, c), (7, a)])
    assert got == [[3, b], [1, c], [7, a]]
    assert R.consensus([(0, a), (0, b)]) == [[0, a]]
    assert R.consensus([(0, a), (0, b), (0, b), (0, a), (0, a)]) == [[0, a]]
