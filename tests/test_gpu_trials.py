"""Reading-cost trials on the GPU (lva_rs_trials through trials.run_trials, csrc/tr_kernels.hip) against the definition,
trials.reference_trials with the existing rs_code.MainDecoder, one trial at a time: all four statistics integer-exact,
and the vote's result where it is asked for.  Filter outputs are synthesised: index, payload, and an original that
rs_code.MainEncoder encoded."""
import io
import os

import numpy as np
import pytest

from nanopore_dna_storage_amd import decode_RS_from_decoded_lists, helper, rs_code, trials

pytestmark = pytest.mark.gpu


def make_code(rng, num_oligos, redundancy, bpo, cut=3, encoder=None):
    """-> (encoded payloads uint8 [num_oligos, bpo], original = the data without its last `cut` bytes)"""
    data = [bytes(rng.integers(0, 256, size=bpo, dtype=np.uint8)) for _ in range(num_oligos - redundancy)]
    enc = (encoder or rs_code.MainEncoder)(data, redundancy)
    return np.frombuffer(b"".join(enc), np.uint8).reshape(num_oligos, bpo).copy(), b"".join(data)[:len(data) * bpo - cut]


def make_reads(rng, enc, n, p_none=0.15, p_wrong=0.10):
    """n reads of random indices: some without an index, some with a wrong payload for theirs"""
    index = rng.integers(0, len(enc), size=n).astype(np.int32)
    payload = enc[index].copy()
    wrong = rng.random(n) < p_wrong
    payload[wrong] = rng.integers(0, 256, size=(int(wrong.sum()), enc.shape[1]), dtype=np.uint8)
    none = rng.random(n) < p_none
    index[none] = -1
    payload[none] = 0
    return index, payload


def both(index, payload, original, redundancy, num_oligos, points, num_trials, seed, **kw):
    bpo = payload.shape[1]
    want = trials.reference_trials(index, payload, original, bpo, redundancy, num_oligos, points, num_trials, seed,
                                   first_trial=kw.get("first_trial", 0), return_consensus=True)
    got = trials.run_trials(index, payload, original, bpo, redundancy, num_oligos, points, num_trials, seed, return_consensus=True, **kw)
    return want, got


def assert_same(want, got):
    for w, g, what in zip(want, got, ("stats", "present", "payload")):
        assert w.shape == g.shape and w.dtype == g.dtype, what
        bad = np.argwhere(w != g)
        assert len(bad) == 0, (what, bad[:5].tolist(), w[tuple(bad[0])], g[tuple(bad[0])])


MIXED_SEED = 11            # of the data; chosen so that the yardstick's outcomes are mixed (asserted below)


@pytest.fixture(scope="module")
def mixed():
    rng = np.random.default_rng(MIXED_SEED)
    enc, original = make_code(rng, 24, 6, 6)
    index, payload = make_reads(rng, enc, 150)
    return dict(index=index, payload=payload, original=original, fec=6, no=24, points=(0, 20, 40, 60, 150))


def test_mixed_outcomes(mixed):
    m = mixed
    want, got = both(m["index"], m["payload"], m["original"], m["fec"], m["no"], m["points"], 50, 5)
    succ = want[0][:, :, 3].sum(axis=1)
    print("successes per point:", succ.tolist())
    assert ((succ >= 10) & (succ <= 40)).any(), succ          # guards the test, not the code
    assert (want[0][0] == 0).all()
    assert_same(want, got)
    plain = trials.run_trials(m["index"], m["payload"], m["original"], 6, m["fec"], m["no"], m["points"], 50, 5)
    assert np.array_equal(plain, want[0])


def test_order_decides_a_tie():
    """one index with 3 + 3 votes for two payloads: the one whose third vote comes first in the trial's order wins"""
    rng = np.random.default_rng(2)
    enc, original = make_code(rng, 12, 4, 4)
    index = np.concatenate([np.zeros(6, np.int32), np.arange(1, 12, dtype=np.int32)])
    payload = enc[index].copy()
    payload[[0, 2, 4]] = (enc[0] ^ 0x5A)
    perm = rng.permutation(len(index))
    index, payload = index[perm], payload[perm]
    want, got = both(index, payload, original, 4, 12, (len(index),), 64, 77)
    winners = {bytes(p) for p in want[2][0, :, 0]}
    assert winners == {bytes(enc[0]), bytes(enc[0] ^ 0x5A)}, winners          # on the yardstick: both occur
    assert_same(want, got)


def test_more_reads_of_an_index_than_lanes():
    """130 reads of one index: three passes of 64 lanes, the majority payload reaching into the last one"""
    rng = np.random.default_rng(3)
    enc, original = make_code(rng, 12, 4, 4)
    index = np.concatenate([np.zeros(130, np.int32), np.arange(1, 12, dtype=np.int32)])
    payload = enc[index].copy()
    payload[:62] = enc[0] ^ 0xFF                          # 62 wrong votes first in read order, 68 right ones behind them
    want, got = both(index, payload, original, 4, 12, (70, 141), 8, 1)
    assert (want[2][1, :, 0] == enc[0]).all() and {bytes(p) for p in want[2][0, :, 0]} == {bytes(enc[0]), bytes(enc[0] ^ 0xFF)}
    assert_same(want, got)


@pytest.mark.parametrize("num_oligos,redundancy,n", [(65, 16, 63), (65, 16, 64), (129, 32, 65), (129, 32, 200), (12, 4, 1)])
def test_sizes_around_a_wavefront(num_oligos, redundancy, n):
    rng = np.random.default_rng(n)
    enc, original = make_code(rng, num_oligos, redundancy, 4)
    index = (np.arange(n, dtype=np.int32) * 7) % num_oligos
    want, got = both(index, enc[index].copy(), original, redundancy, num_oligos, (n,), 4, 3)
    assert (want[0][0, :, 1] == min(n, num_oligos)).all()
    assert (want[0][0, :, 3] == (min(n, num_oligos) >= num_oligos - redundancy)).all()
    assert_same(want, got)


def test_capacity_edge():
    rng = np.random.default_rng(5)
    no, fec, bpo = 24, 6, 6
    enc, original = make_code(rng, no, fec, bpo)
    for present, wrong, outcome in ((no - fec, 0, (no - fec, bpo // 2, 1)),      # every parity symbol spent on an erasure
                                    (no - fec - 1, 0, (no - fec - 1, 0, 0)),     # one erasure too many: refused
                                    (no - fec + 2, 1, (no - fec + 2, bpo // 2, 1))):   # four erasures and an error: corrected
        index = np.repeat(rng.permutation(no)[:present].astype(np.int32), 2)
        payload = enc[index].copy()
        if wrong:
            payload[index == index[0]] ^= 0x33
        want, got = both(index, payload, original, fec, no, (len(index),), 3, 8)
        assert (want[0][0, :, 1:] == outcome).all(), (present, wrong, want[0])
        assert_same(want, got)


def test_counter_based(mixed):
    m = mixed
    args = (m["index"], m["payload"], m["original"], 6, m["fec"], m["no"], m["points"])
    whole = trials.run_trials(*args, 40, 5, return_consensus=True)
    for chunk in (1, 7):
        assert_same(whole, trials.run_trials(*args, 40, 5, chunk_trials=chunk, return_consensus=True))
    assert_same(whole, trials.run_trials(*args, 40, 5, return_consensus=True))
    a = trials.run_trials(*args, 13, 5, return_consensus=True)
    b = trials.run_trials(*args, 27, 5, first_trial=13, return_consensus=True)
    assert_same(whole, tuple(np.concatenate([x, y], axis=1) for x, y in zip(a, b)))
    assert not np.array_equal(whole[0][:, :13], whole[0][:, 13:26])


def test_large_code():
    """beyond 256 parity symbols (several coefficients per thread) and past one wavefront of indices per erasure pass"""
    rng = np.random.default_rng(6)
    no, fec, bpo = 1100, 330, 18
    enc, original = make_code(rng, no, fec, bpo, cut=7)
    index, payload = make_reads(rng, enc, 3000)
    want, got = both(index, payload, original, fec, no, (1500, 2600), 8, 21)
    print("successes per point:", want[0][:, :, 3].sum(axis=1).tolist(), "columns_ok:", want[0][:, :, 2].tolist())
    assert_same(want, got)


def test_cli(tmp_path):
    """--trials device prints the reference's lines per sample size with reference_trials' outcomes; --trials host is untouched"""
    rng = np.random.default_rng(7)
    bpo, n_reads = 4, 120
    original = bytes(rng.integers(0, 256, size=62, dtype=np.uint8))
    (tmp_path / "orig").write_bytes(original)
    _, n_data, fec, no = helper.compute_parameters(bpo, 0.3, 64, False)
    data = original.ljust(64, b"0")
    enc = rs_code.MainEncoder([data[i * bpo:(i + 1) * bpo] for i in range(n_data)], fec)
    lists_dir = tmp_path / "lists"
    lists_dir.mkdir()
    index = np.full(n_reads, -1, np.int32)
    payload = np.zeros((n_reads, bpo), np.uint8)
    for i in range(n_reads):
        if i % 9 == 4:
            continue                                       # no list file
        k = int(rng.integers(no))
        good = helper.attach_index_crc(k, enc[k])
        junk = [good[:5] + ("1" if good[5] == "0" else "0") + good[6:], "0" * len(good)]
        if i % 7 == 3:
            lst = junk                                     # a list without a passing entry
        else:
            lst = [junk[0], good, junk[1]]
            index[i], payload[i] = k, np.frombuffer(enc[k], np.uint8)
        (lists_dir / ("list_%d" % i)).write_text("".join(e + "\n" for e in lst))
    base = ["--num_trials", "12", "--list_size", "8", "--num_reads_total", str(n_reads), "--bytes_per_oligo", str(bpo),
            "--decoded_lists_dir", str(lists_dir), "--rs_redundancy", "0.3", "--original_file", str(tmp_path / "orig"), "--seed", "3"]
    want = trials.reference_trials(index, payload, original, bpo, fec, no, (40, 80), 12, 3)
    assert 0 < want[:, :, 3].sum() < 24                    # guards the test: both words are printed
    lines = []
    for k, u in enumerate((40, 80)):
        lines += ["NUM_READS_TO_USE: %d" % u, "list size: 8"] + ["Success" if s else "Failure" for s in want[k, :, 3]]
        lines += ["NUM_TRIALS 12", "num_successes %d" % want[k, :, 3].sum()]
    for list_ops in ("host", "device"):
        out = io.StringIO()
        n = decode_RS_from_decoded_lists.main(base + ["--trials", "device", "--num_reads_to_use", "40,80", "--list_ops", list_ops], out=out)
        assert out.getvalue().splitlines() == lines and n == want[1, :, 3].sum()
    with pytest.raises(SystemExit):
        decode_RS_from_decoded_lists.main(base[:-2] + ["--trials", "device", "--num_reads_to_use", "40"], out=io.StringIO())
    # --trials host: the loop as it was, for one sample size
    import random
    rnd = random.Random(3)
    host = ["NUM_READS_TO_USE: 80", "list size: 8"]
    for _ in range(12):
        drawn = [i for i in rnd.sample(list(range(n_reads)), 80) if os.path.isfile(lists_dir / ("list_%d" % i))]
        lists = [(lists_dir / ("list_%d" % i)).read_text().split("\n")[:-1][:8] for i in drawn]
        d, passed = rs_code.decode_from_lists(lists, bpo, fec, no)
        host.append("Success" if passed > 0 and d[:len(original)] == original else "Failure")
    host += ["NUM_TRIALS 12", "num_successes %d" % host.count("Success")]
    out = io.StringIO()
    decode_RS_from_decoded_lists.main(base + ["--num_reads_to_use", "80"], out=out)
    assert out.getvalue().splitlines() == host
    out2 = io.StringIO()
    decode_RS_from_decoded_lists.main(base + ["--num_reads_to_use", "80", "--trials", "host"], out=out2)
    assert out2.getvalue() == out.getvalue()
