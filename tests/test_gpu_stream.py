"""Decode stream (lva_stream_* / Decoder.stream / Decoder.decode_iter): a read's list and scores must not depend on when it was
submitted or on what else is in flight -- bit for bit the batch call's, the oracle's and the reference's."""
import numpy as np
import pytest

import nanopore_dna_storage_amd as pkg
from nanopore_dna_storage_amd import synth
from nanopore_dna_storage_amd._lib import LvaError
from golden_util import as_strings, load_case

pytestmark = pytest.mark.gpu

N_READS = 40
ORACLE_SUBSET = (0, 1, 2)          # reads also decoded by the CPU oracle (remembered for the session across the kernel modes)


def _reads(m, r, msg_len, seed0):
    """seeded reads of mixed length and orientation; three of them too short for the reference (:600-601)"""
    reads = [synth.make_read(m, r, msg_len, seed0 + i, rc=bool(i % 3 == 0), margin=3.0 + (i % 4)) for i in range(N_READS)]
    for i in (5, 11, 30):
        reads[i]["post"] = reads[i]["post"][:-(1 + i % 2)].copy()     # both parities of the block count
    for i, keep in ((7, 30), (19, 1), (33, msg_len // 2)):
        reads[i]["post"] = reads[i]["post"][:keep].copy()
    assert len({x["post"].shape[0] & 1 for x in reads}) == 2
    return reads


def _drain(st, got):
    while st.outstanding:
        res = st.poll(wait=True)
        assert res, "poll(wait=True) came back empty with %d reads outstanding" % st.outstanding
        got.extend(res)


def _all_at_once(dec, reads):
    got = []
    with dec.stream(queue_cap=len(reads)) as st:
        for i, x in enumerate(reads):
            assert st.submit(x["post"], rc=x["rc"], tag=i)
        p = st.pending()
        assert p["queued"] + p["in_slots"] + p["finished"] == len(reads)
        _drain(st, got)
        assert st.pending() == dict(queued=0, in_slots=0, finished=0)
    return got, 0


def _one_at_a_time(dec, reads):
    got = []
    with dec.stream(queue_cap=4) as st:
        for i, x in enumerate(reads):
            while not st.submit(x["post"], rc=x["rc"], tag=i):
                got.extend(st.poll(wait=True))
            got.extend(st.poll(wait=False))
        _drain(st, got)
    return got, 0


def _bursts(dec, reads):
    rng = np.random.default_rng(2024)
    got, busy, i = [], 0, 0
    with dec.stream(queue_cap=2) as st:
        while i < len(reads):
            for _ in range(int(rng.integers(1, 7))):
                if i == len(reads):
                    break
                while not st.submit(reads[i]["post"], rc=reads[i]["rc"], tag=i):
                    busy += 1
                    got.extend(st.poll(wait=True))
                i += 1
            if rng.integers(2):
                got.extend(st.poll(wait=False))
        _drain(st, got)
    return got, busy


def _same(want, got, what):
    assert sorted(t for t, _ in got) == list(range(len(want))), "%s: every tag exactly once" % what
    for t, g in got:
        w = want[t]
        if isinstance(w, int):
            assert g == w, "%s read %d: %r, batch call %r" % (what, t, g, w)
            continue
        assert not isinstance(g, int), "%s read %d: error %r" % (what, t, g)
        assert g[0].shape == w[0].shape and np.array_equal(g[0], w[0]), "%s read %d: list differs from the batch call's" % (what, t)
        assert np.array_equal(g[1].view(np.uint32), w[1].view(np.uint32)), "%s read %d: scores differ from the batch call's" % (what, t)


SHAPES = {"m6_r1_L4": (6, 1, 60, 4, 20), "m8_r3_L8": (8, 3, 164, 8, 20), "m6_r1_L32": (6, 1, 60, 32, 20)}
MODES = [(s, k) for s in ("m6_r1_L4", "m8_r3_L8") for k in (0, 1, 2, 3, 4)] + [("m6_r1_L32", k) for k in (0, 1, 2, 3)]


@pytest.mark.parametrize("shape,kernel", MODES)
def test_arrival_time_does_not_matter(oracle, shape, kernel):
    m, r, msg_len, L, md = SHAPES[shape]
    reads = _reads(m, r, msg_len, 8100 + 10 * m + L)
    with pkg.Decoder(m, r, msg_len, list_size=L, max_deviation=md, kernel=kernel, max_slots=8) as dec:
        want = dec.decode([x["post"] for x in reads], rc=[x["rc"] for x in reads])
        assert [i for i, w in enumerate(want) if isinstance(w, int)] == [7, 19, 33] and want[7] == -6
        busy = {}
        for schedule in (_all_at_once, _one_at_a_time, _bursts):
            got, busy[schedule.__name__] = schedule(dec, reads)
            _same(want, got, schedule.__name__)
        assert busy["_bursts"] > 0, "queue_cap = 2 never pushed back"
        again = dec.decode([x["post"] for x in reads[:4]], rc=[x["rc"] for x in reads[:4]])       # the decoder is a batch decoder again
        _same(want[:4], list(enumerate(again)), "batch call after the streams")
    for i in ORACLE_SUBSET:
        wm, ws = oracle.OracleCode(m, r, msg_len, rc=reads[i]["rc"]).decode(reads[i]["post"], L, md, num_threads=16)
        assert np.array_equal(want[i][0], wm) and np.array_equal(want[i][1].view(np.uint32), ws.view(np.uint32))


def test_decode_iter_feeds_from_a_generator():
    m, r, msg_len, L, md = SHAPES["m6_r1_L4"]
    reads = _reads(m, r, msg_len, 8300)
    fetched = []

    def posts():
        for i, x in enumerate(reads):
            fetched.append(i)
            yield x["post"]

    with pkg.Decoder(m, r, msg_len, list_size=L, max_deviation=md, max_slots=4) as dec:
        want = dec.decode([x["post"] for x in reads], rc=[x["rc"] for x in reads])
        got, seen_early = [], None
        for i, res in dec.decode_iter(posts(), rc=(x["rc"] for x in reads)):
            if seen_early is None:
                seen_early = len(fetched)
            got.append((i, res))
    _same(want, got, "decode_iter")
    assert seen_early < len(reads), "the first result came only after the whole iterable had been read"


GOLDEN_M11 = ["m11_r5_L8_clean", "m11_r5_L8_clean_rc", "m11_r5_L8_noisy", "m11_r5_L8_noisy_rc"]


def test_m11_goldens_through_two_slots_with_short_reads_between():
    gold = [load_case(n) for n in GOLDEN_M11]
    m0 = gold[0][0]
    m, r, msg_len, L, md = m0["mem_conv"], m0["rate"], m0["msg_len"], m0["list_size"], m0["max_deviation"]
    assert (m, r, L) == (11, 5, 8)
    npos = pkg.code_info(m, r, msg_len).nstate_pos
    short = []
    for i in range(6):                                     # as short as the reference accepts, odd and even block counts
        x = synth.make_read(m, r, msg_len, 8500 + i, rc=bool(i & 1), margin=5.0)
        short.append(dict(post=x["post"][:npos + 1 + i].copy(), rc=x["rc"]))
    seq, short_at = [], []
    for k in range(6):
        short_at.append(len(seq))
        seq.append(short[k])
        if k < 4:
            seq.append(dict(post=gold[k][1], rc=gold[k][0]["rc"], lines=gold[k][2]))
    seq += [dict(post=g[1], rc=g[0]["rc"], lines=g[2]) for g in gold]          # and once more, behind each other
    with pkg.Decoder(m, r, msg_len, list_size=L, max_deviation=md, max_slots=2) as dec:
        assert dec.profile()["kernel"] == 4
        got = []
        with dec.stream(queue_cap=3) as st:
            for i, x in enumerate(seq):
                while not st.submit(x["post"], rc=x["rc"], tag=i):
                    got.extend(st.poll(wait=True))
            _drain(st, got)
        starts_odd = dec.profile()["step_launches"]
        want_short = dec.decode([x["post"] for x in short], rc=[x["rc"] for x in short])
    assert starts_odd > 0 and sorted(t for t, _ in got) == list(range(len(seq)))
    n_gold = 0
    for t, g in got:
        if "lines" in seq[t]:
            assert as_strings(g[0]) == seq[t]["lines"], "read %d differs from the reference's list" % t
            n_gold += 1
    assert n_gold == 8
    by_tag = dict(got)
    _same(want_short, [(k, by_tag[short_at[k]]) for k in range(len(short))], "short reads")

def test_tie_dense_stream_overflows_like_the_batch(monkeypatch):
    monkeypatch.setenv("LVA_WORK_CAP", "4")
    reads = synth.make_reads(6, 1, 60, 6, seed0=31, rc_mode="odd", margin=3.0, quantum=0.25)
    reads[1]["post"] = reads[1]["post"][:-1].copy()
    for kernel in (2, 4):
        with pkg.Decoder(6, 1, 60, list_size=8, max_deviation=20, kernel=kernel, max_slots=2) as dec:
            want = dec.decode([x["post"] for x in reads], rc=[x["rc"] for x in reads])
            batch = dec.profile()
            assert batch["overflow_steps"] > 0
            got, _ = _bursts(dec, reads)
            prof = dec.profile()
        _same(want, got, "kernel %d" % kernel)
        assert prof["overflow_steps"] > 0 and prof["step_launches"] > 0
        assert prof["read_steps"] == batch["read_steps"] == sum(x["post"].shape[0] for x in reads)
        assert prof["algorithmic_bytes"] == batch["algorithmic_bytes"] and prof["working_bytes"] == batch["working_bytes"]


def test_close_with_reads_in_flight_and_exclusive_use():
    m, r, msg_len, L, md = SHAPES["m6_r1_L4"]
    reads = [x for x in _reads(m, r, msg_len, 8700) if x["post"].shape[0] > 80]
    posts, rc = [x["post"] for x in reads], [x["rc"] for x in reads]
    with pkg.Decoder(m, r, msg_len, list_size=L, max_deviation=md, max_slots=4) as dec:
        want = dec.decode(posts, rc)
        st = dec.stream(queue_cap=10)
        for i in range(10):
            assert st.submit(posts[i], rc=rc[i])
        assert not st.submit(posts[10], rc=rc[10])          # ten reads wait for a slot: back-pressure, nothing taken
        st.poll(wait=False)                                 # launches are enqueued, reads sit in slots and in the queue
        p = st.pending()
        assert p["queued"] + p["in_slots"] + p["finished"] == 10 and p["queued"] > 0
        with pytest.raises(LvaError) as e:
            dec.decode(posts[:1])
        assert e.value.code == -13
        with pytest.raises(LvaError) as e:
            dec.stream()
        assert e.value.code == -13
        with pytest.raises(LvaError):
            dec.locate_payload(posts[:1], "ACGTACGTAC", "TGCATGCATG")
        st.close()                                          # drops what was not handed out
        st.close()                                          # (idempotent)
        _same(want, list(enumerate(dec.decode(posts, rc))), "batch call after close")
        with dec.stream() as st2:                           # and a new stream starts clean: nothing of the dropped reads comes out
            assert st2.poll(wait=True) == []
            assert st2.submit(posts[3], rc=rc[3], tag="x")
            got = st2.poll(wait=True)
        assert [t for t, _ in got] == ["x"] and np.array_equal(got[0][1][0], want[3][0])
