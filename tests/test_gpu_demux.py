"""DESIGN.md row N3' on the GPU: bc_search_multi / bc_demux_finalize through the C ABI.  Every comparison is on integers and
exact: against Decoder.locate_payload (one experiment), against the host yardstick helper.demux_barcodes (many), and of the
entry points against each other."""
import ctypes

import numpy as np
import pytest

import nanopore_dna_storage_amd as pkg
from nanopore_dna_storage_amd import _lib, helper, synth

from demux_util import INF, rand_bases, random_experiments, trans_for

pytestmark = pytest.mark.gpu

SB, EB = "CACCTGTGCTGCGTCAGGCTGTGTC", "GCTGTCCGTTCCGCATTGACACGGC"


@pytest.fixture(scope="module")
def dec():
    with pkg.Decoder(6, 1, 20, list_size=1, max_slots=1) as d:
        yield d


def _host(seqs, transs, exps, **kw):
    return [helper.demux_barcodes(s, t, exps, all=True, **kw) for s, t in zip(seqs, transs)]


def _check_bases(dec, seqs, transs, exps, **kw):
    got, table = dec.demux_bases(seqs, transs, exps, all=True, **kw)
    want = _host(seqs, transs, exps, **kw)
    assert len(got) == len(seqs)
    for i, (w, wt) in enumerate(want):
        assert table[i] == wt, (i, seqs[i])
        assert got[i] == w, (i, seqs[i])
    return got


def test_one_experiment_is_locate_payload(dec):
    """K = 1, no max_dist, min_margin 0: pos (and all_out[:, 0]) is what locate_payload gives -- forward, rc, a read without
    barcodes, a read of 0 blocks"""
    reads = [synth.make_barcoded_read(6, 1, 20, 500 + i, SB, EB, rc=bool(i & 1), flank=(3, 9))["post"] for i in range(4)]
    reads.append(np.random.default_rng(5).normal(0, 1, (200, 40)).astype(np.float32))
    reads.append(np.zeros((0, 40), np.float32))
    reads.append(synth.make_barcoded_read(6, 1, 20, 510, SB, EB, flank=(3, 9))["post"])
    want = dec.locate_payload(reads, SB, EB)
    got, table = dec.demux(reads, [(SB, EB, 6 + 20 + 1)], all=True)
    assert [w["ok"] for w in want[:4]] == [True] * 4 and [w["rc"] for w in want[:4]] == [False, True, False, True]
    assert not want[5]["ok"] and want[5]["start_pos"] == -1
    for w, g, t in zip(want, got, table):
        assert {k: g[k] for k in w} == w
        assert t == [w]
        assert g["experiment"] == (0 if w["start_pos"] != -1 else -1)
        assert g["reason"] == (1 if w["start_pos"] == -1 else 0 if w["ok"] else 4)
        assert (g["runner_up"], g["runner_up_dist"]) == (-1, INF)


@pytest.fixture(scope="module")
def pooled13(dec):
    """13 experiments of seeded 25-mer pairs, 26 pooled reads of both strands; the host yardstick on the device's basecalls
    (which tests/test_gpu_basecall.py holds to the oracle), computed once"""
    exps = random_experiments(43, 13, msg_len=20)
    reads, truth = synth.make_pooled_reads(exps, 26, seed0=4300, flank=(2, 6))
    posts = [x["post"] for x in reads]
    calls = dec.basecall(posts)
    want = _host([c[0] for c in calls], [c[1] for c in calls], exps)
    return exps, posts, truth, reads, want


def test_thirteen_experiments_match_the_yardstick(dec, pooled13):
    exps, posts, truth, reads, want = pooled13
    got, table = dec.demux(posts, exps, all=True)
    for i, (w, wt) in enumerate(want):
        assert table[i] == wt, i
        assert got[i] == w, i
    assert [g["experiment"] for g in got] == truth and all(g["reason"] == 0 for g in got)
    assert [g["rc"] for g in got] == [x["rc"] for x in reads]
    # the resident entry point: bit for bit what the host-buffer one gives
    dev, off = dec.upload(posts)
    try:
        got_r, table_r = dec.demux_resident(dev, off, exps, all=True)
        assert dec.demux_resident(dev, off, exps) == got
    finally:
        dec.free(dev)
    assert got_r == got and table_r == table


@pytest.mark.parametrize("n", [1, 7, 8, 9])
def test_batches_equal_reads_taken_alone(dec, pooled13, n):
    """the basecall packs 8 reads into a wavefront, the search indexes best[read][pattern]: a batch is its reads"""
    exps, posts, _, _, want = pooled13
    part = posts[5:5 + n]
    got, table = dec.demux(part, exps, all=True)
    for j, p in enumerate(part):
        one, one_t = dec.demux([p], exps, all=True)
        assert got[j] == one[0] and table[j] == one_t[0]
        assert got[j] == want[5 + j][0]


def test_bases_mixed_barcode_lengths(dec):
    """barcode lengths 1, 7, 25, 63, 64 in one table: the window ranges differ per pattern; reads for which ls + le > n holds
    for some experiments only; n odd and even; reads of 1 and 0 bases"""
    rng = np.random.default_rng(44)
    w = lambda n: rand_bases(rng, n)
    exps = [(w(1), w(7), 0), (w(7), w(1), 5), (w(25), w(25), 0), (w(63), w(64), 0), (w(64), w(63), 10), (w(64), w(64), 0),
            (w(1), w(1), 0), (w(25), w(7), 0)]
    seqs = []
    for n in (150, 151, 129, 128, 127, 126, 90, 51, 50, 49, 33, 32, 15, 14, 9, 8, 3, 2, 1, 0):
        s = w(n)
        if n >= 150:                                   # plant experiment 3 (forward) resp. 4 (other strand)
            sb, eb = exps[3][:2] if n == 150 else (helper.reverse_complement(exps[4][1]), helper.reverse_complement(exps[4][0]))
            s = sb + s[len(sb):n - len(eb) - 1] + eb + s[-1:]
            assert len(s) == n
        seqs.append(s)
    transs = [trans_for(rng, len(s)) for s in seqs]
    got = _check_bases(dec, seqs, transs, exps)
    assert (got[0]["experiment"], got[0]["rc"]) == (3, False) and (got[1]["experiment"], got[1]["rc"]) == (4, True)
    assert got[-1]["reason"] == 1 and got[-2]["reason"] == 1
    # reads one at a time give the same
    for i in (0, 1, 6, 12):
        assert dec.demux_bases([seqs[i]], [transs[i]], exps) == [got[i]]


def _plant(s, at, word):
    return s[:at] + word + s[at + len(word):]


def test_bases_long_read_equal_minima(dec):
    """1 300 bases: more than 256 windows per half, several passes per thread; two exact copies 256 windows apart (the same
    thread, different passes) and 64 apart (neighbouring wavefronts) in either half -- the first index wins"""
    rng = np.random.default_rng(45)
    n = 1300
    exps = [(rand_bases(rng, 12), rand_bases(rng, 12), 0), (rand_bases(rng, 11), rand_bases(rng, 13), 0)]
    seqs, where = [], []
    for gs, ge in ((256, 64), (64, 256)):
        s = rand_bases(rng, n)
        a, b = 300, n // 2 + 37
        s = _plant(_plant(s, a, exps[0][0]), a + gs, exps[0][0])
        s = _plant(_plant(s, b, exps[0][1]), b + ge, exps[0][1])
        seqs.append(s)
        where.append((a, b))
        s = helper.reverse_complement(rand_bases(rng, n))              # the other strand of experiment 1
        rs, re_ = helper.reverse_complement(exps[1][1]), helper.reverse_complement(exps[1][0])
        s = _plant(_plant(s, a + 5, rs), a + 5 + gs, rs)
        s = _plant(_plant(s, b + 5, re_), b + 5 + ge, re_)
        seqs.append(s)
        where.append((a + 5, b + 5))
    transs = [np.arange(1, n + 1) * 2 for _ in seqs]
    got = _check_bases(dec, seqs, transs, exps)
    for g, s, (a, b), k in zip(got, seqs, where, (0, 1, 0, 1)):
        ls = len(exps[k][0]) if k == 0 else len(exps[k][1])
        assert (g["experiment"], g["rc"], g["dist_start"], g["dist_end"]) == (k, k == 1, 0, 0)
        assert g["start_pos"] == 2 * (a + ls + 1) - 1 and g["end_pos"] == 2 * b - 1      # the FIRST copies


def test_bases_n_in_the_text(dec):
    rng = np.random.default_rng(46)
    exps = [(rand_bases(rng, 9), rand_bases(rng, 9), 0), (rand_bases(rng, 9), rand_bases(rng, 9), 0)]
    s = rand_bases(rng, 6) + exps[1][0] + rand_bases(rng, 30) + exps[1][1] + rand_bases(rng, 5)
    at = 6 + 4
    withn = s[:at] + "N" + s[at + 1:]
    alln = "N" * len(s)
    seqs = [s, withn, alln, withn.replace("A", "N")]
    got = _check_bases(dec, seqs, [trans_for(rng, len(x)) for x in seqs], exps)
    assert got[0]["dist_start"] == 0 and got[1]["dist_start"] == 1 and got[1]["experiment"] == 1
    assert got[2]["dist_start"] == 9 and got[2]["dist_end"] == 9


def test_bases_64_experiments(dec):
    rng = np.random.default_rng(47)
    exps = [(rand_bases(rng, int(rng.integers(5, 9))), rand_bases(rng, int(rng.integers(5, 9))), int(rng.integers(0, 30)))
            for _ in range(64)]
    seqs = []
    for e in (0, 31, 63, 17):
        s = rand_bases(rng, 4) + exps[e][0] + rand_bases(rng, 25) + exps[e][1] + rand_bases(rng, 3)
        seqs.append(s if e != 17 else helper.reverse_complement(s))
    seqs.append(rand_bases(rng, 41))
    got = _check_bases(dec, seqs, [trans_for(rng, len(x)) for x in seqs], exps)
    assert [g["experiment"] for g in got[:4]] == [0, 31, 63, 17] and got[3]["rc"]


def test_reasons_and_boundaries(dec):
    rng = np.random.default_rng(48)
    a = (rand_bases(rng, 10), rand_bases(rng, 10))
    b = (rand_bases(rng, 10), rand_bases(rng, 10))
    flip = lambda w, i: w[:i] + "ACGT"[("ACGT".index(w[i]) + 1) % 4] + w[i + 1:]
    clean = rand_bases(rng, 5) + a[0] + rand_bases(rng, 40) + a[1] + rand_bases(rng, 6)
    worn = rand_bases(rng, 5) + flip(a[0], 4) + rand_bases(rng, 40) + flip(a[1], 6) + rand_bases(rng, 6)
    seqs = [clean, worn, "ACGTACG", ""]
    transs = [np.arange(1, len(s) + 1) * 3 for s in seqs]
    exps = [a + (30,), b + (30,)]
    base = _check_bases(dec, seqs, transs, exps)
    assert [g["reason"] for g in base] == [0, 0, 1, 1]
    total, lead = base[1]["dist_start"] + base[1]["dist_end"], base[1]["runner_up_dist"] - (base[1]["dist_start"] + base[1]["dist_end"])
    assert total >= 1 and 0 < lead < INF
    got = _check_bases(dec, seqs, transs, exps, max_dist=total)            # total == max_dist passes
    assert got[1]["reason"] == 0
    got = _check_bases(dec, seqs, transs, exps, max_dist=total - 1)
    assert [g["reason"] for g in got] == [0, 2, 1, 1] and got[1]["experiment"] == 0 and not got[1]["ok"]
    got = _check_bases(dec, seqs, transs, exps, min_margin=lead)            # runner_up_dist - total == min_margin passes
    assert got[1]["reason"] == 0
    got = _check_bases(dec, seqs, transs, exps, min_margin=lead + 1)
    assert got[1]["reason"] == 3 and got[1]["start_pos"] == base[1]["start_pos"] and not got[1]["ok"]
    width = base[0]["end_pos"] - base[0]["start_pos"] + 1
    assert _check_bases(dec, seqs, transs, [a + (width,), b + (30,)])[0]["reason"] == 0
    got = _check_bases(dec, seqs, transs, [a + (width + 1,), b + (30,)])
    assert got[0]["reason"] == 4 and got[0]["experiment"] == 0 and not got[0]["ok"]
    # identical pairs: the lower index wins, and is ambiguous as soon as a margin is asked for
    twins = [b + (0,), a + (0,), a + (0,)]
    got = _check_bases(dec, seqs[:1], transs[:1], twins)
    assert (got[0]["experiment"], got[0]["runner_up"], got[0]["runner_up_dist"], got[0]["reason"]) == (1, 2, 0, 0)
    assert _check_bases(dec, seqs[:1], transs[:1], twins, min_margin=1)[0]["reason"] == 3
    # a margin larger than any int32 difference and no runner-up: never ambiguous
    assert _check_bases(dec, seqs[:1], transs[:1], [a + (0,)], min_margin=2 ** 31 - 1)[0]["reason"] == 0


def _raw(dec, exps, n_exps=None, min_margin=0, n_reads=1):
    L = _lib.load_library()
    arr = (_lib.ExperimentBarcodes * max(len(exps), 1))()
    for x, (sb, eb) in zip(arr, exps):
        x.start_barcode, x.end_barcode, x.min_len = sb, eb, 0
    bases = np.frombuffer(b"ACGTACGTACGTACGTACGT", dtype=np.uint8).copy()
    trans = np.arange(1, 21, dtype=np.uint32)
    off = np.array([0, 20], np.int64)
    post = np.zeros((20, 40), np.float32)
    res = (_lib.DemuxPos * 1)()
    k = len(exps) if n_exps is None else n_exps
    return (L.lva_demux_bases_batch(dec._h, bases.ctypes.data, trans.ctypes.data, off.ctypes.data, n_reads, arr, k, -1, min_margin, res, None),
            L.lva_demux_batch(dec._h, post.ctypes.data, off.ctypes.data, n_reads, arr, k, -1, min_margin, res, None))


def test_argument_errors(dec):
    ok = [(b"ACGT", b"TTGA")]
    assert _raw(dec, ok) == (0, 0)
    assert _raw(dec, ok, n_reads=0) == (0, 0)
    assert _raw(dec, ok, n_exps=0) == (-10, -10)
    assert _raw(dec, ok * 65) == (-10, -10)
    assert _raw(dec, ok * 64) == (0, 0)
    assert _raw(dec, [(b"A" * 65, b"TTGA")]) == (-10, -10)
    assert _raw(dec, [(b"A" * 64, b"TTGA")]) == (0, 0)
    assert _raw(dec, [(b"ACGT", b"")]) == (-10, -10)
    assert _raw(dec, [(b"", b"ACGT")]) == (-10, -10)
    assert _raw(dec, [(b"ACGT", None)]) == (-10, -10)
    assert _raw(dec, [(b"ACXT", b"TTGA")]) == (-10, -10)
    assert _raw(dec, [(b"ACGT", b"ttga")]) == (-10, -10)
    assert _raw(dec, [(b"ACNT", b"TTGA")]) == (0, 0)
    assert _raw(dec, ok, min_margin=-1) == (-10, -10)
    assert _raw(dec, ok + [(b"ACGT", b"TTGU")]) == (-10, -10)           # any experiment of the table
    with pytest.raises(pkg.LvaError) as e:
        dec.demux_bases(["ACGTACGTAC"], [np.arange(1, 11)], [])
    assert e.value.code == -10
    assert dec.demux([], [("ACGT", "TTGA", 0)]) == [] and dec.demux_bases([], [], [("ACGT", "TTGA", 0)], all=True) == ([], [])


def test_busy_while_a_stream_is_open(dec):
    post = synth.make_barcoded_read(6, 1, 20, 520, SB, EB, flank=(3, 9))["post"]
    dev, off = dec.upload([post])
    try:
        with dec.stream():
            for call in (lambda: dec.demux([post], [(SB, EB, 0)]), lambda: dec.demux_resident(dev, off, [(SB, EB, 0)]),
                         lambda: dec.demux_bases(["ACGTACGTAC"], [np.arange(1, 11)], [("ACG", "TTG", 0)])):
                with pytest.raises(pkg.LvaError) as e:
                    call()
                assert e.value.code == _lib.ERR_BUSY
        assert dec.demux_resident(dev, off, [(SB, EB, 0)])[0]["reason"] == 0
    finally:
        dec.free(dev)
