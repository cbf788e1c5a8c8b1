"""The read-mapping index built on the GPU (csrc/mi_kernels.hip through lva_map_index_create_device, read_map.MapIndex(device=0))
against the index the host builds and against read_map.ReferenceIndex expanded to the direct table: offsets, lists, match
masks and the three counts, byte for byte -- integers throughout, no tolerance.  Then map_reads with the resident index
against map_reads with the uploaded one, and the command line with --index device against --index host."""
import io

import numpy as np
import pytest

from nanopore_dna_storage_amd import read_map as rm

import map_index_util as U
import pooled_map_util as P
from test_gpu_read_map import barcoded, channel, fit, flip, pack  # noqa: F401  (barcoded: a fixture)

pytestmark = pytest.mark.gpu


def held(refs, k, max_occ=64, what=""):
    """the device-built tables and counts against the host-built ones and the definition's -> (tables, info)"""
    want = U.direct_tables(refs, k, max_occ)
    with rm.MapIndex(refs, k, max_occ) as host, rm.MapIndex(refs, k, max_occ, device=0) as dev:
        got, info = dev.tables(), dev.info()
        assert dev.device == 0 and host.device is None
        U.same_tables(got, host.tables(), what + " against the host index")
        assert info == host.info() == want[3], (what, info, host.info(), want[3])
    U.same_tables(got, want[:3], what + " against the definition")
    assert got[0][0] == 0 and got[0][-1] == info[1] == len(got[1])
    return got, info


# ---------------------------------------------------------------- tables

@pytest.mark.parametrize("k", [6, 9, 12])
def test_random_oligos_at_three_scan_lengths(k):
    """4^k + 1 = 4 097, 262 145, 16 777 217 offsets: one tile of the scan, 64 of them, 4 096 (their sums take 16 rounds)"""
    _, info = held(U.random_oligos(k, 300, 100), k, what="k=%d" % k)
    assert info[0] > 0 and (k == 6 or info[2] == 0)         # (at k = 6 a k-mer may be held by more than 64 of the 300)


@pytest.mark.parametrize("k", [6, 12])
def test_ragged_lengths(k):
    oligos = U.ragged(k)
    (offsets, lists, masks), info = held(oligos, k, what="ragged k=%d" % k)
    assert masks.shape == (len(oligos), 2, 4, 16)
    lens = [len(o) for o in oligos]
    assert 1 not in lists and lens.index(k - 1) not in lists and (lists == lens.index(k)).sum() == 1     # no k-mer, none, exactly one
    for o, m in enumerate(lens):                          # rows past the oligo's length stay clear, in both directions
        bits = np.unpackbits(masks[o].view(np.uint8), bitorder="little").reshape(2, 4, 1024)
        assert not bits[:, :, m:].any() and (bits[:, :, :m].sum(axis=1) == 1).all()


def test_a_single_oligo():
    for k, m in ((6, 6), (10, 115), (12, 1024)):
        _, info = held(U.random_oligos(m, 1, m), k, what="one oligo of %d" % m)
        assert info[0] == info[1] > 0


@pytest.mark.parametrize("k", [6, 12])
@pytest.mark.parametrize("where", U.N_WHERE)
def test_n_in_the_oligos(k, where):
    """an N restarts the run of bases; with one at every k-th position no k-mer is left: an index of no pairs"""
    (offsets, lists, _), info = held(U.with_n(k, where), k, what="N %s k=%d" % (where, k))
    if where == "every k":
        assert info == (0, 0, 0) and not offsets.any() and len(lists) == 0
    else:
        assert info[1] == 5 * (5 * k + 3 - k + 1 - (1 if where in ("first", "last") else k))


def test_repeats_inside_an_oligo():
    """an oligo counts a k-mer once: 1 019 positions of a homopolymer are one pair, a dinucleotide repeat gives two"""
    for k in (6, 12):
        assert held([np.full(1024, 2, np.uint8)], k, what="homopolymer")[1] == (1, 1, 0)
        assert held([np.resize(np.array([1, 3], np.uint8), 1024)], k, what="dinucleotide")[1] == (2, 2, 0)
    _, info = held(U.random_oligos(77, 1, 1024), 6, what="a random 1024-mer at k=6")
    assert info[0] == info[1] < 1019                      # (of 1 019 positions some repeat a 6-mer: 4 096 exist)
    _, info = held(list(U.random_oligos(78, 3, 1024)) + [np.resize(np.array([0, 1, 2], np.uint8), 700)], 6, what="four long oligos at k=6")
    assert info[1] > info[0]


def test_the_max_occ_boundary():
    """70 identical oligos: lists of 70 (past one wavefront) are kept with max_occ = 70 and all dropped with 69"""
    refs = np.repeat(U.random_oligos(5, 1, 90), 70, axis=0)
    (offsets, lists, _), info = held(refs, 8, 70, what="max_occ 70")
    assert info == (83, 83 * 70, 0) and (lists.reshape(83, 70) == np.arange(70)).all()
    (offsets, lists, _), info = held(refs, 8, 69, what="max_occ 69")
    assert info == (0, 0, 83) and not offsets.any() and len(lists) == 0


@pytest.mark.parametrize("max_occ", [65535, 1999, 64])
def test_long_segments(max_occ):
    """2 000 oligos that share their first 20 bases, k = 6: every 6-mer occurs, lists of every length up to 2 000 (past 64,
    256 and 1 024 entries) come out ascending; max_occ 1 999 drops the prefix's 15 k-mers, 64 drops more, beside kept lists"""
    (offsets, lists, _), info = held(U.shared_prefix(), 6, max_occ, what="shared prefix, max_occ %d" % max_occ)
    length = np.diff(offsets.astype(np.int64))
    if max_occ == 65535:
        assert info[0] == 4096 and info[2] == 0 and length.max() == 2000 and (length == 2000).sum() == 15 and info[1] == 187926
        assert sum(((length > lo) & (length <= hi)).any() for lo, hi in ((0, 64), (64, 256), (256, 1024), (1024, 2000))) >= 3
    else:
        assert info[2] >= 15 and info[0] + info[2] == 4096 and 0 < length.max() <= max_occ
    seg = np.repeat(np.arange(len(length)), length)
    assert (np.diff(lists)[np.diff(seg) == 0] > 0).all()   # ascending inside every k-mer


def test_three_builds_give_the_same_bytes():
    refs = U.shared_prefix()
    got = []
    for _ in range(3):
        with rm.MapIndex(refs, 6, 65535, device=0) as idx:
            got.append(tuple(t.tobytes() for t in idx.tables()) + (idx.info(),))
    assert got[0] == got[1] == got[2]


def test_two_indexes_alive_at_once():
    a_refs, b_refs = U.random_oligos(1, 40, 80), U.ragged(8)
    for first in (0, 1):
        a, b = rm.MapIndex(a_refs, 10, device=0), rm.MapIndex(b_refs, 8, device=0)
        (b, a)[first].close()
        left = (a, b)[first]
        U.same_tables(left.tables(), U.direct_tables((a_refs, b_refs)[first], left.k, 64)[:3], "the index left open")
        left.close()
        left.close()                                      # closing twice is closing once
        with pytest.raises(ValueError):
            left.tables()


# ---------------------------------------------------------------- mapping with the resident index

def same_maps(bases, win, refs, k=10, max_occ=64, groups=None, **kw):
    """map_reads with the index built on the device against map_reads with the one built on the host -> the latter"""
    with rm.MapIndex(refs, k, max_occ, groups) as host, rm.MapIndex(refs, k, max_occ, groups, device=0) as dev:
        want, got = rm.map_reads(bases, win, host, **kw), rm.map_reads(bases, win, dev, **kw)
        with pytest.raises(ValueError):
            rm.map_reads(bases, win, dev, device=1, **kw)
    assert got.out.dtype == np.int32 and got.out.tobytes() == want.out.tobytes()
    assert (got.supp is None) == (want.supp is None) and (got.supp is None or got.supp.out.tobytes() == want.supp.out.tobytes())
    return want


@pytest.fixture(scope="module")
def plain():
    """90 reads over 9 oligos of 115 bases, a third reverse strands, flanks, some junk"""
    rng = np.random.default_rng(141)
    refs = rng.integers(0, 4, (9, 115)).astype(np.uint8)
    reads = []
    for i in range(90):
        r = np.concatenate([rng.integers(0, 4, int(rng.integers(0, 30))), channel(rng, refs[rng.integers(0, 9)], 0.04, 0.04, 0.03),
                            rng.integers(0, 4, int(rng.integers(0, 30)))]).astype(np.uint8)
        reads.append(rng.integers(0, 4, 150).astype(np.uint8) if i % 17 == 0 else flip(r) if i % 3 == 0 else r)
    return pack(reads) + (refs,)


@pytest.mark.parametrize("chunk_reads", [0, 7])
def test_the_plain_path(plain, chunk_reads):
    bases, win, refs = plain
    assert same_maps(bases, win, refs, chunk_reads=chunk_reads).mapped >= 70


def test_one_small_case_against_the_definition(plain):
    bases, win, refs = plain
    with rm.MapIndex(refs, device=0) as dev:
        got = rm.map_reads(bases, win[:24], dev)
    assert got.out.tobytes() == rm.reference_map(bases, win[:24], refs).out.tobytes()


@pytest.mark.parametrize("chunk_reads", [0, 7])
def test_the_pooled_path(chunk_reads):
    """ragged oligos, a max_dist array, min_flank > 0: the constructed chimeric reads of tests/pooled_map_util.py"""
    oligos, groups = P.chimeric_pool()
    reads, rows, supp_rows = P.chimeric_reads()
    bases, win = pack(reads)
    max_dist = np.array([len(o) // 4 - (i % 3) for i, o in enumerate(oligos)])
    want = same_maps(bases, win, oligos, P.CHIM["k"], P.CHIM["max_occ"], groups, cands=P.CHIM["cands"], min_votes=P.CHIM["min_votes"],
                     max_dist=max_dist, min_flank=P.MIN_FLANK, chunk_reads=chunk_reads)
    P.expect(want.out, rows)
    P.expect(want.supp.out, supp_rows)


def test_past_one_vote_range():
    """4 099 distinct oligos of 12 bases at k = 6 (the construction of tests/test_gpu_read_map.py), reads from both ranges"""
    n_refs = rm.VOTE_RANGE + 3
    rng = np.random.default_rng(n_refs)
    ids = rng.permutation(4 ** 8)[:n_refs]
    refs = np.concatenate([(ids[:, None] >> (2 * np.arange(8))) & 3, rng.integers(0, 4, (n_refs, 4))], axis=1).astype(np.uint8)
    refs[n_refs - 1] = refs[0]
    reads = []
    for o in (0, 1, rm.VOTE_RANGE - 1, rm.VOTE_RANGE, n_refs - 2, n_refs - 1):
        reads += [refs[o], flip(refs[o]), fit(rng, np.concatenate([[1, 2], refs[o]]).astype(np.uint8), 20)]
    bases, win = pack(reads)
    assert same_maps(bases, win, refs, k=6, min_votes=1, cands=8, max_dist=3).mapped == len(reads)


def test_the_empty_index_maps_nothing():
    rng = np.random.default_rng(43)
    refs = rng.integers(0, 4, (3, 9)).astype(np.uint8)
    bases, win = pack([refs[0], rng.integers(0, 4, 40).astype(np.uint8), flip(refs[2])])
    assert same_maps(bases, win, refs, k=10).out.tolist() == [list(rm.UNMAPPED)] * 3
    assert same_maps(bases, win, [refs[0], refs[1][:4]], k=10, min_flank=5).out.tolist() == [list(rm.UNMAPPED)] * 3


def test_the_library_refuses_an_index_of_another_device(plain):
    """LVA_ERR_ARG with the other argument refusals: before n_reads = 0 succeeds and before the ordinal is looked at"""
    from nanopore_dna_storage_amd import _lib
    L = _lib.load_library()
    bases, win, refs = plain
    first, count, out = np.ascontiguousarray(win[:4, 0]), np.ascontiguousarray(win[:4, 1], dtype=np.int32), np.zeros((4, 8), np.int32)
    max_dist = np.full(len(refs), 28, np.int32)
    with rm.MapIndex(refs, device=0) as dev:
        for device, n, want in ((1, 4, -10), (9999, 4, -10), (1, 0, -10), (0, 0, 0), (0, 4, 0)):
            args = (device, dev.handle, bases.ctypes.data, first.ctypes.data, count.ctypes.data, n, 4, 2)
            assert L.lva_map_reads(*args, 28, 0, out.ctypes.data) == want, (device, n)
            assert L.lva_map_reads_pooled(*args, max_dist.ctypes.data, 0, 0, out.ctypes.data, None) == want, (device, n)


# ---------------------------------------------------------------- the command line

@pytest.mark.parametrize("more", [[], ["--min_flank", "30"]], ids=["plain", "pooled"])
def test_the_command_line_writes_the_same_files(barcoded, more):
    b = barcoded
    texts = {}
    for where in ("host", "device"):
        prefix = str(b["dir"] / ("idx_%s_%d" % (where, len(more))))
        out = io.StringIO()
        res = rm.main(b["files"] + more + ["--out_prefix", prefix, "--chunk", "7", "--index", where], out=out, decoder=b["dec"])
        names = [".map.tsv", ".coverage.tsv"] + ([".oligos.readids.txt"] if more else [])
        texts[where] = [open(prefix + n, "rb").read() for n in names] + [out.getvalue(), res.out.tobytes()]
        assert res.mapped >= 15
    assert texts["host"] == texts["device"]
