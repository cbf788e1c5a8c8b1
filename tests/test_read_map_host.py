"""Read mapping (read_map.py, lva_map_index_*, lva_map_reads, csrc/mp_kernels.hip) without a GPU: the definition on hand-made
cases with the expected rows written out, the start pass on a random sweep, the host-built index against the numpy index,
every refusal of the entry points before a device is looked for, the declarations, and the recovery of simulated reads by
the definition alone."""
import ctypes
import os
import re

import numpy as np
import pytest

from nanopore_dna_storage_amd import _lib, read_map as rm, simulate as S
from nanopore_dna_storage_amd.decoder import encode
from nanopore_dna_storage_amd.error_profile import MAX_READ, MAX_REF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nanopore_dna_storage_amd", "csrc")
ERR_ARG = -10

# two oligos of 20 bases that share no 6-mer with each other, with themselves elsewhere or with any reverse complement; 15
# positions hold a 6-mer
R0, R1 = "ACGTTGCATCAGGTTACTAG", "CTCAAGTCGGCTTAACGAGA"
K6 = dict(k=6, min_votes=2)


def rc(s):
    return s[::-1].translate(str.maketrans("ACGTN", "TGCAN"))


def one(read, refs=(R0, R1), **kw):
    return rm.reference_map(read, [[0, len(read)]], list(refs), **{**K6, **kw}).out.tolist()[0]


def test_the_hand_made_oligos_are_what_the_cases_assume():
    kmers = lambda s: [s[i:i + 6] for i in range(len(s) - 5)]
    both = kmers(R0) + kmers(R1)
    assert len(set(both)) == 30 and not set(both) & set(kmers(rc(R0)) + kmers(rc(R1)))


# (ref, best, rc, dist, start, count, votes, second)
CASES = {
    # all 15 positions vote; the other oligo gets no vote and is no candidate
    "an exact copy": (R0, {}, [0, 0, 0, 0, 0, 20, 15, -1]),
    "an exact copy of the other": (R1, {}, [1, 1, 0, 0, 0, 20, 15, -1]),
    # base 10 lies in the 6-mers of positions 5 .. 10: 15 - 6 votes
    "one substitution": (R0[:10] + "C" + R0[11:], {}, [0, 0, 0, 1, 0, 20, 9, -1]),
    # 19 bases, 14 positions, those at 5 .. 9 span the gap: 14 - 5 votes
    "one deletion": (R0[:10] + R0[11:], {}, [0, 0, 0, 1, 0, 19, 9, -1]),
    # 21 bases, 16 positions, those at 5 .. 10 hold the inserted base: 16 - 6 votes
    "one insertion": (R0[:10] + "T" + R0[10:], {}, [0, 0, 0, 1, 0, 21, 10, -1]),
    # the flanks vote for nobody; the alignment ends at column 25 and starts at 5
    "flanks on both sides": ("TTTTT" + R0 + "GGGGGGG", {}, [0, 0, 0, 0, 5, 20, 15, -1]),
    # as strand 1 the window is the read above: [5, 25) there is [32 - 25, 32 - 5) in the window as given
    "the reverse complement": (rc("TTTTT" + R0 + "GGGGGGG"), {}, [0, 0, 1, 0, 7, 20, 15, -1]),
    "the reverse complement of the other": (rc(R1), {}, [1, 1, 1, 0, 0, 20, 15, -1]),
    # N equals nothing: a substitution that also takes the 6-mers over it
    "N in the read": (R0[:10] + "N" + R0[11:], {}, [0, 0, 0, 1, 0, 20, 9, -1]),
    "a read shorter than k": (R0[:5], {}, list(rm.UNMAPPED)),
    "an empty read": ("", {}, list(rm.UNMAPPED)),
    "min_votes above any vote": (R0, dict(min_votes=16), list(rm.UNMAPPED)),
    "max_dist turns ref to -1, best stays": (R0[:10] + "C" + R0[11:], dict(max_dist=0), [-1, 0, 0, 1, 0, 20, 9, -1]),
    "max_dist is inclusive": (R0[:10] + "C" + R0[11:], dict(max_dist=1), [0, 0, 0, 1, 0, 20, 9, -1]),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_made_case(name):
    read, kw, want = CASES[name]
    assert one(read, **kw) == want
    if read:
        codes = np.array(["ACGTN".index(c) if c != "N" else 9 for c in read], np.uint8)          # lva_encode's codes are the same bases
        assert rm.reference_map(codes, [[0, len(codes)]], [R0, R1], **{**K6, **kw}).out.tolist()[0] == want


def test_n_in_the_oligo():
    """the oligo's 6-mers over its N are not in the index (positions 0 .. 4 and 11 .. 14 remain) and the N costs one"""
    assert one(R0, refs=(R0[:10] + "N" + R0[11:], R1)) == [0, 0, 0, 1, 0, 20, 9, -1]


def test_two_identical_oligos():
    """the same votes and the same distance: the lower id is first in the order and wins; second is the other's distance"""
    assert one(R0, refs=(R1, R0, R0)) == [1, 1, 0, 0, 0, 20, 15, 0]
    assert one(R0, refs=(R1, R0, R0), cands=1) == [1, 1, 0, 0, 0, 20, 15, -1]
    assert one(R0, refs=(R1, R0, R0), max_occ=1) == list(rm.UNMAPPED)              # every 6-mer of the read is shared: dropped


def test_the_result_type_and_its_helpers():
    reads = ["TT" + R0, rc(R1) + "A", "ACACACACAC"]
    bases = "".join(reads)
    off = np.cumsum([0] + [len(r) for r in reads])
    win = np.stack([off[:-1], np.diff(off)], axis=1)
    res = rm.reference_map(bases, win, [R0, R1], **K6)
    assert res.out.dtype == np.int32 and res.out.shape == (3, 8) and len(res) == 3 and res.mapped == 2
    assert res.ref.tolist() == [0, 1, -1] and res.rc.tolist() == [0, 1, 0] and res.dist.tolist() == [0, 0, -1]
    assert res.windows(win).tolist() == [[2, 20], [22, 20], [43, 0]] and res.windows(win).dtype == np.int64
    assert res.coverage(2).tolist() == [[1, 0], [0, 1]] and res.coverage(2).dtype == np.int64


def test_parameters_out_of_range_are_refused():
    for kw in (dict(k=5), dict(k=13), dict(max_occ=0), dict(max_occ=65536), dict(cands=0), dict(cands=9), dict(min_votes=0), dict(max_dist=-1)):
        with pytest.raises(ValueError):
            one(R0, **kw)


def test_the_start_pass_attains_the_distance():
    """E[m][j] >= d for every j and == d for one: the global distance of x[s:e] is d (error_profile's matrix says so too)"""
    from nanopore_dna_storage_amd.error_profile import _distance_matrix
    rng = np.random.default_rng(5)
    for trial in range(120):
        m, n = int(rng.integers(1, 40)), int(rng.integers(0, 60))
        alphabet = (2, 4, 5)[trial % 3]                                            # 5: with N
        ref, x = rng.integers(0, alphabet, m).astype(np.uint8), rng.integers(0, alphabet, n).astype(np.uint8)
        d, e = rm.end_distance(ref, x)
        E = rm.start_row(ref, x, e)
        assert E.min() == d and 0 <= d <= m, (trial, d, E.tolist())
        s = e - int(np.argmax(E == d))
        assert _distance_matrix(ref, x[s:e])[m][e - s] == d


# ---------------------------------------------------------------- the index built on the host

def index_info(refs, k, max_occ):
    with rm.MapIndex(refs, k, max_occ) as idx:
        return idx.info()


@pytest.mark.parametrize("k", [6, 10, 12])
def test_index_counts_equal_the_numpy_index(k):
    rng = np.random.default_rng(100 + k)
    for n_refs, ref_len, alphabet, max_occ in ((40, 30, 4, 64), (200, 16, 2, 3), (25, 50, 5, 2), (3, 12, 4, 1)):
        refs = rng.integers(0, alphabet, (n_refs, ref_len)).astype(np.uint8)
        refs[refs == 4] = ord("N")
        want = rm.ReferenceIndex(refs, k, max_occ).info()
        assert index_info(refs, k, max_occ) == want, (k, n_refs)
        assert want[0] > 0 or ref_len < k or alphabet == 2


def test_index_special_sets():
    rng = np.random.default_rng(9)
    refs = rng.integers(0, 4, (5, 40)).astype(np.uint8)
    dup = np.concatenate([refs, refs])                    # max_occ = 1: everything is shared and dropped
    want = rm.ReferenceIndex(dup, 10, 1).info()
    assert index_info(dup, 10, 1) == want and want[:2] == (0, 0) and want[2] == rm.ReferenceIndex(refs, 10, 1).info()[0] > 0
    homo = np.repeat(np.arange(4, dtype=np.uint8)[:, None], 30, axis=1)[[0, 0, 1, 2, 3, 3]]
    assert index_info(homo, 8, 64) == rm.ReferenceIndex(homo, 8, 64).info() == (4, 6, 0)
    assert index_info(homo, 8, 1) == rm.ReferenceIndex(homo, 8, 1).info() == (2, 2, 2)
    short = rng.integers(0, 4, (7, 9)).astype(np.uint8)   # ref_len < k: an empty index, no error
    assert index_info(short, 10, 64) == rm.ReferenceIndex(short, 10, 64).info() == (0, 0, 0)
    assert rm.reference_map(short[0], [[0, 9]], short).out.tolist() == [list(rm.UNMAPPED)]


# ---------------------------------------------------------------- refusals, before any device

def test_index_create_refusals():
    L = _lib.load_library()
    refs = np.zeros((2, 20), np.uint8)
    h = ctypes.c_void_p()
    create = lambda *a: L.lva_map_index_create(*a)
    p = refs.ctypes.data
    assert create(p, 2, 20, 5, 64, ctypes.byref(h)) == ERR_ARG and create(p, 2, 20, 13, 64, ctypes.byref(h)) == ERR_ARG
    assert create(p, 2, 20, 10, 0, ctypes.byref(h)) == ERR_ARG and create(p, 2, 20, 10, 65536, ctypes.byref(h)) == ERR_ARG
    assert create(p, 0, 20, 10, 64, ctypes.byref(h)) == ERR_ARG and create(p, 2, 0, 10, 64, ctypes.byref(h)) == ERR_ARG
    assert create(p, 2, MAX_REF + 1, 10, 64, ctypes.byref(h)) == ERR_ARG
    assert create(None, 2, 20, 10, 64, ctypes.byref(h)) == ERR_ARG and create(p, 2, 20, 10, 64, None) == ERR_ARG
    assert h.value is None
    assert L.lva_map_index_info(None, None, None, None) == ERR_ARG
    L.lva_map_index_destroy(None)                         # like free


def test_map_reads_refusals_need_no_device():
    L = _lib.load_library()
    bases = np.zeros(MAX_READ + 8, np.uint8)
    first, count, out = np.zeros(2, np.int64), np.array([10, 12], np.int32), np.zeros((2, 8), np.int32)
    with rm.MapIndex(np.zeros((2, 20), np.uint8)) as idx:
        def call(device=9999, index=idx.handle, b=bases.ctypes.data, f=first.ctypes.data, c=count.ctypes.data, n=2, cands=4, min_votes=2,
                 max_dist=5, chunk=0, o=out.ctypes.data):
            return L.lva_map_reads(device, index, b, f, c, n, cands, min_votes, max_dist, chunk, o)
        for kw in (dict(index=None), dict(b=None), dict(f=None), dict(c=None), dict(o=None), dict(n=-1), dict(cands=0), dict(cands=9),
                   dict(min_votes=0), dict(max_dist=-1), dict(chunk=-1)):
            assert call(**kw) == ERR_ARG, kw
        count[1] = MAX_READ + 1                           # a window past MAX_READ
        assert call() == ERR_ARG
        count[1] = -1
        assert call() == ERR_ARG
        count[1], first[0] = 12, -1
        assert call() == ERR_ARG
        first[0] = 0
        assert call(n=0) == 0                             # nothing to do: no device is looked for
        assert call() == -11                              # arguments pass: now the device ordinal is refused
    with pytest.raises(ValueError):
        rm.map_reads(bases, [[0, MAX_READ + 1]], rm.MapIndex(np.zeros((2, 20), np.uint8)))
    with pytest.raises(ValueError):
        rm.MapIndex(np.zeros((2, MAX_REF + 1), np.uint8))


# ---------------------------------------------------------------- declarations

def test_declarations():
    with open(os.path.join(ROOT, "include", "lva_decoder.h")) as f:
        header = f.read()
    assert "typedef struct lva_map_index lva_map_index;" in header and "#define LVA_ABI_VERSION 5" in header
    assert not re.search(r"struct lva_map_index\s*\{", header)                     # opaque
    flat = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    flat = re.sub(r"\s+", " ", flat)
    for proto in ("int lva_map_index_create(const uint8_t *refs, int32_t n_refs, int32_t ref_len, int32_t k, int32_t max_occ, lva_map_index **out);",
                  "void lva_map_index_destroy(lva_map_index *idx);",
                  "int lva_map_index_info(const lva_map_index *idx, int64_t *kmers, int64_t *pairs, int64_t *dropped_kmers);",
                  "int lva_map_reads(int32_t device, const lva_map_index *idx, const uint8_t *bases, const int64_t *first_base, "
                  "const int32_t *n_bases, int32_t n_reads, int32_t cands, int32_t min_votes, int32_t max_dist, int32_t chunk_reads , int32_t *out);"):
        assert proto in flat, proto
    names = ["lva_map_index_create", "lva_map_index_destroy", "lva_map_index_info", "lva_map_reads"]
    assert _lib.EXPORTS[-4:] == names and _lib.ABI_VERSION == 5
    with open(os.path.join(CSRC, "Makefile")) as f:
        make = f.read()
    assert re.search(r"^SRC\s*=.*\bmp_kernels\.hip\b", make, re.M) and re.search(r"^HDR\s*=.*\bmp_kernels\.h\b", make, re.M)


def test_vote_range_equals_the_header():
    with open(os.path.join(CSRC, "mp_kernels.h")) as f:
        text = f.read()
    with open(os.path.join(CSRC, "seq_bits.h")) as f:                              # the limits every sequence stage shares
        text += f.read()
    const = lambda name: int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))
    assert rm.VOTE_RANGE == const("kMpVoteRange") >= 4096                          # one experiment, one pass
    assert rm.MAX_CANDS == const("kMpMaxCands") and const("kMaxRef") == MAX_REF and const("kMaxRead") == MAX_READ
    assert re.search(r"kMpMinK = (\d+), kMpMaxK = (\d+)", text).groups() == tuple(str(v) for v in rm.K_RANGE)


# ---------------------------------------------------------------- recovery, the definition alone

CODE = (6, 1, 60)
SET = dict(sub=0.02, dele=0.02, ins=0.01)                 # the channel of tests/test_gpu_error_profile.py


def test_the_definition_recovers_every_simulated_read():
    """200 reads of a pool of 12 random messages, a coin per read for the strand, at sub 0.02, dele 0.02, ins 0.01 (the
    rates of tests/test_gpu_error_profile.py, unchanged): the definition with its defaults returns the source oligo and the
    strand of every read, and the mapped part's distance is a few edits."""
    pool = np.random.default_rng(7).integers(0, 2, size=(12, CODE[2]), dtype=np.uint8)
    oligos = encode(*CODE, pool)
    ref = S.reference_reads(*CODE, 200, 2026, scores=False, pool=pool, rc_mode=3, **SET)
    off = ref["base_offsets"]
    res = rm.reference_map(ref["bases"], np.stack([off[:-1], np.diff(off)], axis=1), oligos)
    assert np.array_equal(res.ref, ref["source"]) and np.array_equal(res.rc, ref["rc"].astype(np.int32))
    assert ref["rc"].any() and not ref["rc"].all() and res.dist.max() <= oligos.shape[1] // 4 and np.median(res.dist) <= 5
