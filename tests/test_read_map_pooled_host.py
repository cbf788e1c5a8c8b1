"""A pooled run mapped (read_map.py, lva_map_index_create_pooled, lva_map_reads_pooled) without a GPU: the extended definition
is today's on equally long oligos, the host-built index of ragged oligos against the numpy index, the refusals before a
device is looked for, nested prefixes and constructed chimeric reads against a plain full-matrix statement of the definition
(tests/pooled_map_util.py), the recovery of three simulated pools by the definition alone, and the declarations."""
import ctypes
import os
import re

import numpy as np
import pytest

from nanopore_dna_storage_amd import _lib, read_map as rm, simulate as S
from nanopore_dna_storage_amd.decoder import encode
from nanopore_dna_storage_amd.error_profile import MAX_READ, MAX_REF

import pooled_map_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -10


# ---------------------------------------------------------------- equal lengths: nothing moves

def test_equal_lengths_give_the_rows_of_the_recovery_test():
    """the inputs of tests/test_read_map_host.py's recovery test (its first 60 reads): the oligos as a rectangular array, as
    strings of one length, as a flat array with offsets, max_dist in its three forms -- the same rows, and they are the
    source and strand of every read, which is what the definition returned before it knew of lengths"""
    code = (6, 1, 60)
    pool = np.random.default_rng(7).integers(0, 2, size=(12, code[2]), dtype=np.uint8)
    oligos = encode(*code, pool)
    ref = S.reference_reads(*code, 200, 2026, scores=False, pool=pool, rc_mode=3, sub=0.02, dele=0.02, ins=0.01)
    off = ref["base_offsets"][:61]
    win = np.stack([off[:-1], np.diff(off)], axis=1)
    want = rm.reference_map(ref["bases"], win, oligos)
    assert np.array_equal(want.ref, ref["source"][:60]) and np.array_equal(want.rc, ref["rc"][:60].astype(np.int32))
    assert want.supp is None and not want.chimeric.any() and want.groups is None
    m = oligos.shape[1]
    forms = [dict(refs=["".join("ACGT"[b] for b in o) for o in oligos]),
             dict(refs=(np.ascontiguousarray(oligos.reshape(-1)), np.arange(13, dtype=np.int64) * m)),
             dict(refs=oligos, max_dist=m // 4), dict(refs=oligos, max_dist=np.full(12, m // 4))]
    for kw in forms:
        assert np.array_equal(rm.reference_map(ref["bases"], win, **kw).out, want.out), list(kw)
    plain = [U.plain_row(rm._CODE[ref["bases"][f:f + c]], list(oligos), 10, 64, 4, 2, np.full(12, m // 4)) for f, c in win[:12]]
    assert plain == want.out[:12].tolist()


# ---------------------------------------------------------------- the index

def pooled_info(flat, off, k, max_occ):
    L = _lib.load_library()
    h = ctypes.c_void_p()
    assert L.lva_map_index_create_pooled(flat.ctypes.data, off.ctypes.data, len(off) - 1, k, max_occ, ctypes.byref(h)) == 0
    got = (ctypes.c_int64 * 3)()
    assert L.lva_map_index_info(h, *(ctypes.addressof(got) + 8 * i for i in range(3))) == 0
    L.lva_map_index_destroy(h)
    return tuple(int(x) for x in got)


@pytest.mark.parametrize("k", [6, 10])
def test_the_pooled_index_counts(k):
    rng = np.random.default_rng(300 + k)
    for n_refs, ref_len, alphabet, max_occ in ((40, 30, 4, 64), (200, 16, 2, 3), (25, 50, 5, 2)):
        refs = rng.integers(0, alphabet, (n_refs, ref_len)).astype(np.uint8)
        refs[refs == 4] = ord("N")
        with rm.MapIndex(refs, k, max_occ) as idx:                                 # lva_map_index_create
            want = idx.info()
        assert pooled_info(refs.reshape(-1).copy(), np.arange(n_refs + 1, dtype=np.int64) * ref_len, k, max_occ) == want
        lens = rng.integers(1, 2 * ref_len, n_refs)                                # ragged, some shorter than k
        lens[:3] = (1, k - 1, k)
        ragged = [rng.integers(0, alphabet, int(m)).astype(np.uint8) for m in lens]
        o = rm.Oligos(ragged)
        want = rm.ReferenceIndex(ragged, k, max_occ).info()
        assert pooled_info(o.flat, o.off, k, max_occ) == want and (want[0] > 0 or alphabet == 2)
        with rm.MapIndex(ragged, k, max_occ) as idx:
            assert idx.info() == want and idx.ragged and idx.refs is None and idx.lens.tolist() == lens.tolist() and idx.ref_len == lens.max()


def test_refs_in_every_form_are_the_same_oligos():
    a = rm.Oligos(["ACGT", "AC", "GGGTT"])
    b = rm.Oligos([np.frombuffer(s, np.uint8) for s in (b"ACGT", b"AC", b"GGGTT")])
    c = rm.Oligos((a.flat, a.off))
    for o in (a, b, c):
        assert o.lens.tolist() == [4, 2, 5] and bytes(o[2]) == b"GGGTT" and o.refs is None and len(o) == 3
    assert rm.Oligos(["ACGT", "TTTT"]).refs.shape == (2, 4)
    for bad in ([], ["ACGT", ""], ["A" * (MAX_REF + 1)], (a.flat, a.off[:-1].copy())):
        with pytest.raises(ValueError):
            rm.Oligos(bad)


# ---------------------------------------------------------------- refusals, before any device

def test_pooled_index_refusals():
    L = _lib.load_library()
    flat = np.zeros(4 * MAX_REF, np.uint8)
    h = ctypes.c_void_p()

    def create(off, n=None, k=10, max_occ=64, refs=flat.ctypes.data, out=ctypes.byref(h)):
        off = np.array(off, np.int64)
        return L.lva_map_index_create_pooled(refs, off.ctypes.data, len(off) - 1 if n is None else n, k, max_occ, out)

    assert create([0, 20, 20, 40]) == ERR_ARG                                      # a length of 0
    assert create([0, 20, MAX_REF + 21]) == ERR_ARG                                # MAX_REF + 1
    assert create([0, 30, 20, 50]) == ERR_ARG                                      # descending
    assert create([5, 30]) == ERR_ARG                                              # not from 0
    assert create([0, 20], n=0) == ERR_ARG and create([0, 20], k=5) == ERR_ARG and create([0, 20], k=13) == ERR_ARG
    assert create([0, 20], max_occ=0) == ERR_ARG and create([0, 20], max_occ=65536) == ERR_ARG
    assert create([0, 20], refs=None) == ERR_ARG and create([0, 20], out=None) == ERR_ARG
    assert L.lva_map_index_create_pooled(flat.ctypes.data, None, 1, 10, 64, ctypes.byref(h)) == ERR_ARG
    assert h.value is None
    assert create([0, 1, MAX_REF + 1]) == 0 and h.value is not None                # lengths 1 and MAX_REF
    L.lva_map_index_destroy(h)


def test_map_reads_pooled_refusals_need_no_device():
    L = _lib.load_library()
    bases = np.zeros(MAX_READ + 8, np.uint8)
    first, count = np.zeros(2, np.int64), np.array([10, 12], np.int32)
    out, supp, md = np.zeros((2, 8), np.int32), np.zeros((2, 8), np.int32), np.array([5, 6], np.int32)
    with rm.MapIndex(["A" * 20, "C" * 30]) as idx:
        assert idx.ragged
        # the equal-length entry point refuses the ragged index
        assert L.lva_map_reads(9999, idx.handle, bases.ctypes.data, first.ctypes.data, count.ctypes.data, 2, 4, 2, 5, 0, out.ctypes.data) == ERR_ARG

        def call(device=9999, index=idx.handle, b=bases.ctypes.data, f=first.ctypes.data, c=count.ctypes.data, n=2, cands=4, min_votes=2,
                 max_dist=md.ctypes.data, min_flank=0, chunk=0, o=out.ctypes.data, s=None):
            return L.lva_map_reads_pooled(device, index, b, f, c, n, cands, min_votes, max_dist, min_flank, chunk, o, s)
        for kw in (dict(index=None), dict(b=None), dict(f=None), dict(c=None), dict(o=None), dict(n=-1), dict(cands=0), dict(cands=9),
                   dict(min_votes=0), dict(max_dist=None), dict(min_flank=-1), dict(chunk=-1), dict(min_flank=1)):       # (supp is null)
            assert call(**kw) == ERR_ARG, kw
        md[1] = -1
        assert call() == ERR_ARG
        md[1] = 6
        count[1] = MAX_READ + 1
        assert call() == ERR_ARG
        count[1], first[0] = 12, -1
        assert call() == ERR_ARG
        first[0] = 0
        assert call(n=0) == 0 and call(n=0, min_flank=3) == 0                      # nothing to do: no device is looked for
        assert call() == -11 and call(min_flank=3, s=supp.ctypes.data) == -11      # arguments pass: now the device ordinal is refused
    for kw in (dict(max_dist=-1), dict(max_dist=[1, -1]), dict(max_dist=[1, 2, 3]), dict(min_flank=-1), dict(groups=[0]), dict(groups=[0, -1])):
        with pytest.raises(ValueError):
            rm.reference_map(bases, [[0, 10]], ["A" * 20, "C" * 30], **kw)


# ---------------------------------------------------------------- nested prefixes

def test_nested_prefixes():
    """a read that is the prefix of p bases between junk maps to the oligo of p bases at distance 0, where the junk ends; the
    longer prefixes are at most len - p away (the read ends, the oligo does not) and the runner-up says so; every row equals
    the plain full-matrix statement of the definition"""
    oligos, reads, front = U.nested(1024)
    bases, win = U.pack(reads)
    lens = [len(o) for o in oligos]
    res = rm.reference_map(bases, win, oligos, **U.NESTED)
    assert (res.out[:, 6] >= 1).all()
    for r, p in enumerate(lens):
        assert res.out[r, :6].tolist() == [r, r, 0, 0, front[r], p], (p, res.out[r])
        dist = [int(U.full_matrix(o, reads[r], True)[-1].min()) for o in oligos]
        assert all(m - len(reads[r]) <= d <= m - p for d, m in zip(dist[r + 1:], lens[r + 1:])) and not any(dist[:r + 1])
        # the candidates: the oligos that hold the whole prefix by their number, then the shorter ones, the longest first
        others = (list(range(r + 1, len(lens))) + list(range(r - 1, -1, -1)))[:7]
        assert res.second[r] == min(dist[o] for o in others), (p, res.out[r])
    md = np.array(lens) // 4
    for r in (0, 1, 3, 5, 8):                                                      # (the plain statement is slow: a few reads)
        assert U.plain_row(reads[r], oligos, U.NESTED["k"], U.NESTED["max_occ"], 8, 1, md) == res.out[r].tolist(), r
    # the shorter prefixes are inside the read whole: the runner-up of a read is at 0 once one is a candidate
    assert 0 < res.second[0] <= lens[1] - lens[0] and res.second[5] == 0


# ---------------------------------------------------------------- the supplementary pass

def test_the_supplementary_pass_on_constructed_reads():
    oligos, groups = U.chimeric_pool()
    reads, want, want_supp = U.chimeric_reads()
    bases, win = U.pack(reads)
    res = rm.reference_map(bases, win, oligos, min_flank=U.MIN_FLANK, groups=groups, **U.CHIM)
    U.expect(res.out, want)
    U.expect(res.supp.out, want_supp)
    chimeric = np.array([s is not None for s in want_supp])
    assert np.array_equal(res.chimeric, chimeric) and chimeric.sum() == 6
    assert res.group.tolist() == [groups[w[0]] for w in want] and res.supp.group.tolist() == [groups[s[0]] if s else -1 for s in want_supp]
    split = res.split()
    assert [s.tolist() for s in split] == [[i for i, w in enumerate(want) if groups[w[0]] == g and not chimeric[i]] for g in range(3)]
    assert [s.tolist() for s in res.split(groups, 3)] == [s.tolist() for s in split]
    # a flank of exactly min_flank bases is mapped, one base fewer is not: read 6's right flank is its second oligo
    more = rm.reference_map(bases, win, oligos, min_flank=U.MIN_FLANK + 1, groups=groups, **U.CHIM)
    assert np.array_equal(more.out, res.out) and more.supp.out[6].tolist() == U.UNMAPPED and res.supp.ref[6] >= 0
    assert np.array_equal(np.delete(more.supp.out, 6, axis=0), np.delete(res.supp.out, 6, axis=0))
    # no pass: the rows of the primary alone; every supplementary row is the flank's own mapping, moved
    none = rm.reference_map(bases, win, oligos, groups=groups, **U.CHIM)
    assert none.supp is None and np.array_equal(none.out, res.out)
    md = np.array([len(o) for o in oligos]) // 4
    for r in (0, 2, 7):
        at, n = rm.flank(int(res.start[r]), int(res.count[r]), len(reads[r]))
        row = U.plain_row(reads[r][at:at + n], oligos, 8, 64, 4, 2, md)
        row[4] += at
        assert row == res.supp.out[r].tolist(), r
    assert rm.flank(10, 5, 25) == (0, 10) and rm.flank(10, 5, 26) == (15, 11) and rm.flank(0, 9, 9) == (0, 0)


# ---------------------------------------------------------------- recovery, the definition alone

SEED = 2026


def test_the_definition_recovers_three_pools():
    """3 x 70 reads of three pools whose codes and oligo lengths differ, the channel and rates of
    tests/test_read_map_host.py's recovery test, a coin per read for the strand: every read returns to its source oligo,
    strand and group, with the defaults of the definition and the tools' min_flank; none is called chimeric"""
    p = U.simulated_pools(SEED)
    lens = sorted(set(len(o) for o in p["oligos"]))
    assert len(lens) == 3
    res = rm.reference_map(p["bases"], p["win"], p["oligos"], min_flank=lens[0] // 2, groups=p["groups"])
    assert np.array_equal(res.ref, p["source"]) and np.array_equal(res.rc, p["rc"]) and np.array_equal(res.group, p["group"])
    assert not res.chimeric.any() and p["rc"].any() and not p["rc"].all()
    assert [len(s) for s in res.split()] == [70, 70, 70]


# ---------------------------------------------------------------- declarations

def test_declarations():
    with open(os.path.join(ROOT, "include", "lva_decoder.h")) as f:
        header = f.read()
    assert "#define LVA_ABI_VERSION 5" in header
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", header, flags=re.S))
    for proto in ("int lva_map_index_create_pooled(const uint8_t *refs, const int64_t *ref_off , int32_t n_refs, int32_t k, "
                  "int32_t max_occ, lva_map_index **out);",
                  "int lva_map_reads_pooled(int32_t device, const lva_map_index *idx, const uint8_t *bases, const int64_t *first_base, "
                  "const int32_t *n_bases, int32_t n_reads, int32_t cands, int32_t min_votes, const int32_t *max_dist , int32_t min_flank, "
                  "int32_t chunk_reads, int32_t *out , int32_t *supp );"):
        assert proto in flat, proto
    assert _lib.EXPORTS[-6:-4] == ["lva_map_index_create_pooled", "lva_map_reads_pooled"] and _lib.ABI_VERSION == 5
    assert _lib.EXPORTS[-4:] == ["lva_map_index_create", "lva_map_index_destroy", "lva_map_index_info", "lva_map_reads"]
    with open(os.path.join(ROOT, "nanopore_dna_storage_amd", "csrc", "Makefile")) as f:
        make = f.read()
    assert re.search(r"^SRC\s*=.*\bmq_kernels\.hip\b", make, re.M) and re.search(r"^HDR\s*=.*\bmq_kernels\.h\b", make, re.M)
