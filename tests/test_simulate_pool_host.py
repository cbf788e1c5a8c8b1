"""The pool source of the read simulator's definition (simulate.reference_reads(pool=...), stream 6), without a GPU: which
word picks the pool entry and the orientation, that a pool changes nothing but the message and the orientation of a read, and
that a call without a pool is what it was."""
import numpy as np
import pytest

import nanopore_dna_storage_amd as pkg
from nanopore_dna_storage_amd import simulate as S
from nanopore_dna_storage_amd.philox import STREAM_SOURCE, philox

CODE = (6, 1, 60)
SEED = 77
N = 4096
HEAVY = dict(sub=0.1, dele=0.1, ins=0.1)


def _pool(n_pool, seed=1):
    return np.random.default_rng(seed).integers(0, 2, size=(n_pool, CODE[2]), dtype=np.uint8)


def _words(n, seed=SEED, first_read=0):
    """stream 6 by the counter the issue states, (0, 0, R, 6), one Philox call per read"""
    assert STREAM_SOURCE == 6
    return np.stack([philox(0, 0, first_read + r, 6, seed) for r in range(n)]).astype(np.uint64)


def test_the_source_is_mulhi_of_word_0_or_the_first_entry_above_it():
    W = _words(64, first_read=5)
    for n_pool in (1, 3, 65, 1 << 24):
        want = [(int(w) * n_pool) >> 32 for w in W[:, 0]]                     # mulhi by hand, in Python integers
        got, _ = S.pool_draws(64, SEED, 5, n_pool)
        assert got.dtype == np.int32 and got.tolist() == want
    cdf = np.array([1 << 30, 1 << 30, 3 << 30, 0xFFFFFFFF], np.uint32)       # entry 1 equals its predecessor
    want = [next((k for k in range(4) if int(w) < int(cdf[k])), 3) for w in W[:, 0]]
    got, _ = S.pool_draws(64, SEED, 5, 4, cdf)
    assert got.tolist() == want and 1 not in want and len(set(want)) == 3
    ref = S.reference_reads(*CODE, 64, SEED, first_read=5, scores=False, pool=_pool(4), pool_cdf=cdf)
    assert ref["source"].tolist() == want and ref["source"].dtype == np.int32 and ref["rc"].dtype == np.uint8


def test_a_word_at_or_above_every_entry_takes_the_last():
    """`else n_pool - 1`: the definition's search, on words chosen by hand instead of drawn"""
    cdf = np.array([10, 10, 20, 0xFFFFFFFF], np.uint32)
    for w, k in ((0, 0), (9, 0), (10, 2), (19, 2), (20, 3), (0xFFFFFFFE, 3), (0xFFFFFFFF, 3)):
        assert min(int(np.searchsorted(cdf, np.uint32(w), side="right")), 3) == k
        assert next((j for j in range(4) if w < int(cdf[j])), 3) == k


def test_one_entry_pools_and_a_table_that_leaves_one_entry():
    assert not S.pool_draws(N, SEED, 0, 1)[0].any()
    ref = S.reference_reads(*CODE, 50, SEED, scores=False, pool=_pool(1))
    assert not ref["source"].any() and (ref["msgs"] == _pool(1)[0]).all()
    src, _ = S.pool_draws(N, SEED, 0, 2, np.array([0, 0xFFFFFFFF], np.uint32))
    assert (src == 1).all()


def test_an_entry_equal_to_its_predecessor_is_never_drawn():
    cdf = S.weights_to_cdf([2, 0, 1, 0, 1])
    assert cdf[1] == cdf[0] and cdf[3] == cdf[2]
    src, _ = S.pool_draws(N, SEED, 0, 5, cdf)
    assert set(src.tolist()) == {0, 2, 4}


def test_uniform_sources_stay_in_a_sanity_band():
    """a band on one fixed seed, not a statistical claim"""
    counts = np.bincount(S.pool_draws(N, SEED, 0, 3)[0], minlength=3)
    print("counts over 3 entries:", counts)
    assert counts.sum() == N and (counts >= N / 4).all() and (counts <= N * 5 / 12).all()


def test_the_coin_is_the_top_bit_of_word_1():
    W = _words(256)
    for mode, want in ((0, np.zeros(256)), (1, np.ones(256)), (2, np.arange(256) & 1), (3, W[:, 1] >> np.uint64(31))):
        assert np.array_equal(S.pool_draws(256, SEED, 0, 3, rc_mode=mode)[1], want.astype(np.uint8)), mode
    coin = S.pool_draws(256, SEED, 0, 3, rc_mode=3)[1]
    assert 64 < int(coin.sum()) < 192                                          # both orientations
    ref = S.reference_reads(*CODE, 256, SEED, scores=False, pool=_pool(3), rc_mode=3)
    assert np.array_equal(ref["rc"], coin)
    with pytest.raises(ValueError):
        S.reference_reads(*CODE, 2, SEED, scores=False, pool=_pool(3), rc_mode=4)


def test_a_clean_read_is_its_pool_entry_encoded():
    pool = _pool(5)
    pool[0], pool[4] = 0, 1                                                    # an all-zero and an all-one message
    ref = S.reference_reads(*CODE, 40, SEED, scores=False, pool=pool, rc_mode=3)
    assert np.array_equal(ref["msgs"], pool[ref["source"]]) and ref["rc"].min() == 0 and ref["rc"].max() == 1
    assert {0, 4} <= set(ref["source"].tolist())
    oligos = pkg.encode(*CODE, pool)
    off = ref["base_offsets"]
    for r in range(40):
        want = oligos[ref["source"][r]]
        want = (3 - want)[::-1] if ref["rc"][r] else want
        assert np.array_equal(ref["bases"][off[r]:off[r + 1]], want), r


def test_a_pool_read_keeps_the_channel_events_of_its_number():
    """Deletions, insertions and substitutions are decided by (read number, position) in stream 1, the dwell by (read number,
    emitted base) in stream 2: a pool read emits as many bases and as many blocks as today's read of the same number, and the
    positions that differ from its clean strand are the positions at which today's read differs from its own."""
    kw = dict(scores=False, **HEAVY)
    pool = _pool(7)
    plain, clean_plain = S.reference_reads(*CODE, 48, SEED, **kw), S.reference_reads(*CODE, 48, SEED, scores=False)
    pooled, clean_pooled = S.reference_reads(*CODE, 48, SEED, pool=pool, **kw), S.reference_reads(*CODE, 48, SEED, scores=False, pool=pool)
    assert np.array_equal(plain["base_offsets"], pooled["base_offsets"])       # same deletions and insertions in number
    assert np.array_equal(plain["row_offsets"], pooled["row_offsets"])         # equal dwell counts
    assert not np.array_equal(plain["msgs"], pooled["msgs"])
    # per read: the places of deletions and insertions, from the channel's own draws (stream 1), must explain both reads
    q = S.parameters(**HEAVY)
    n = pkg.code_info(*CODE).oligo_len
    for r in range(48):
        i = np.arange(n + 1)
        A, B = philox(i, 0, r, 1, SEED), philox(i, 1, r, 1, SEED)
        n_ins = np.cumprod(A < q["ins"], axis=1).sum(axis=1)
        kept = (B[:, 1] >= q["dele"]) & (i < n)
        for ref, clean in ((plain, clean_plain), (pooled, clean_pooled)):
            strand = clean["bases"][clean["base_offsets"][r]:clean["base_offsets"][r + 1]]
            got = ref["bases"][ref["base_offsets"][r]:ref["base_offsets"][r + 1]]
            assert len(got) == int(n_ins.sum() + kept.sum())
            at = np.cumsum(n_ins + kept) - kept                                # where position i's own base landed
            own = got[at[:n][kept[:n]]]
            sub = B[:n, 2][kept[:n]] < q["sub"]
            assert np.array_equal(own[~sub], strand[kept[:n]][~sub]) and (own[sub] != strand[kept[:n]][sub]).all()


def test_without_a_pool_nothing_changes():
    kw = dict(first_read=2, start_barcode="ACGTAC", end_barcode="TTGCA", flank=(3, 9), rc_mode=2, **HEAVY)
    before = S.reference_reads(*CODE, 12, SEED, **kw)                          # before any pool argument is touched
    S.reference_reads(*CODE, 12, SEED, pool=_pool(3), rc_mode=3, **{k: v for k, v in kw.items() if k != "rc_mode"})
    after = S.reference_reads(*CODE, 12, SEED, pool=None, pool_cdf=None, **kw)
    assert sorted(before) == sorted(after) == ["base_offsets", "bases", "msgs", "row_offsets", "scores", "true_idx"]
    for key in before:
        assert before[key].dtype == after[key].dtype and np.array_equal(before[key], after[key]), key
    with pytest.raises(ValueError):
        S.reference_reads(*CODE, 2, SEED, pool_cdf=np.array([0xFFFFFFFF], np.uint32))


def test_parameters_still_refuses_the_coin():
    with pytest.raises(ValueError):
        S.parameters(rc_mode=3)
    with pytest.raises(ValueError):
        S.reference_reads(*CODE, 2, SEED, rc_mode=3)


def test_weights_to_cdf():
    cdf = S.weights_to_cdf([1, 0, 3])
    assert cdf.dtype == np.uint32 and cdf.tolist() == [1 << 30, 1 << 30, 0xFFFFFFFF]
    assert S.weights_to_cdf([5]).tolist() == [0xFFFFFFFF]
    assert S.weights_to_cdf([1, 1, 1]).tolist() == [0x55555555, 0xAAAAAAAA, 0xFFFFFFFF]
    for bad in ([], [0, 0], [1, -1], [1, float("nan")], [[1, 2]]):
        with pytest.raises(ValueError):
            S.weights_to_cdf(bad)


def test_pools_that_are_refused():
    ok = _pool(3)
    for pool, cdf in ((ok[:, :59], None), (ok[:0], None), (ok + 1, None), (ok, np.array([5, 4, 0xFFFFFFFF], np.uint32)),
                      (ok, np.array([1, 2, 3], np.uint32)), (ok, np.array([1, 0xFFFFFFFF], np.uint32))):
        with pytest.raises(ValueError):
            S.reference_reads(*CODE, 2, SEED, scores=False, pool=pool, pool_cdf=cdf)
