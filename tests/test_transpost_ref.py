"""The yardsticks of the transition posteriors (tests/transpost_ref.py) against each other, against brute force and against
the list decoder's CPU oracle; and the synthetic score reads.  No GPU."""
import hashlib

import numpy as np
import pytest

import transpost_ref as T
from nanopore_dna_storage_amd import synth
from transpost_cases import CLEAN_CASES, clean_reads


def _ulp32(x):
    return float(np.spacing(np.float32(x)))


@pytest.mark.parametrize("nblk", [24, 300, 1500])
@pytest.mark.parametrize("kind", ["uniform", "read"])
def test_restatements_agree_to_float32_rounding(nblk, kind):
    """flappie's float32 order against float64.  Its forward and backward values reach M = (5 + ln 8) nblk between them
    (scores within +-5, at most 8 sources); every step rounds about four times at that magnitude (two sums, the
    difference, max + log1p) by at most half a unit each, the 40-entry normalisation 40 times more: worst case
    (2 nblk + 24) ulp(M).  The observed distance is orders of magnitude below (errors do not all add up)."""
    rng = np.random.default_rng(nblk)
    if kind == "uniform":
        x = rng.uniform(-5, 5, (nblk, 40)).astype(np.float32)
    else:
        x = synth.scores_from_bases(rng.integers(0, 4, size=nblk // 4), rng)[:nblk]
    n = x.shape[0]
    a, c = T.posteriors_f64(x), T.posteriors_flappie_f32(x)
    err = float(np.abs(a - c).max())
    bound = (2 * n + 24) * _ulp32((5 + np.log(8)) * n)
    print("nblk %d %s: |flappie_f32 - f64| = %.3g, bound %.3g" % (n, kind, err, bound))
    assert err <= bound
    assert c.dtype == np.float32 and a.dtype == np.float64


def test_f64_blocks_are_normalised():
    rng = np.random.default_rng(2)
    xs = [rng.uniform(-5, 5, (n, 40)).astype(np.float32) for n in (1, 7, 400)]
    for p in T.posteriors_f64_batch(xs):
        assert np.abs(np.logaddexp.reduce(p, axis=1)).max() < 1e-11


def test_batch_equals_single():
    rng = np.random.default_rng(3)
    xs = [rng.normal(0, 2, (n, 40)).astype(np.float32) for n in (5, 0, 9, 2)]
    for x, a, c in zip(xs, T.posteriors_f64_batch(xs), T.posteriors_flappie_f32_batch(xs)):
        assert a.shape == x.shape and c.shape == x.shape
        if len(x):
            assert np.array_equal(a, T.posteriors_f64(x)) and np.array_equal(c, T.posteriors_flappie_f32(x))


def test_three_blocks_equal_brute_force():
    """every state sequence of a 3-block example enumerated: 8^4 sequences, of which the flip-flop graph allows 8 * 5^3"""
    x = np.random.default_rng(4).normal(0, 2, (3, 40)).astype(np.float32)
    want = T.brute_force(x)
    assert np.abs(T.posteriors_f64(x) - want).max() < 1e-12
    assert np.abs(T.posteriors_flappie_f32(x) - want).max() < 1e-5


def _scaled_worst(nblk, spread, largest):
    return (2 * nblk + 24) * _ulp32(2 * (2 * spread + 2 * np.log(8)) + largest)


def _scaled_case(nblk, reads):
    rng = np.random.default_rng(900 + nblk)
    xs = [rng.uniform(-5, 5, (nblk, 40)).astype(np.float32) for _ in range(reads)]
    a, c = T.posteriors_f64_batch(xs), T.posteriors_scaled_f32_batch(xs)
    assert all(y.dtype == np.float32 and y.shape == x.shape for x, y in zip(xs, c))
    return max(float(np.abs(y.astype(np.float64) - z).max()) for y, z in zip(c, a))


def test_scaled_f32_stays_at_float32_rounding_at_every_length():
    """The rescaled float32 order against float64 at 1, 3, 33, 400 and 3000 blocks of uniform +-5 scores.  With scores of
    spread D, every flip entry of a new vector lies within D + ln 8 of the largest (all eight states lead into every flip, and
    every state leads into all four flips); a flop entry is reached from one flip and itself, so it lies at most one more
    step's D + ln 8 and D below.  A rescaled vector therefore stays within [-(2 D + 2 ln 8), 0] at any length, and a
    posterior candidate -- forward + backward + score -- below M = 2 (2 D + 2 ln 8) + max |score|.  Every step rounds about
    four times at that magnitude, the 40-entry normalisation 40 times more: the worst case of the flappie test with M
    constant.  That bound still counts every step's rounding as if all added up; what rescaling is for is that they do not:
    the error of 3000 blocks is held to twice that of 33."""
    sizes = {1: 512, 3: 256, 33: 256, 400: 32, 3000: 8}
    err = {n: _scaled_case(n, r) for n, r in sizes.items()}
    for n, e in err.items():
        bound = _scaled_worst(n, 10, 5)
        print("nblk %d: |scaled_f32 - f64| = %.3g, worst case %.3g" % (n, e, bound))
        assert e <= bound
    assert err[3000] <= 2 * err[33]


@pytest.mark.parametrize("nblk", [1, 2, 3])
def test_scaled_f32_equals_brute_force(nblk):
    """every state sequence enumerated; the float32 distance within the worst case of the test above for these scores"""
    x = np.random.default_rng(40 + nblk).normal(0, 2, (nblk, 40)).astype(np.float32)
    want = T.brute_force(x)
    assert np.abs(T.posteriors_f64(x) - want).max() < 1e-12
    bound = _scaled_worst(nblk, float(x.max() - x.min()), float(np.abs(x).max()))
    got = T.posteriors_scaled_f32(x)
    assert got.dtype == np.float32 and np.abs(got - want).max() <= bound


def test_scaled_f32_batch_equals_single():
    rng = np.random.default_rng(31)
    xs = [rng.normal(0, 2, (n, 40)).astype(np.float32) for n in (5, 0, 9, 1, 34, 2, 0)]
    got = T.posteriors_scaled_f32_batch(xs)
    for x, c in zip(xs, got):
        assert c.shape == x.shape and c.dtype == np.float32
        if len(x):
            assert np.array_equal(c, T.posteriors_scaled_f32(x))
    assert T.posteriors_scaled_f32_batch([]) == []


def test_argmax_follows_the_true_path():
    for seed in (1, 2, 3):
        x = synth.make_read_scores(6, 1, 60, seed, margin=6.0)
        p = T.posteriors_f64(x["scores"])
        assert x["scores"].dtype == np.float32 and np.abs(x["scores"]).max() <= synth.SCORE_CLIP
        assert np.array_equal(p.argmax(axis=1), x["true_idx"])


@pytest.mark.parametrize("case", CLEAN_CASES, ids=lambda c: "m%d" % c["mem_conv"])
def test_oracle_decodes_the_clean_seeds(case, oracle):
    """the reads of tests/test_gpu_scores_chain.py: 'clean' = the float32 cast of posteriors_f64"""
    for x in clean_reads(case):
        post = T.posteriors_f64(x["scores"]).astype(np.float32)
        msgs, _ = oracle.OracleCode(case["mem_conv"], case["rate"], case["msg_len"], rc=x["rc"]).decode(
            post, case["list_size"], case["max_deviation"])
        assert np.array_equal(msgs[0], x["msg"]), x["seed"]


def _digest(d):
    m = hashlib.sha256()
    for k in sorted(d):
        v = d[k]
        if isinstance(v, np.ndarray):
            m.update(k.encode()); m.update(str(v.dtype).encode()); m.update(str(v.shape).encode())
            m.update(np.ascontiguousarray(v).tobytes())
        else:
            m.update(("%s=%r" % (k, v)).encode())
    return m.hexdigest()[:16]


SB, EB = "CACCTGTGCTGCGTCAGGCTGTGTC", "GCTGTCCGTTCCGCATTGACACGGC"


@pytest.mark.parametrize("kw,want", [
    (dict(mem_conv=6, rate=1, msg_len=60, seed=11), "dd6b995c112cf6ef"),
    (dict(mem_conv=8, rate=3, msg_len=164, seed=7, rc=True, margin=4.3, sub=0.01, dele=0.01, ins=0.005), "639e5ec4b97fa1a1"),
    (dict(mem_conv=6, rate=1, msg_len=60, seed=3, quantum=0.5), "d518ea3b06db78a5"),
])
def test_make_read_is_unchanged(kw, want):
    """digests taken before the score makers existed: the posterior makers draw the random numbers they always drew"""
    assert _digest(synth.make_read(**kw)) == want


@pytest.mark.parametrize("kw,want", [
    (dict(mem_conv=6, rate=1, msg_len=60, seed=5, rc=True, flank=(5, 12)), "7bd0c6ab81f2b476"),
    (dict(mem_conv=8, rate=3, msg_len=164, seed=21, sub=0.004, dele=0.0085, ins=0.0005), "83ce021f82eb704d"),
])
def test_make_barcoded_read_is_unchanged(kw, want):
    assert _digest(synth.make_barcoded_read(start_barcode=SB, end_barcode=EB, **kw)) == want


def test_barcoded_score_read_has_the_strand_of_the_posterior_read():
    a = synth.make_barcoded_read(6, 1, 60, 5, SB, EB, rc=True, flank=(5, 12))
    b = synth.make_barcoded_read_scores(6, 1, 60, 5, SB, EB, rc=True, flank=(5, 12))
    assert np.array_equal(a["strand"], b["strand"]) and a["post"].shape == b["scores"].shape
