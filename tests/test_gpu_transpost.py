"""Transition posteriors on the device (lva_transpost_batch*, csrc/tp_kernels.hip) against the yardsticks of
tests/transpost_ref.py, and what the entry points promise about batches, non-finite input, limits and an open stream.

Accuracy.  For a set S of reads, E(S) is the largest |value - float64 value| over all entries of all reads of S.  Two float32
yardsticks are computed here, from their own arithmetic on the same inputs: E_ref from flappie's unscaled order
(posteriors_flappie_f32), E_scaled from the same order with per-step rescaling (posteriors_scaled_f32).
  (A)  E_gpu(S) <= 2 E_ref(S)      (device expf / logf are specified to about twice glibc's error)
  (B)  E_gpu(S) <= 2 E_scaled(S)   (the same margin for the same reason)
and with either the float64 log-sum-exp of every output block of S within the same bound of 0.  E_ref grows with the read
(about 1e-3 at 400 blocks, 7e-3 at 3000), E_scaled does not (about 4e-6), so (A) is applied per length class to short reads,
from 1 block up, where it is tight, and (B) to everything of 16 blocks and more.  No absolute figure is written into a test:
every test prints E_gpu, E_ref and E_scaled (figures: DESIGN.md section 4).

Shapes.  Both kernels run a pipeline of 4-block chunks (the forward kernel two per trip) with clamped block indices, as
long as any of a wavefront's 8 reads has blocks: every length 1..20 and both sides of 24 and 32, wavefronts that hold a
1500-block read beside empty, 1-block and other short reads with the long one in each of the 8 positions, partial last
wavefronts, in place / out of place / host call at lengths below two chunks, scores far outside +-5, a forward scratch
buffer that grows and is used again."""
import ctypes

import numpy as np
import pytest

import nanopore_dna_storage_amd as pkg
from nanopore_dna_storage_amd import _lib, synth
import transpost_ref as T

pytestmark = pytest.mark.gpu

ERR_ARG = -10


@pytest.fixture(scope="module")
def dec():
    with pkg.Decoder(6, 1, 60, list_size=4, max_deviation=20, max_slots=4) as d:
        yield d


def _family(kind, n=64):
    rng = np.random.default_rng(77 if kind == "uniform" else 78)
    if kind == "uniform":
        return [rng.uniform(-synth.SCORE_CLIP, synth.SCORE_CLIP, (int(k), 40)).astype(np.float32) for k in rng.integers(200, 3001, n)]
    out = []
    for i in range(n):                      # m=8 r=3/4 msg_len 164 reads are about 500 blocks; dele/ins vary the length
        out.append(synth.make_read_scores(8, 3, 164, 5000 + i, rc=bool(i & 1), margin=4.5, sub=0.01, dele=0.01, ins=0.01)["scores"])
    return out


def _errors(got, scores):
    a = T.posteriors_f64_batch(scores)
    c = T.posteriors_flappie_f32_batch(scores)
    e_gpu = max(float(np.abs(g.astype(np.float64) - x).max()) for g, x in zip(got, a))
    e_ref = max(float(np.abs(y.astype(np.float64) - x).max()) for y, x in zip(c, a))
    lse = max(float(np.abs(np.logaddexp.reduce(g.astype(np.float64), axis=1)).max()) for g in got)
    return e_gpu, e_ref, lse


class Yard:
    """float64 values and the two float32 yardsticks of a list of reads, computed once"""

    def __init__(self, scores):
        self.f64 = T.posteriors_f64_batch(scores)
        self.ref = T.posteriors_flappie_f32_batch(scores)
        self.scaled = T.posteriors_scaled_f32_batch(scores)

    def err(self, ys, sel):
        return max(float(np.abs(ys[i].astype(np.float64) - self.f64[i]).max()) for i in sel if len(self.f64[i]))


def _lse(got, sel):
    return max(float(np.abs(np.logaddexp.reduce(got[i].astype(np.float64), axis=1)).max()) for i in sel if len(got[i]))


def _hold(name, got, yard, sel=None, a=False, b=False):
    """print E_gpu, E_ref, E_scaled of the reads `sel` and hold E_gpu and the block sums to criterion (A) and / or (B)"""
    sel = list(range(len(got))) if sel is None else list(sel)
    assert a or b
    assert all(got[i].dtype == np.float32 and got[i].shape == yard.f64[i].shape for i in sel)
    e_gpu, lse = yard.err(got, sel), _lse(got, sel)
    e_ref = yard.err(yard.ref, sel)
    e_scaled = yard.err(yard.scaled, sel)
    print("%s: E_gpu = %.3g, E_ref = %.3g, E_scaled = %.3g, max |logsumexp| = %.3g" % (name, e_gpu, e_ref, e_scaled, lse))
    if a:
        assert e_gpu <= 2 * e_ref, (name, "A", e_gpu, e_ref)
        assert lse <= 2 * e_ref, (name, "A", lse, e_ref)
    if b:
        assert e_gpu <= 2 * e_scaled, (name, "B", e_gpu, e_scaled)
        assert lse <= 2 * e_scaled, (name, "B", lse, e_scaled)


def _by_length(scores):
    cls = {}
    for i, x in enumerate(scores):
        cls.setdefault(len(x), []).append(i)
    return cls


def _same(xs, ys):
    return len(xs) == len(ys) and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(xs, ys))


@pytest.mark.parametrize("kind", ["reads", "uniform"])
def test_accuracy_against_float64(dec, kind):
    scores = _family(kind)
    assert len(scores) >= 64 and all(200 <= len(s) <= 3000 for s in scores)
    got = dec.posteriors(scores)
    _hold(kind, got, Yard(scores), a=True, b=True)


def test_accuracy_on_a_read_of_200000_blocks(dec):
    """held to (A) alone: a third pass of 200 000 numpy steps is not worth its time; the 20 000-block read below has (B)"""
    scores = [np.random.default_rng(79).uniform(-synth.SCORE_CLIP, synth.SCORE_CLIP, (200000, 40)).astype(np.float32)]
    got = dec.posteriors(scores)
    e_gpu, e_ref, lse = _errors(got, scores)
    print("200000 blocks: E_gpu = %.3g, E_ref = %.3g, max |logsumexp| = %.3g" % (e_gpu, e_ref, lse))
    assert e_gpu <= 2 * e_ref
    assert lse <= 2 * e_ref


def test_the_error_stays_flat_to_20000_blocks(dec):
    scores = [np.random.default_rng(80).uniform(-synth.SCORE_CLIP, synth.SCORE_CLIP, (20000, 40)).astype(np.float32)]
    _hold("20000 blocks", dec.posteriors(scores), Yard(scores), a=True, b=True)


# ---- every short length ----------------------------------------------------------------------------------------------
SHORT_LENGTHS = list(range(1, 21)) + [23, 24, 25, 31, 32, 33]      # every residue of the 4-block chunk and the 8-block trip


class _Short:
    scores = yard = None


def _short():
    """64 reads of every short length, shuffled so that every 8-read wavefront mixes lengths; yardsticks computed once"""
    if _Short.scores is None:
        rng = np.random.default_rng(81)
        xs = [rng.uniform(-synth.SCORE_CLIP, synth.SCORE_CLIP, (n, 40)).astype(np.float32) for n in SHORT_LENGTHS for _ in range(64)]
        xs = [xs[i] for i in np.random.default_rng(82).permutation(len(xs))]
        assert all(len({len(x) for x in xs[g:g + 8]}) > 1 for g in range(0, len(xs), 8))
        _Short.scores, _Short.yard = xs, Yard(xs)
    return _Short.scores, _Short.yard


def test_every_short_length(dec):
    scores, yard = _short()
    assert synth.SCORE_CLIP == 5.0
    got = dec.posteriors(scores)
    cls = _by_length(scores)
    assert sorted(cls) == SHORT_LENGTHS and all(len(v) == 64 for v in cls.values())
    failed = []
    for n in SHORT_LENGTHS:
        try:
            _hold("%d blocks" % n, got, yard, cls[n], a=True, b=n >= 16)
        except AssertionError as e:
            failed.append(e.args[0])
    assert not failed, failed


def test_short_reads_in_place_out_of_place_and_host_call(dec):
    """below 8 blocks every prefetch of the backward kernel is clamped to block 0 of a buffer it is about to overwrite"""
    scores, _ = _short()
    host = dec.posteriors(scores)
    dev, off = dec.upload(scores)
    out = dec.alloc(int(off[-1]) * 160)
    try:
        dec.posteriors_resident(dev, off, out_ptr=out)
        oop = dec.download(out, off)
        assert _same(dec.download(dev, off), scores), "out of place changed its input"
        dec.posteriors_resident(dev, off)
        inp = dec.download(dev, off)
    finally:
        dec.free(dev)
        dec.free(out)
    bad = sorted({len(h) for h, o, i in zip(host, oop, inp) if not (np.array_equal(h, o) and np.array_equal(h, i))})
    assert not bad, "lengths that differ between host call, out of place and in place: %r" % bad


# ---- ragged wavefronts -----------------------------------------------------------------------------------------------
RAGGED_SHORT = (0, 1, 2, 3, 4, 5, 9)


def _ragged_pool():
    """two reads of 1500 blocks and two of each short length but the empty one: 15 distinct reads"""
    rng = np.random.default_rng(83)
    pool = {("long", v): rng.uniform(-5, 5, (1500, 40)).astype(np.float32) for v in (0, 1)}
    for n in RAGGED_SHORT:
        for v in (0, 1):
            pool[(n, v)] = rng.uniform(-5, 5, (n, 40)).astype(np.float32) if n else np.zeros((0, 40), np.float32)
    return pool


def _ragged_batch(n_reads, rot):
    """keys of a batch: wavefront g holds the long read at position (g + rot) % 8 and the seven short ones around it"""
    keys = []
    for g in range((n_reads + 7) // 8):
        short = [(n, g & 1) for n in RAGGED_SHORT]
        pos = (g + rot) % 8
        keys += short[:pos] + [("long", (g >> 1) & 1)] + short[pos:]
    return keys[:n_reads]


def test_ragged_wavefronts(dec):
    pool = _ragged_pool()
    names = list(pool)
    alone = {k: dec.posteriors([pool[k]])[0] for k in names}          # one call per distinct read
    assert all(alone[k].shape == pool[k].shape for k in names)
    wrong = []
    seen = set()
    for n_reads in (1, 7, 8, 9, 63, 65):
        for rot in range(8):
            keys = _ragged_batch(n_reads, rot)
            assert len(keys) == n_reads
            seen |= {(i % 8, k[0]) for i, k in enumerate(keys)}
            got = dec.posteriors([pool[k] for k in keys])
            wrong += [(n_reads, rot, i, k) for i, k in enumerate(keys) if not _same([got[i]], [alone[k]])]
    assert {(i, "long") for i in range(8)} <= seen
    # first and last read empty, the second wavefront holds a long read and an empty one only
    keys = [(0, 0), ("long", 0), (1, 0), (2, 0), (3, 1), (4, 0), (5, 1), (9, 0), ("long", 1), (0, 1)]
    got = dec.posteriors([pool[k] for k in keys])
    wrong += [("empty ends", 0, i, k) for i, k in enumerate(keys) if not _same([got[i]], [alone[k]])]
    assert not wrong, "reads that differ from the same read decoded alone (batch, rotation, position, read): %r" % wrong[:20]
    # accuracy of the reads themselves (bit-equal wherever they stood)
    scores = [pool[k] for k in names]
    res = [alone[k] for k in names]
    yard = Yard(scores)
    for n, sel in sorted(_by_length(scores).items()):
        if n:
            _hold("ragged, %d blocks" % n, res, yard, sel, a=True, b=n == 1500)


# ---- scores outside +-5 ----------------------------------------------------------------------------------------------
def _wide_family(kind):
    rng = np.random.default_rng(84 if kind == "wide" else 85)
    out = []
    for n in ((3, 8, 17, 33, 400) if kind == "wide" else (3, 8, 17, 33)):
        for _ in range(64):
            if kind == "wide":                 # expf underflows, posteriors go down to about -150
                x = np.clip(rng.normal(0, 12, (n, 40)), -40, 40)
            else:                              # one constant per block: mathematically the same posteriors
                x = rng.uniform(-5, 5, (n, 40)) + rng.uniform(-1000, 1000, (n, 1))
            out.append(x.astype(np.float32))
    return out


@pytest.mark.parametrize("kind", ["wide", "shifted"])
def test_scores_outside_the_usual_range(dec, kind):
    scores = _wide_family(kind)
    got = dec.posteriors(scores)
    assert all(np.isfinite(g).all() for g in got)
    yard = Yard(scores)
    failed = []
    for n, sel in sorted(_by_length(scores).items()):
        assert len(sel) == 64
        try:
            _hold("%s, %d blocks" % (kind, n), got, yard, sel, a=True, b=kind == "wide" and n >= 33)
        except AssertionError as e:
            failed.append(e.args[0])
    assert not failed, failed


# ---- the forward scratch buffer --------------------------------------------------------------------------------------
def test_the_forward_scratch_grows_and_is_used_again():
    rng = np.random.default_rng(86)
    small = [rng.uniform(-5, 5, (int(n), 40)).astype(np.float32) for n in (3, 40, 1, 17, 0, 64, 9, 33, 5, 120)]
    big = [rng.uniform(-5, 5, (50000, 40)).astype(np.float32)]
    with pkg.Decoder(6, 1, 60, list_size=4, max_deviation=20, max_slots=4) as d:
        first = d.posteriors(small)
        long_ = d.posteriors(big)
        third = d.posteriors(small)
    assert _same(first, third)
    _hold("scratch, 10 short reads", first, Yard(small), a=True)
    _hold("scratch, 50000 blocks", long_, Yard(big), a=True, b=True)


def _batch100(seed=5):
    rng = np.random.default_rng(seed)
    return [rng.uniform(-5, 5, (int(k), 40)).astype(np.float32) for k in rng.integers(20, 700, 100)]


def test_a_read_does_not_depend_on_the_batch(dec):
    batch = _batch100()
    probe = np.random.default_rng(6).normal(0, 2.5, (613, 40)).astype(np.float32)
    alone = dec.posteriors([probe])[0]
    assert np.isfinite(alone).all()
    for pos in (0, 50, 99):
        b = list(batch)
        b[pos] = probe
        assert np.array_equal(dec.posteriors(b)[pos], alone), pos
    # host call, device call out of place, device call in place
    b = list(batch)
    b[50] = probe
    host = dec.posteriors(b)
    dev, off = dec.upload(b)
    out = dec.alloc(int(off[-1]) * 160)
    try:
        dec.posteriors_resident(dev, off, out_ptr=out)
        oop = dec.download(out, off)
        assert all(np.array_equal(x, y) for x, y in zip(dec.download(dev, off), b)), "out of place changed its input"
        dec.posteriors_resident(dev, off)
        inp = dec.download(dev, off)
    finally:
        dec.free(dev)
        dec.free(out)
    for h, o, i in zip(host, oop, inp):
        assert np.array_equal(h, o) and np.array_equal(h, i)


def test_non_finite_reads_stay_alone(dec):
    batch = _batch100(8)[:40]
    want = dec.posteriors(batch)
    nan_read = batch[3].copy()
    nan_read[7, 11] = np.nan
    inf_read = batch[4].copy()
    inf_read[0, 33] = np.inf
    b = batch[:10] + [nan_read] + batch[10:25] + [inf_read] + batch[25:]
    got = dec.posteriors(b)          # LVA_OK, or it would raise
    rest = got[:10] + got[11:26] + got[27:]
    assert len(rest) == len(want) and all(np.array_equal(x, y) for x, y in zip(rest, want))


def test_empty_batches_and_empty_reads(dec):
    assert dec.posteriors([]) == []
    L = _lib.load_library()
    off = np.zeros(1, np.int64)
    assert L.lva_transpost_batch(dec._h, None, off.ctypes.data, 0, None) == 0
    assert L.lva_transpost_batch_device(dec._h, None, off.ctypes.data, 0, None) == 0
    a, b = _batch100(9)[:2]
    empty = np.zeros((0, 40), np.float32)
    got = dec.posteriors([empty, a, empty, empty, b, empty])
    assert [g.shape[0] for g in got] == [0, len(a), 0, 0, len(b), 0]
    want = dec.posteriors([a, b])
    assert np.array_equal(got[1], want[0]) and np.array_equal(got[4], want[1])
    assert [g.shape for g in dec.posteriors([empty, empty])] == [(0, 40), (0, 40)]


def test_limits_come_from_the_offsets(dec):
    """a read above 2^20 blocks: LVA_ERR_ARG before anything is read or allocated (the pointers are not even valid)"""
    L = _lib.load_library()
    off = np.array([0, 10, 10 + (1 << 20) + 1], np.int64)
    bogus = ctypes.c_void_p(16)
    assert L.lva_transpost_batch(dec._h, bogus, off.ctypes.data, 2, bogus) == ERR_ARG
    assert L.lva_transpost_batch_device(dec._h, bogus, off.ctypes.data, 2, bogus) == ERR_ARG
    off = np.array([0] + [(1 << 20) * (i + 1) for i in range(2048)], np.int64)           # 2^31 blocks in all
    assert L.lva_transpost_batch_device(dec._h, bogus, off.ctypes.data, 2048, bogus) == ERR_ARG
    off = np.array([0, 5, 3], np.int64)                                                  # not ascending
    assert L.lva_transpost_batch(dec._h, bogus, off.ctypes.data, 2, bogus) == ERR_ARG
    # exactly 2^20 blocks is legal
    x = np.zeros((1 << 20, 40), np.float32)
    got = dec.posteriors([x])[0]
    assert np.abs(np.logaddexp.reduce(got[:1000].astype(np.float64), axis=1)).max() < 1e-5


def test_busy_while_a_stream_is_open(dec):
    x = _batch100(10)[0]
    with dec.stream():
        with pytest.raises(pkg.LvaError) as e:
            dec.posteriors([x])
        assert e.value.code == _lib.ERR_BUSY
        dev = dec.alloc(x.nbytes)
        try:
            with pytest.raises(pkg.LvaError) as e:
                dec.posteriors_resident(dev, np.array([0, len(x)], np.int64))
            assert e.value.code == _lib.ERR_BUSY
        finally:
            dec.free(dev)
    assert dec.posteriors([x])[0].shape == x.shape
