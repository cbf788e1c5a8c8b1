"""Transition posteriors on the device (lva_transpost_batch*, csrc/tp_kernels.hip) against the yardsticks of
tests/transpost_ref.py, and what the entry points promise about batches, non-finite input, limits and an open stream.

Accuracy: per input family E_gpu = max |gpu - f64| and E_ref = max |flappie_f32 - f64| over all entries of all reads;
required E_gpu <= 2 E_ref (device expf / logf are specified to about twice glibc's error), and the float64 log-sum-exp of
every output block within the same bound of 0.  E_ref is computed here from the reference's own arithmetic on the same
inputs.  The kernels keep forward and backward values small, so they come in far under it (figures: DESIGN.md section 4)."""
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


@pytest.mark.parametrize("kind", ["reads", "uniform"])
def test_accuracy_against_float64(dec, kind):
    scores = _family(kind)
    assert len(scores) >= 64 and all(200 <= len(s) <= 3000 for s in scores)
    got = dec.posteriors(scores)
    assert all(g.dtype == np.float32 and g.shape == s.shape for g, s in zip(got, scores))
    e_gpu, e_ref, lse = _errors(got, scores)
    print("%s: E_gpu = %.3g, E_ref = %.3g, max |logsumexp| = %.3g" % (kind, e_gpu, e_ref, lse))
    assert e_gpu <= 2 * e_ref
    assert lse <= 2 * e_ref


def test_accuracy_on_a_read_of_200000_blocks(dec):
    scores = [np.random.default_rng(79).uniform(-synth.SCORE_CLIP, synth.SCORE_CLIP, (200000, 40)).astype(np.float32)]
    got = dec.posteriors(scores)
    e_gpu, e_ref, lse = _errors(got, scores)
    print("200000 blocks: E_gpu = %.3g, E_ref = %.3g, max |logsumexp| = %.3g" % (e_gpu, e_ref, lse))
    assert e_gpu <= 2 * e_ref
    assert lse <= 2 * e_ref


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
