"""The three kernels of the one-message trellis are one frame (csrc/sc_frame.h) under three cell rules: sc_score, st_fill and
fw_forward.  What a shared frame could newly get wrong is a rule's hook reaching another kernel -- the forward score's cleared
band in the score, the trace's winner bookkeeping in either -- so on ONE set of pairs, through one decoder: score_bases and
the scores of trace_bases are the same bits, both are trellis_score.reference_score's, forward_bases lies within the bound of
tests/test_gpu_trellis_forward.py (its _bound, no other tolerance) of reference_forward, and score_bases after the two others
returns what it returned before them.  Sequences of 1, 2, 63, 64, 65 and 128 bases (one and two passes of 64 positions) in
windows of len + 2 and len + 2 + 16 blocks (within and across a staged chunk), a band of 4 -- narrower than a pass, so cells
leave and re-enter it: the score reads them stale, the forward score cleared -- and no band."""
import functools

import numpy as np
import pytest

import nanopore_dna_storage_amd as pkg
from nanopore_dna_storage_amd import trellis_score as T
from test_gpu_trellis_forward import _bound
from trellis_forward_cases import OFF, err

pytestmark = pytest.mark.gpu

LENGTHS = (1, 2, 63, 64, 65, 128)


def same_bits(a, b):
    return np.asarray(a, np.float32).tobytes() == np.asarray(b, np.float32).tobytes()


@functools.lru_cache(maxsize=None)
def reads():
    """-> (posts, seqs, pairs): every sequence on a read of len + 2 blocks and on one of len + 2 + 16"""
    rng = np.random.default_rng(53)
    seqs = [rng.integers(0, 4, n).astype(np.uint8) for n in LENGTHS]
    posts = [rng.normal(-2.0, 1.0, size=(len(s) + 2 + more, 40)).astype(np.float32) for s in seqs for more in (0, 16)]
    return posts, seqs, [(r, r // 2) for r in range(len(posts))]


@functools.lru_cache(maxsize=None)
def want(md):
    """the definitions on every pair, once: -> (reference_score float32 [n, 2], reference_forward float64 [n, 2])"""
    posts, seqs, pairs = reads()
    return (np.array([T.reference_score(posts[r], seqs[s], md) for r, s in pairs], np.float32),
            np.array([T.reference_forward(posts[r], seqs[s], md) for r, s in pairs], np.float64))


@pytest.fixture(scope="module")
def dec():
    with pkg.Decoder(6, 1, 60, list_size=4, max_deviation=20, device=0, max_slots=4) as d:
        yield d


@pytest.mark.parametrize("md", [4, OFF])
def test_no_rule_reaches_another_kernel(dec, md):
    posts, seqs, pairs = reads()
    assert md == 4 or md >= max(LENGTHS) + 1
    score, f64 = want(md)
    first = dec.score_bases(posts, seqs, pairs, max_deviation=md)
    traced = dec.trace_bases(posts, seqs, pairs, max_deviation=md)["score"]
    fw = dec.forward_bases(posts, seqs, pairs, max_deviation=md)
    again = dec.score_bases(posts, seqs, pairs, max_deviation=md)
    assert first.shape == (len(pairs), 2) and np.isfinite(first).any(axis=1).all()
    assert same_bits(first, traced) and same_bits(first, score) and same_bits(again, first)
    assert np.isfinite(f64).any(axis=1).all()
    for k, (r, _) in enumerate(pairs):
        tol = _bound(f64[k], len(posts[r]))
        print(md, k, fw[k].tolist(), f64[k].tolist(), "E_gpu %.3g bound %.3g" % (err(fw[k], f64[k]), tol))
        assert err(fw[k], f64[k]) <= tol
