"""The one-message trellis on the GPU (sc_score, st_fill / st_walk, fw_forward: one frame, csrc/sc_frame.h) at the shapes that
no other test runs -- the case classes of tests/trellis_shape_cases.py, which tests/test_trellis_shape_cases_host.py holds to
what they claim.  For every class and max_deviation, on the same pairs in one call per kernel:

  score          score_bases is trellis_score.reference_score's float32 bits;
  trace          trace_bases' scores are the same bits, and for end in (-1, 0, 1) every array is reference_trace's byte for
                 byte (trellis_trace_cases.same_trace: the stride tail and n_stale included);
  forward        forward_bases lies within test_gpu_trellis_forward._bound of reference_forward in float64
                 (trellis_forward_cases.err; no other tolerance; a pair without a finite value is -inf on both sides);
  forward/score  with the band off no cell is stale and a log-sum-exp is at least its largest term: forward >= score - bound;
  score again    score_bases after the two others returns its first bits.

The gaps the classes close (each named again at its test): 1 long sequences (LONG), 2 bands between one pass and the whole
sequence (WIDE), 3 where trace_width switches (WIDTH), 4 stale hops at the edge of a run in st_walk (RUN_EDGE), 5 staged-row
remainders (REMAINDERS), 6 one call, extreme mix (LONG)."""
import numpy as np
import pytest

import nanopore_dna_storage_amd as pkg
import trellis_shape_cases as C
from test_gpu_trellis_forward import _bound
from test_gpu_trellis_trace import _need
from trellis_forward_cases import err
from trellis_trace_cases import same_trace

pytestmark = pytest.mark.gpu

NEG = np.float32(-np.inf)


def same_bits(a, b):
    return np.asarray(a, np.float32).tobytes() == np.asarray(b, np.float32).tobytes()


@pytest.fixture(scope="module")
def dec():
    with pkg.Decoder(6, 1, 60, list_size=4, max_deviation=20, device=0, max_slots=4) as d:
        yield d


def check_traces(c, got, w, end, pairs=None):
    """got: trace_bases' result for `pairs` (indices into the class's pairs; default all, in order)"""
    pairs = range(len(c["pairs"])) if pairs is None else pairs
    for row, k in enumerate(pairs):
        n = len(c["seqs"][c["pairs"][k][1]])
        t = w["trace"][end][k]
        assert same_trace(got, row, t, n), (k, end, t, {key: got[key][row][:n] for key in got})
        assert int(got["n_stale"][row]) == t["n_stale"]


def check_forward(name, md, c, fw, w):
    assert fw.dtype == np.float32 and fw.shape == w["f64"].shape
    for k, (r, _) in enumerate(c["pairs"]):
        f64 = w["f64"][k]
        tol = _bound(f64, len(c["posts"][r])) if np.isfinite(f64).any() else 0.0     # nothing finite: -inf, exactly
        e = err(fw[k], f64)
        print(name, md, k, fw[k].tolist(), f64.tolist(), "E_gpu %.3g E_f32 %.3g bound %.3g" % (e, err(w["f32"][k], f64), tol))
        assert e <= tol, (name, md, k)
        if md == C.OFF and np.isfinite(f64).any():           # band off: no stale cell, so the sum over paths holds the best path
            assert (fw[k].astype(np.float64) >= w["score"][k].astype(np.float64) - tol).all(), (name, md, k, fw[k], w["score"][k])


def check_class(dec, name, md):
    """the six checks of this file's docstring on one class under one max_deviation -> (the class, the definitions, the score
    call's result, the trace's of end = -1)"""
    c, w = C.klass(name), C.want(name, md)
    posts, seqs, pairs = c["posts"], c["seqs"], c["pairs"]
    first = dec.score_bases(posts, seqs, pairs, max_deviation=md)
    traced = {end: dec.trace_bases(posts, seqs, pairs, max_deviation=md, end=end) for end in C.ENDS}
    fw = dec.forward_bases(posts, seqs, pairs, max_deviation=md)
    again = dec.score_bases(posts, seqs, pairs, max_deviation=md)
    n = C.counts(name, md)
    print(name, "max_deviation", md, n)
    assert first.shape == (len(pairs), 2) and same_bits(first, w["score"])
    for end in C.ENDS:
        assert same_bits(traced[end]["score"], first)
        assert traced[end]["enter"].shape == (len(pairs), max(len(s) for s in seqs))
        check_traces(c, traced[end], w, end)
    check_forward(name, md, c, fw, w)
    assert same_bits(again, first)
    return c, w, first, traced[-1]


@pytest.mark.parametrize("md", [20, C.OFF])
def test_long_sequences_and_the_extreme_mix_in_one_call(dec, md):
    """gap 1, long sequences: 1024 bases -- 1025 positions, 17 passes of 64 lanes, the largest LDS; st_fill's brow[p - lo] and
    st_walk's row stride where.w and col - lo at a width of 1025 -- on 1026 blocks (the fewest), on a read cut to 1026 and on
    one of 1130.  gap 6, one call, extreme mix: the prefixes of 1 and 2 bases are pairs of the same call, whose LDS the
    1024-mer sizes."""
    c, w, first, _ = check_class(dec, "LONG", md)
    assert {len(c["seqs"][s]) for _, s in c["pairs"]} >= {1, 2, 1024}
    assert np.isfinite(first[c["pairs"].index((2, 0))]).any() or md != C.OFF


def test_long_unbanded_trace_in_chunks_of_one_pair(dec):
    """gap 1: the unbanded 1024-mer's back-pointers, rows of 1025 bytes, with the default scratch and with a scratch_limit of the
    call's largest single need -- a chunk per large pair -- give the same bytes, the definition's"""
    c, w = C.klass("LONG"), C.want("LONG", C.OFF)
    need = _need(c["posts"], c["seqs"], c["pairs"], C.OFF)
    assert max(need) == (1130 * 1025 + 15) // 16 * 16 and sorted(need)[-3] > max(need) // 2      # three pairs, a chunk each
    whole = dec.trace_bases(c["posts"], c["seqs"], c["pairs"], max_deviation=C.OFF)
    cut = dec.trace_bases(c["posts"], c["seqs"], c["pairs"], max_deviation=C.OFF, scratch_limit=max(need))
    for key in whole:
        assert whole[key].tobytes() == cut[key].tobytes(), key
    check_traces(c, cut, w, -1)


@pytest.mark.parametrize("md", [20, C.OFF])
def test_long_resident_entry_points_give_the_host_calls_bytes(dec, md):
    """gap 1 and gap 6 through score_bases_resident, trace_bases_resident and forward_bases_resident: windows of one buffer"""
    c, w = C.klass("LONG"), C.want("LONG", md)
    posts, seqs, pairs = c["posts"], c["seqs"], c["pairs"]
    pad = np.zeros((5, 40), np.float32)
    with dec.resident([pad] + posts + [pad]) as (dev, off):
        at = (dev, off[1:-2], np.diff(off)[1:-1], seqs, pairs)
        score = dec.score_bases_resident(*at, max_deviation=md)
        trace = dec.trace_bases_resident(*at, max_deviation=md)
        fw = dec.forward_bases_resident(*at, max_deviation=md)
    assert same_bits(score, w["score"]) and same_bits(score, dec.score_bases(posts, seqs, pairs, max_deviation=md))
    host = dec.trace_bases(posts, seqs, pairs, max_deviation=md)
    for key in host:
        assert host[key].tobytes() == trace[key].tobytes(), key
    check_traces(c, trace, w, -1)
    assert same_bits(fw, dec.forward_bases(posts, seqs, pairs, max_deviation=md))


@pytest.mark.parametrize("md", C.WIDE_MDS)
def test_bands_between_one_pass_and_the_whole_sequence(dec, md):
    """gap 2, bands between one pass and the whole sequence: 66, 128, 130 and 200 positions on 257 and 300 bases -- two to four
    passes, the last partial, lo moving at nearly every block: st_fill's brow[p - lo] across passes, and fw_forward's cleared
    band (plo / phi of the block before) cutting through the middle of a pass"""
    c, w, first, _ = check_class(dec, "WIDE", md)
    assert np.isfinite(first).any(axis=1).all()
    for r, s in c["pairs"]:
        widest, moves = C.wide_band(c, r, s, md)
        assert widest == 2 * md > 64 and moves >= 100


@pytest.mark.parametrize("md", [5, 6, 32, 33])
def test_where_trace_width_switches(dec, md):
    """gap 3, where trace_width switches: w = min(2 * md, len + 1) at 2 * md = len, len + 1 and len + 2 for 9, 10, 63 and 64
    bases; a scratch_limit of exactly the largest need is enough, as the width's formula says"""
    c, w, first, whole = check_class(dec, "WIDTH", md)
    need = _need(c["posts"], c["seqs"], c["pairs"], md)
    assert any(2 * md - len(s) in (0, 1, 2) for s in c["seqs"])                              # a neighbour of a switch
    cut = dec.trace_bases(c["posts"], c["seqs"], c["pairs"], max_deviation=md, scratch_limit=max(need))
    for key in whole:
        assert whole[key].tobytes() == cut[key].tobytes(), key
    with pytest.raises(pkg.LvaError) as e:
        dec.trace_bases(c["posts"], c["seqs"], c["pairs"], max_deviation=md, scratch_limit=max(need) - 1)
    assert e.value.code == -10


def test_max_deviation_zero_is_an_empty_band(dec):
    """gap 3, max_deviation = 0: w = 0 and zero bytes of scratch, every band empty -- scores (-inf, -inf), end_state -1, enter
    all -1, kind all 255; the same call with scratch_limit = 16 succeeds, because the need is 0 bytes"""
    c, w, first, tr = check_class(dec, "WIDTH", 0)
    assert _need(c["posts"], c["seqs"], c["pairs"], 0) == [0] * len(c["pairs"])
    small = dec.trace_bases(c["posts"], c["seqs"], c["pairs"], max_deviation=0, scratch_limit=16)
    for got in (tr, small):
        assert same_bits(got["score"], np.full((len(c["pairs"]), 2), NEG))
        assert (got["end_state"] == -1).all() and (got["start_state"] == -1).all() and (got["n_stale"] == 0).all()
        assert (got["enter"] == -1).all() and (got["kind"] == 255).all()
    assert same_bits(first, np.full((len(c["pairs"]), 2), NEG))
    assert same_bits(dec.forward_bases(c["posts"], c["seqs"], c["pairs"], max_deviation=0), np.full((len(c["pairs"]), 2), NEG))


@pytest.mark.parametrize("md", [1, 2, 3])
def test_stale_hops_at_the_edge_of_a_run(dec, md):
    """gap 4, stale hops at the edge of a run in st_walk: the frozen reads hold a hop at u = 63 (the walk leaves the run with
    u = 65) and at u = 62 (u = 64), one in a run of fewer than 64 rows and three runs with a hop each
    (test_trellis_shape_cases_host.py); the device's n_stale is the definition's -- every case alone, then all of them in one
    shuffled call"""
    c, w, first, whole = check_class(dec, "RUN_EDGE", md)
    posts, seqs, pairs = c["posts"], c["seqs"], c["pairs"]
    mine = [k for k, frozen_md in c["frozen"] if frozen_md == md]
    assert mine and all(w["trace"][-1][k]["n_stale"] > 0 for k in mine)
    assert [int(x) for x in whole["n_stale"]] == [t["n_stale"] for t in w["trace"][-1]]
    for k in range(len(pairs)):
        alone = dec.trace_bases(posts, seqs, [pairs[k]], max_deviation=md)
        print("md", md, "case", k, "n_stale", int(alone["n_stale"][0]), w["trace"][-1][k]["n_stale"])
        check_traces(c, alone, w, -1, pairs=[k])
    order = [int(i) for i in np.random.default_rng(md).permutation(len(pairs))]
    order = order[::-1] if order == sorted(order) else order
    assert order != sorted(order) and len(order) > 1
    shuffled = dec.trace_bases(posts, seqs, [pairs[k] for k in order], max_deviation=md)
    check_traces(c, shuffled, w, -1, pairs=order)


@pytest.mark.parametrize("md", [3, C.OFF])
def test_every_remainder_of_the_staged_rows(dec, md):
    """gap 5, staged-row remainders: sc_frame stages 16 posterior rows at a time; 16 reads of 90 to 105 blocks, one per value
    of nblk mod 16, under a band of 3 that moves at every other block, and with the band off"""
    c, w, first, _ = check_class(dec, "REMAINDERS", md)
    assert {len(p) % 16 for p in c["posts"]} == set(range(16)) and np.isfinite(first).any(axis=1).all()
