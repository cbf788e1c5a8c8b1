"""The traceback of the one-message trellis without a GPU: trellis_score.reference_trace, the definition of
csrc/st_kernels.hip.  Its scores are reference_score's bits; a path without stale hops adds up to its end score, one float32
addition per block, and on the top entry of an oracle list that is the list's score; on small cases the path is an argmax
over every alignment and, where everything ties, the first in the tie rule's order; the stale-band fixtures give stale hops;
deviation_needed is the smallest band by exhaustion; the C entry points refuse a null decoder."""
import itertools

import numpy as np
import pytest

from nanopore_dna_storage_amd import _lib, str_to_bits
from nanopore_dna_storage_amd import trellis_score as T
from trellis_score_cases import FIXTURES, case
from trellis_trace_cases import path_sum, truth_seq

NEG = np.float32(-np.inf)


def bits(x):
    return np.asarray(x, np.float32).tobytes()


_traces = {}


def truth_trace(name):
    """the trace of a fixture's true message under the fixture's band, computed once"""
    if name not in _traces:
        c = case(name)
        _traces[name] = T.reference_trace(c["post"], truth_seq(c), c["md"])
    return _traces[name]


@pytest.mark.parametrize("name", FIXTURES)
def test_score_is_reference_score_bit_for_bit(name):
    c = case(name)
    tr = truth_trace(name)
    assert bits(tr["score"]) == bits(T.reference_score(c["post"], truth_seq(c), c["md"]))
    n = len(truth_seq(c))
    assert tr["enter"].dtype == np.int32 and tr["enter"].shape == (n,) and tr["kind"].dtype == np.uint8 and tr["kind"].shape == (n,)
    if tr["end_state"] >= 0:
        assert tr["end_state"] == int(tr["score"][1] > tr["score"][0]) and 0 <= tr["start_state"] < 8
        assert set(tr["kind"].tolist()) <= {0, 1} and tr["kind"][-1] == tr["end_state"]
        assert (np.diff(tr["enter"]) > 0).all() and tr["enter"][0] >= 0 and tr["enter"][-1] < c["post"].shape[0]


@pytest.mark.parametrize("name", FIXTURES)
def test_a_path_without_stale_hops_adds_up_to_its_score(name):
    c = case(name)
    tr = truth_trace(name)
    print(name, "n_stale", tr["n_stale"], "score", tr["score"])
    if name in ("m6_r1_L8_unbanded",):
        assert tr["n_stale"] == 0 and tr["end_state"] >= 0   # the band is off: no cell is ever stale
    if tr["end_state"] >= 0 and tr["n_stale"] == 0:
        assert bits(path_sum(c["post"], truth_seq(c), tr)) == bits(tr["score"][tr["end_state"]])
    for end in (0, 1):                                       # and from either end state that has a path
        one = T.reference_trace(c["post"], truth_seq(c), c["md"], end=end)
        assert bits(one["score"]) == bits(tr["score"])
        assert (one["end_state"] == end) == (tr["score"][end] != NEG)
        if one["end_state"] >= 0 and one["n_stale"] == 0:
            assert bits(path_sum(c["post"], truth_seq(c), one)) == bits(tr["score"][end])


@pytest.mark.parametrize("name", FIXTURES)
def test_the_top_entry_of_a_list_adds_up_to_the_lists_score(oracle, name):
    c = case(name)
    msgs, scores = oracle.OracleCode(*c["code"], rc=c["rc"], **c["sync"]).decode(c["post"], c["m"]["list_size"], c["md_arg"])
    seq = T.message_bases(*c["code"], msgs[0], c["rc"], **c["sync"])
    tr = T.reference_trace(c["post"], seq, c["md"])
    assert bits(max(tr["score"])) == bits(scores[0]) and tr["end_state"] >= 0
    print(name, "n_stale of the top entry", tr["n_stale"])
    if tr["n_stale"] == 0:
        assert bits(path_sum(c["post"], seq, tr)) == bits(scores[0])
    if name in ("m6_r1_L8_unbanded", "m6_r1_L8_wide"):       # with the band off no cell is stale: these two always add up
        off = T.reference_trace(c["post"], seq, len(seq) + 1)
        assert off["n_stale"] == 0 and bits(path_sum(c["post"], seq, off)) == bits(max(off["score"]))
        assert name != "m6_r1_L8_unbanded" or bits(max(off["score"])) == bits(scores[0])


def test_stale_band_fixtures_give_stale_hops():
    n = {name: truth_trace(name)["n_stale"] for name in FIXTURES if "edge" in name}
    print(n)
    assert len(n) == 3 and max(n.values()) > 0
    tr = truth_trace(max(n, key=n.get))
    assert tr["end_state"] >= 0 and (tr["enter"] >= 0).all()             # a path all the same: every position is entered


# --- brute force: every monotone alignment of a short sequence ---------------------------------------------------

def alignments(seq, nblk):
    """every path: (start_state, enter blocks) -> (enter, kind, end_state, choices), choices the walk's decisions from the last
    block back to block 0 (0: stay, 1 + s: a flip entered from state s, 1: a flop entered by its step).  The kinds follow from
    the start state: a position is entered as flop exactly when the state below is the flip of the same base."""
    n = len(seq)
    for s0 in range(8):
        for enter in itertools.combinations(range(nblk), n):
            state, kind, how = s0, [], {}
            for p, t in enumerate(enter):
                b = int(seq[p])
                if state == b:
                    kind.append(1)
                    how[t] = 1
                    state = b + 4
                else:
                    kind.append(0)
                    how[t] = 1 + state
                    state = b
            yield s0, np.array(enter, np.int32), np.array(kind, np.uint8), kind[-1], tuple(how.get(t, 0) for t in range(nblk - 1, -1, -1))


def brute(post, seq):
    """-> (the best float32 score over every alignment, the alignments that reach it as (end_state, choices, start, enter, kind))"""
    best, arg = NEG, []
    for s0, enter, kind, end, how in alignments(seq, post.shape[0]):
        v = path_sum(post, seq, dict(start_state=s0, enter=enter, kind=kind))
        if v > best:
            best, arg = v, []
        if v == best:
            arg.append((end, how, s0, enter, kind))
    return best, arg


SMALL = [(n, nblk) for n in (1, 2, 3, 4) for nblk in range(max(3, n + 2), 8)]


@pytest.mark.parametrize("n, nblk", SMALL)
def test_the_traced_path_is_an_argmax_over_every_alignment(n, nblk):
    rng = np.random.default_rng(100 * n + nblk)
    for trial in range(6):
        seq = rng.integers(0, 2 if trial % 2 else 4, size=n).astype(np.uint8)      # (two letters: homopolymer runs, flops)
        post = rng.normal(-2.0, 1.0, size=(nblk, 40)).astype(np.float32)
        tr = T.reference_trace(post, seq, n + 1)
        best, arg = brute(post, seq)
        assert bits(max(tr["score"])) == bits(best)
        assert any(tr["start_state"] == s0 and np.array_equal(tr["enter"], e) and np.array_equal(tr["kind"], k) for _, _, s0, e, k in arg)
        assert bits(path_sum(post, seq, tr)) == bits(best)


@pytest.mark.parametrize("n, nblk", SMALL)
def test_where_everything_ties_the_path_is_the_first_in_the_tie_rules_order(n, nblk):
    for seq in (np.zeros(n, np.uint8), (np.arange(n) % 4).astype(np.uint8), np.array(([1, 1, 2, 2] * 2)[:n], np.uint8)):
        post = np.zeros((nblk, 40), np.float32)
        best, arg = brute(post, seq)
        assert best == 0 and len(arg) > 1
        first = min(arg, key=lambda a: (a[0], a[1]))         # flip before flop at the end, then the walk's decisions in its order
        tr = T.reference_trace(post, seq, n + 1)
        assert tr["score"][first[0]] == 0 and tr["end_state"] == first[0] and tr["start_state"] == first[2]
        assert np.array_equal(tr["enter"], first[3]) and np.array_equal(tr["kind"], first[4])
        for end in (0, 1):
            some = [a for a in arg if a[0] == end]
            one = T.reference_trace(post, seq, n + 1, end=end)
            if not some:
                assert one["end_state"] == -1 and (one["enter"] == -1).all() and (one["kind"] == 255).all() and one["start_state"] == -1
                continue
            want = min(some, key=lambda a: a[1])
            assert one["start_state"] == want[2] and np.array_equal(one["enter"], want[3]) and np.array_equal(one["kind"], want[4])


def test_no_path():
    post = np.zeros((6, 40), np.float32)
    post[2] = NEG                                            # a block that forbids every transition, the band off: nothing survives
    tr = T.reference_trace(post, [0, 1, 2], 9)
    assert tr["score"] == (NEG, NEG) and tr["end_state"] == tr["start_state"] == -1 and tr["n_stale"] == 0
    assert tr["enter"].tolist() == [-1] * 3 and tr["kind"].tolist() == [255] * 3


def test_refusals_of_the_definition():
    post = np.zeros((10, 40), np.float32)
    for bad in ([], [0, 4], "ACGN"):
        with pytest.raises(ValueError):
            T.reference_trace(post, bad, 5)
    with pytest.raises(ValueError):
        T.reference_trace(post[:4], [0, 1, 2], 5)
    for end in (-2, 2):
        with pytest.raises(ValueError):
            T.reference_trace(post, [0, 1, 2], 5, end=end)
    p = post.copy()
    p[3, 7] = np.nan
    with pytest.raises(ValueError):
        T.reference_trace(p, [0, 1, 2], 5)


# --- what a band does to a path -----------------------------------------------------------------------------

def random_path(rng):
    n = int(rng.integers(1, 40))
    nblk = int(rng.integers(n + 2, 4 * n + 12))
    return np.sort(rng.choice(nblk, size=n, replace=False)).astype(np.int32), nblk


def test_deviation_needed_is_the_smallest_band_that_holds_the_path():
    rng = np.random.default_rng(7)
    seen = set()
    for _ in range(50):
        enter, nblk = random_path(rng)
        holds = [T.band_contains(enter, nblk, D) for D in range(1, len(enter) + 3)]
        assert holds[-1] and holds[-2]
        first = holds.index(True) + 1
        assert T.deviation_needed(enter, nblk) == first
        assert all(holds[first - 1:])                        # monotone: D holds the path -> D + 1 does
        assert T.left_band_at(enter, nblk, first) == -1
        if first > 1:
            t = T.left_band_at(enter, nblk, first - 1)
            lo, hi = T.band_table(nblk, len(enter) + 1, first - 1)[t]
            at = T.positions_after(enter, nblk)
            assert t >= 0 and not lo <= at[t] < hi and all(a <= at[u] < b for u, (a, b) in enumerate(T.band_table(nblk, len(enter) + 1, first - 1)[:t]))
        seen.add(first)
    assert len(seen) > 5
    with pytest.raises(ValueError):
        T.deviation_needed(np.array([-1, -1]), 9)


def test_a_truth_that_the_band_holds_needs_at_most_the_band():
    c = case("m6_r1_L4_indel")
    tr = truth_trace("m6_r1_L4_indel")
    assert tr["n_stale"] == 0
    wide = T.reference_trace(c["post"], truth_seq(c), len(truth_seq(c)) + 1)
    need = T.deviation_needed(wide["enter"], c["post"].shape[0])
    assert 1 <= need <= c["md"] and T.left_band_at(wide["enter"], c["post"].shape[0], c["md"]) == -1
    assert np.array_equal(wide["enter"], tr["enter"])        # and under the band it is the same path


# --- the tool's files -----------------------------------------------------------------------------------------

def test_table_columns_and_the_trace_file(tmp_path):
    enter = np.array([3, 5, 9], np.int32)
    rows = [dict(rank=0, banded=np.float32(-5), unbanded=np.float32(-5), first=-5.0, last=-9.0, verdict="in_list", dev_needed=4,
                 left_band_at=-1, trace=dict(start_state=2, end_state=0, enter=enter)),
            dict(rank=-1, banded=NEG, unbanded=np.float32(-7), first=-6.0, last=-9.5, verdict="band", dev_needed=31, left_band_at=17,
                 trace=dict(start_state=7, end_state=1, enter=enter + 1)),
            dict(rank=-1, banded=NEG, unbanded=np.float32(-8), first=-6.0, last=-9.5, verdict="band", dev_needed=12, left_band_at=40,
                 trace=dict(start_state=7, end_state=1, enter=enter + 1)),
            dict(rank=-1, banded=None, unbanded=None, first=float("nan"), last=float("nan"), verdict="short_read",
                 dev_needed=float("nan"), left_band_at=-1, trace=None)]
    T.write_table(rows, str(tmp_path / "x.truth.tsv"))
    lines = [ln.split("\t") for ln in open(str(tmp_path / "x.truth.tsv")).read().splitlines()]
    assert lines[0] == ["read", "rank", "banded", "unbanded", "first", "last", "verdict", "dev_needed", "left_band_at"]
    assert [ln[7:] for ln in lines[1:]] == [["4", "-1"], ["31", "17"], ["12", "40"], ["nan", "-1"]]
    assert lines[1][:7] == ["0", "0", "-5.0", "-5.0", "-5.0", "-9.0", "in_list"]
    T.write_trace(rows, str(tmp_path / "x.trace.tsv"))
    lines = [ln.split("\t") for ln in open(str(tmp_path / "x.trace.tsv")).read().split("\n")[:-1]]
    assert lines[0] == ["read", "start_state", "end_state", "enter"]
    assert lines[1] == ["0", "2", "0", "3,5,9"] and lines[2] == ["1", "7", "1", "4,6,10"] and lines[4] == ["3", "-1", "-1", ""]
    assert T.band_dev_needed(rows) == 31 and T.band_dev_needed(rows[:1]) == 0
    assert T.summary_line(rows, dev_needed=True) == T.summary_line(rows) + ", band dev_needed 31"
    assert T.build_parser().parse_args(["--simulate", "1"]).trace is False


def test_simulator_summary_carries_the_count():
    import io
    from nanopore_dna_storage_amd import simulator
    args = simulator.build_parser().parse_args([])
    args.msg_len, args.num_trials = 4, 1
    reads = [dict(msg=np.array([0, 1, 1, 0], np.uint8), oligo=np.array([0, 1], np.uint8))]
    results = [(np.array([[1, 1, 1, 0]], np.uint8), np.array([-1.0], np.float32))]
    rows = [dict(rank=-1, banded=NEG, unbanded=np.float32(-1), first=-1.0, last=-1.0, verdict="band", dev_needed=9, left_band_at=2,
                 trace=None)]
    stats = simulator.report(args, reads, results, io.StringIO(), truth_rows=rows)
    assert stats["Number truth band"] == 1 and stats["Number truth band dev_needed"] == 9


# --- the C entry points without a device -------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["lva_trace_bases", "lva_trace_bases_device"])
def test_null_decoder_is_an_argument_error(name):
    fn = getattr(_lib.load_library(), name)
    buf = np.zeros(64, np.int64)
    p = buf.ctypes.data
    where = (p, p) if name == "lva_trace_bases" else (p, p, p)
    assert fn(None, *where, 0, p, p, p, 0, p, 0, 5, -1, 0, 4, p, p, p, p) == -10
    assert fn(None, *(None,) * len(where), 0, None, None, None, 0, None, 0, 5, -1, 0, 4, None, None, None, None) == -10
    assert fn(None, *where, 0, p, p, p, 0, p, 0, 5, 7, 0, 4, p, p, p, p) == -10        # the decoder is looked at first


def test_the_entry_points_are_in_the_header_the_table_and_the_build():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "lva_decoder.h")).read()
    for name in ("lva_trace_bases", "lva_trace_bases_device"):
        assert "int %s(" % name in header and name in _lib.EXPORTS
    assert "#define LVA_ABI_VERSION 5" in header and _lib.ABI_VERSION == 5
    mk = open(os.path.join(root, "nanopore_dna_storage_amd", "csrc", "Makefile")).read()
    assert " st_kernels.hip" in mk and " st_kernels.h " in mk
