"""The case classes of tests/trellis_shape_cases.py are what tests/test_gpu_trellis_shapes.py takes them to be -- checked on the
definitions alone (trellis_score.py), without a GPU: a case that no longer reaches its shape would let the GPU test pass and
show nothing.  This is also where the CPU cost of the definitions shows (trellis_shape_cases' docstring has the figures)."""
import numpy as np
import pytest

from nanopore_dna_storage_amd import trellis_score as T
import trellis_shape_cases as C
from test_gpu_trellis_forward import _bound
from test_gpu_trellis_trace import _need
from trellis_forward_cases import err


@pytest.mark.parametrize("name", C.NAMES)
def test_every_class_has_a_finite_score_and_a_flop_on_a_traced_path(name):
    c = C.klass(name)
    total = dict(pairs=0, finite=0, flops=0, stale=0)
    for md in c["mds"]:
        n = C.counts(name, md)
        print(name, "max_deviation", md, n)
        for key in total:
            total[key] += n[key]
        w = C.want(name, md)
        for end in C.ENDS:                                   # the trace's scores are the score's, on the CPU too
            assert np.array([t["score"] for t in w["trace"][end]], np.float32).tobytes() == w["score"].tobytes()
    assert total["finite"] > 0 and total["flops"] > 0
    if name in ("RUN_EDGE", "REMAINDERS", "LONG"):           # a narrow band: the path leaves it and comes back
        assert total["stale"] > 0


@pytest.mark.parametrize("name", ["LONG", "WIDE"])
def test_the_forward_bound_holds_for_the_float32_restatement(name):
    """the bound of tests/test_gpu_trellis_forward.py at the long and wide shapes: if the restatement missed it, it would be too
    tight for the shape, and a device that missed it no finding"""
    c = C.klass(name)
    for md in c["mds"]:
        w = C.want(name, md)
        for k, (r, _) in enumerate(c["pairs"]):
            if not np.isfinite(w["f64"][k]).any():
                assert err(w["f32"][k], w["f64"][k]) == 0
                continue
            e32, tol = err(w["f32"][k], w["f64"][k]), _bound(w["f64"][k], len(c["posts"][r]))
            print(name, md, k, "E_f32 %.3g bound %.3g" % (e32, tol))
            assert e32 <= tol


def test_long_reaches_the_longest_sequence_on_the_fewest_blocks():
    """gap 1 (long sequences) and gap 6 (one call, extreme mix): 1024 bases on exactly 1026 blocks has a path with the band off,
    and the 1-base and 2-base prefixes are pairs of the same call"""
    c = C.klass("LONG")
    k = c["pairs"].index((2, 0))
    assert len(c["seqs"][0]) == 1024 and len(c["posts"][2]) == 1026
    assert np.isfinite(C.want("LONG", C.OFF)["score"][k]).any()
    assert {len(c["seqs"][s]) for _, s in c["pairs"]} >= {1, 2, 1024}
    assert C.OFF >= 1025 and T.band_table(1026, 1025, C.OFF)[:, 0].max() == 0


def test_wide_bands_span_passes_and_move():
    """gap 2 (bands between one pass and the whole sequence): 66, 128, 130 and 200 positions -- two passes of 64 lanes with the
    second nearly empty, exactly two, two and a bit, four with the last partial -- and lo at 100 values or more"""
    c = C.klass("WIDE")
    assert sorted(len(s) for s in c["seqs"]) == [257, 300] and c["mds"] == (33, 64, 65, 100)
    for r, s in c["pairs"]:
        assert 2.0 <= len(c["posts"][r]) / len(c["seqs"][s]) <= 2.4
        for md, width, passes in zip(c["mds"], (66, 128, 130, 200), (2, 2, 3, 4)):
            widest, moves = C.wide_band(c, r, s, md)
            print(len(c["seqs"][s]), md, "widest band", widest, "distinct lo", moves)
            assert widest == width == 2 * md < len(c["seqs"][s]) + 1 and -(-widest // 64) == passes
            assert moves >= 100


def test_width_switches_where_the_cases_say():
    """gap 3 (where trace_width switches): w = min(2 * md, len + 1), as trace_width of csrc/lva_stages.cpp and as _need of
    tests/test_gpu_trellis_trace.py state it; per length the neighbours 2 * md = len, len + 1, len + 2, and md = 0"""
    c = C.klass("WIDTH")
    assert tuple(len(s) for s in c["seqs"]) == (9, 10, 63, 64) and c["mds"] == (0, 5, 6, 32, 33)
    assert [C.width_mds(n) for n in (9, 10, 63, 64)] == [[5], [5, 6], [32], [32, 33]]
    for n in (9, 10, 63, 64):
        assert {2 * md for md in C.width_mds(n)} == {v for v in (n, n + 1, n + 2) if v % 2 == 0}
        for md in c["mds"]:
            w = min(2 * md, n + 1)                           # the rule
            assert C.trace_width(md, n) == w
            assert w == (2 * md if 2 * md <= n + 1 else n + 1)
            post, seq = np.zeros((n + 2, 40), np.float32), np.zeros(n, np.uint8)
            assert _need([post], [seq], [(0, 0)], md) == [((n + 2) * w + 15) // 16 * 16]
            bands = T.band_table(n + 2, n + 1, md)
            assert (bands[:, 1] - bands[:, 0]).max() <= w      # a row of w bytes holds every block's band
    assert C.trace_width(0, 9) == 0 and _need([np.zeros((11, 40))], [np.zeros(9)], [(0, 0)], 0) == [0]
    assert (C.trace_width(5, 10), C.trace_width(6, 10)) == (10, 11)       # below the switch, and at it
    assert (C.trace_width(32, 64), C.trace_width(33, 64)) == (64, 65)
    assert (C.trace_width(5, 9), C.trace_width(32, 63)) == (10, 64)       # 2 * md = len + 1: both terms
    w0 = C.want("WIDTH", 0)                                  # max_deviation 0: (-inf, -inf) and no path, from the definitions
    assert np.isneginf(w0["score"]).all() and np.isneginf(w0["f64"]).all()
    assert all(t["end_state"] == -1 and t["n_stale"] == 0 for end in C.ENDS for t in w0["trace"][end])


def test_run_edge_places_stale_hops_at_the_last_rows_of_a_run():
    """gap 4 (stale hops at the edge of a run in st_walk): across the frozen cases a hop at u = 63, one at u = 62, one in a run
    of fewer than 64 rows and a read with three runs that each hold a hop; the replay counts the definition's n_stale"""
    c = C.klass("RUN_EDGE")
    assert all(len(p) >= 200 for p in c["posts"]) and set(c["mds"]) <= {1, 2, 3}
    got = C.run_edge_conditions()
    print(got)
    assert got == dict(hop_at_u63=True, hop_at_u62=True, hop_in_a_short_run=True, three_runs_with_a_hop=True)
    for k, md in c["frozen"]:
        assert C.want("RUN_EDGE", md)["trace"][-1][k]["n_stale"] > 0


def test_run_edge_guard_sees_a_case_that_lost_its_hops():
    """the guard itself: the same reads under a band that holds their paths have no stale hop, and every condition fails"""
    c = C._run_edge(tuple((seed, n, nblk, 60) for seed, n, nblk, _ in C.RUN_EDGE_FROZEN))
    assert not any(C.run_edge_conditions(c).values())


def test_walk_runs_on_a_path_made_by_hand():
    """3 bases on 70 blocks, band 1 (two positions): the path enters its positions in the first blocks and stands at 3 from
    then on, outside the band until the band reaches it -- the hops of the replay are where the band table says"""
    nblk, enter = 70, np.array([1, 2, 3])
    bands = T.band_table(nblk, 4, 1)
    at = T.positions_after(enter, nblk)
    hops = C.walk_runs(enter, nblk, 1)
    t, want = nblk - 1, []
    while t >= 0:                                            # the definition's walk: t - 2 on a stale cell, t - 1 otherwise
        stale = not bands[t, 0] <= at[t] < bands[t, 1]
        want += [t] if stale else []
        t -= 2 if stale else 1
    assert t == -1 and len(hops) == len(want) > 0
    assert [nblk - 1 - u for u, _, run in hops if run == 0] == [t for t in want if t >= nblk - 64]     # the first run: blocks 69 .. 6
    assert hops[0] == (nblk - 1 - 52, 64, 0)                 # the band reaches position 3 at block 53: the first hop is at block 52
    assert (63, 64, 0) in hops                               # block 6, the run's last row: the next run starts at block 4
    assert [(u, nrows) for u, nrows, run in hops if run == 1] == [(0, 5), (2, 5)]                    # blocks 4 and 2


def test_remainders_cover_every_staged_row_count():
    """gap 5 (staged-row remainders): one read per value of nblk mod 16, and under band 3 lo moves on every one"""
    c = C.klass("REMAINDERS")
    assert len(c["seqs"]) == 1 and len(c["seqs"][0]) == 40 and c["mds"] == (3, C.OFF)
    assert sorted(len(p) for p in c["posts"]) == list(range(90, 106))
    assert {len(p) % 16 for p in c["posts"]} == set(range(16))
    for p in c["posts"]:
        assert len(set(T.band_table(len(p), 41, 3)[:, 0].tolist())) >= 30
