"""What the shape tests of the one-message trellis share (tests/test_trellis_shape_cases_host.py,
tests/test_gpu_trellis_shapes.py): five case classes at the shapes that csrc/sc_frame.h, st_kernels.hip and fw_kernels.hip take
other paths at, each with the definitions' answers (trellis_score.reference_score, reference_trace for the three end rules,
reference_forward in float64 and its float32 restatement), computed once per session and never changed.  numpy and the package
only: no GPU.

  LONG        1024 bases (kMaxRef: 1025 positions, 17 passes of 64 lanes, the largest LDS) and its prefixes of 1023, 513, 2 and
              1 bases in one call; bands 20 and off
  WIDE        257 and 300 bases under bands of 66, 128, 130 and 200 positions: two to four passes, lo moving at nearly every block
  WIDTH       9, 10, 63 and 64 bases where the back-pointer row width min(2 * max_deviation, len + 1) switches, and max_deviation 0
  RUN_EDGE    bands of 1 to 3 whose best path takes stale hops at the last two rows of st_walk's runs of 64 blocks
  REMAINDERS  40 bases on 16 reads, one per value of nblk mod 16 (the rows staged at a time), bands 3 and off

A class is dict(posts, seqs, pairs, mds): every pair runs under every max_deviation of mds, in one call per kernel.

The cost of the definitions (reference_score and reference_trace are Python loops over cells, about 3 us a cell, and the
trace runs once per end rule) decided LONG's read lengths: the 1024-mer needs 1026 blocks and so 1.05 M cells per unbanded
pass, 13 s for the four passes of one pair, whatever the read.  Its long read is therefore about 1.1 blocks per base (1 130
blocks), not S3's 2.2: with the five prefixes on it and the 1024-mer on the two reads of 1026 blocks, LONG's unbanded
definitions take about a minute on one core, the other four classes together less than ten seconds.  The sequence lengths
are the issue's."""
import functools

import numpy as np

from nanopore_dna_storage_amd import synth
from nanopore_dna_storage_amd import trellis_score as T

OFF = 1 << 12                                                # a max_deviation above every sequence here: the band is off
ENDS = (-1, 0, 1)
NAMES = ("LONG", "WIDE", "WIDTH", "RUN_EDGE", "REMAINDERS")
K_ST_RUN = 64                                                # csrc/st_kernels.h, kStRun: the blocks of one run of st_walk
K_SC_STAGE = 16                                              # csrc/sc_kernels.h, kScStage: the posterior rows staged at a time


def _normals(rng, nblk):
    return rng.normal(-2.0, 1.0, size=(nblk, 40)).astype(np.float32)


def _long():
    rng = np.random.default_rng(61)
    seq = rng.integers(0, 4, 1024 + 60).astype(np.uint8)     # the read goes on beyond the sequence, as S3's does
    post = synth.posteriors_from_bases(seq, rng, margin=4.5, mean_extra_dwell=0.1)
    assert post.shape[0] >= 1130
    posts = [np.ascontiguousarray(post[:1130]), np.ascontiguousarray(post[:1026]), _normals(rng, 1026)]
    seqs = [seq[:n].copy() for n in (1024, 1023, 513, 2, 1)]
    pairs = [(0, s) for s in range(len(seqs))] + [(1, 0), (2, 0)]
    return dict(posts=posts, seqs=seqs, pairs=pairs, mds=(20, OFF))


WIDE_MDS = (33, 64, 65, 100)                                 # 66, 128, 130 and 200 positions


def _wide():
    rng = np.random.default_rng(67)
    seqs = [rng.integers(0, 4, n).astype(np.uint8) for n in (257, 300)]
    posts = [synth.posteriors_from_bases(s, rng, margin=4.5, mean_extra_dwell=1.2) for s in seqs]
    return dict(posts=posts, seqs=seqs, pairs=[(0, 0), (1, 1)], mds=WIDE_MDS)


WIDTH_LENGTHS = (9, 10, 63, 64)


def width_mds(n):
    """the max_deviation values with 2 * md in {n, n + 1, n + 2}"""
    return sorted({v // 2 for v in (n, n + 1, n + 2) if v % 2 == 0})


def _width():
    """every sequence on a read made from it and on one of random normals with len + 2 blocks, the fewest; every sequence
    under every max_deviation that any of them switches at (so below, at and above the switch), and under 0"""
    rng = np.random.default_rng(71)
    seqs = [rng.integers(0, 4, n).astype(np.uint8) for n in WIDTH_LENGTHS]
    posts = []
    for s in seqs:
        post = synth.posteriors_from_bases(s, rng, margin=4.0, mean_extra_dwell=1.2)
        if post.shape[0] < len(s) + 2:
            post = np.concatenate([post, _normals(rng, len(s) + 2 - post.shape[0])])
        posts += [np.ascontiguousarray(post, np.float32), _normals(rng, len(s) + 2)]
    mds = (0,) + tuple(sorted({md for n in WIDTH_LENGTHS for md in width_mds(n)}))
    return dict(posts=posts, seqs=seqs, pairs=[(r, r // 2) for r in range(len(posts))], mds=mds)


# RUN_EDGE: (seed, bases, blocks, max_deviation), searched on the CPU over seeds 0..399 with walk_runs below and frozen: the
# best path of each under its max_deviation has stale hops, and across them the four conditions of run_edge_conditions hold
RUN_EDGE_FROZEN = ((0, 100, 200, 1), (0, 110, 230, 3), (1, 110, 230, 2), (0, 120, 260, 3))


def run_edge_read(seed, n, nblk):
    rng = np.random.default_rng(seed)
    seq = rng.integers(0, 4, n).astype(np.uint8)
    post = synth.posteriors_from_bases(seq, rng, margin=3.0, mean_extra_dwell=1.2)
    assert post.shape[0] >= nblk >= 200
    return np.ascontiguousarray(post[:nblk]), seq


def _run_edge(frozen=RUN_EDGE_FROZEN):
    """every frozen read with its own sequence, all of them under each of the frozen max_deviation values"""
    made = {}
    for seed, n, nblk, _ in frozen:
        made.setdefault((seed, n, nblk), run_edge_read(seed, n, nblk))
    keys = list(made)
    return dict(posts=[made[k][0] for k in keys], seqs=[made[k][1] for k in keys], pairs=[(i, i) for i in range(len(keys))],
                mds=tuple(sorted({md for *_, md in frozen})), frozen=[(keys.index(k[:3]), k[3]) for k in frozen])


def walk_runs(enter, nblk, max_deviation):
    """st_walk's run arithmetic replayed on a path of the definition (enter as reference_trace gives it): from t = nblk - 1
    backwards in runs of min(64, t + 1) rows; row u of a run is block t - u, where the path stands at positions_after(...)[t - u];
    outside that block's band the hop is stale and adds 2 to u, any other block adds 1; the next run starts at t - u.
    -> [(u, nrows, run)] of every stale hop, run counted from the read's end"""
    bands = T.band_table(nblk, len(enter) + 1, max_deviation)
    at = T.positions_after(enter, nblk)
    hops, t, run = [], nblk - 1, 0
    while t >= 0:
        nrows, u = min(K_ST_RUN, t + 1), 0
        while u < nrows:
            lo, hi = bands[t - u]
            if lo <= at[t - u] < hi:
                u += 1
            else:
                hops.append((u, nrows, run))
                u += 2
        t -= u
        run += 1
    return hops


def run_edge_conditions(c=None):
    """the four conditions on RUN_EDGE's frozen cases -> dict of bools, and asserts that the replay counts the definition's
    stale hops on every one"""
    c = klass("RUN_EDGE") if c is None else c
    us, short, runs3 = set(), False, False
    for k, md in c["frozen"]:
        r, s = c["pairs"][k]
        w = T.reference_trace(c["posts"][r], c["seqs"][s], md)
        hops = walk_runs(w["enter"], len(c["posts"][r]), md) if w["end_state"] >= 0 else []
        assert len(hops) == w["n_stale"]
        us |= {u for u, _, _ in hops}
        short |= any(nrows < K_ST_RUN for _, nrows, _ in hops)
        runs3 |= len({run for _, _, run in hops}) >= 3
    return dict(hop_at_u63=K_ST_RUN - 1 in us, hop_at_u62=K_ST_RUN - 2 in us, hop_in_a_short_run=short, three_runs_with_a_hop=runs3)


def _remainders():
    rng = np.random.default_rng(73)
    seq = rng.integers(0, 4, 40).astype(np.uint8)
    posts = []
    for nblk in range(90, 106):
        post = synth.posteriors_from_bases(seq, rng, margin=3.0, mean_extra_dwell=1.6)
        while post.shape[0] < nblk:
            post = synth.posteriors_from_bases(seq, rng, margin=3.0, mean_extra_dwell=1.6)
        posts.append(np.ascontiguousarray(post[:nblk]))
    return dict(posts=posts, seqs=[seq], pairs=[(r, 0) for r in range(16)], mds=(3, OFF))


@functools.lru_cache(maxsize=None)
def klass(name):
    """-> dict(posts, seqs, pairs, mds) of a class, with what the class itself promises asserted"""
    c = dict(LONG=_long, WIDE=_wide, WIDTH=_width, RUN_EDGE=_run_edge, REMAINDERS=_remainders)[name]()
    for r, s in c["pairs"]:
        assert len(c["posts"][r]) >= len(c["seqs"][s]) + 2
    if name == "LONG":
        assert [len(s) for s in c["seqs"]] == [1024, 1023, 513, 2, 1] and len(c["posts"][2]) == 1024 + 2 == len(c["posts"][1])
    if name == "WIDE":
        for r, s in c["pairs"]:
            for md in c["mds"]:
                assert wide_band(c, r, s, md)[1] >= 100
    if name == "WIDTH":                                      # max_deviation 0: every band is empty, no end score, no path
        for r, s in c["pairs"]:
            w = T.reference_trace(c["posts"][r], c["seqs"][s], 0)
            assert T.reference_score(c["posts"][r], c["seqs"][s], 0) == (T.NEG, T.NEG) == w["score"]
            assert w["end_state"] == -1 and (w["enter"] == -1).all() and (w["kind"] == 255).all()
            assert T.reference_forward(c["posts"][r], c["seqs"][s], 0) == (-np.inf, -np.inf)
    if name == "RUN_EDGE":
        assert all(run_edge_conditions(c).values())
    if name == "REMAINDERS":
        assert sorted(len(p) % K_SC_STAGE for p in c["posts"]) == list(range(K_SC_STAGE))
    return c


def wide_band(c, r, s, md):
    """-> (the widest band of the pair's blocks, the number of distinct lo over them)"""
    bands = T.band_table(len(c["posts"][r]), len(c["seqs"][s]) + 1, md)
    return int((bands[:, 1] - bands[:, 0]).max()), len(set(bands[:, 0].tolist()))


@functools.lru_cache(maxsize=None)
def want(name, md):
    """the definitions on every pair of a class under one max_deviation, once: -> dict(score float32 [n, 2], trace {end: [dict per
    pair]}, f64 [n, 2], f32 [n, 2])"""
    c = klass(name)
    on = [(c["posts"][r], c["seqs"][s]) for r, s in c["pairs"]]
    return dict(score=np.array([T.reference_score(p, s, md) for p, s in on], np.float32),
                trace={end: [T.reference_trace(p, s, md, end=end) for p, s in on] for end in ENDS},
                f64=np.array([T.reference_forward(p, s, md) for p, s in on], np.float64),
                f32=np.array([T.reference_forward(p, s, md, dtype=np.float32) for p, s in on], np.float32))


def counts(name, md):
    """what a class holds under one max_deviation: pairs, pairs with a finite end score, flop entries and stale hops on the
    paths of end = -1"""
    w = want(name, md)
    tr = w["trace"][-1]
    return dict(pairs=len(tr), finite=int(np.isfinite(w["score"]).any(axis=1).sum()),
                flops=int(sum((t["kind"] == 1).sum() for t in tr)), stale=int(sum(t["n_stale"] for t in tr)))


def trace_width(md, n):
    """the back-pointer row width of a sequence of n bases: w = min(2 * md, n + 1) (trace_width, csrc/lva_stages.cpp)"""
    return min(2 * md, n + 1)
