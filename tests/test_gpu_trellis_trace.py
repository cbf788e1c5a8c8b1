"""The traceback of the one-message trellis on the GPU (csrc/st_kernels.hip through Decoder.trace_bases /
trace_bases_resident / trace_messages): every output array byte for byte trellis_score.reference_trace, the scores also
lva_score_bases' on the same pairs -- sequence lengths around the 64-lane pass, block counts around the staged rows, bands of
1, 2, 10 and none, homopolymers, ties, -inf, pairs without a path, stale hops, the three end rules, mixed and shuffled pairs
with the stride tail, chunked scratch; the property that ties dev_needed to the banded score on simulated reads; the tool."""
import io

import numpy as np
import pytest

import nanopore_dna_storage_amd as pkg
from nanopore_dna_storage_amd import synth
from nanopore_dna_storage_amd import trellis_score as T
from trellis_score_cases import INVARIANT, INVARIANT_RUNS, case
from trellis_trace_cases import same_trace, truth_seq

pytestmark = pytest.mark.gpu

ARG = -10
NEG = np.float32(-np.inf)
OFF = 2000                                                   # a max_deviation beyond every sequence here: the band is off
BANDS = (1, 2, 10, OFF)


@pytest.fixture(scope="module")
def dec():
    with pkg.Decoder(6, 1, 60, list_size=4, max_deviation=20, device=0, max_slots=4) as d:
        yield d


def _reads():
    """-> (posts, seqs, pairs, names): reads with the sequence they were made from, and pairs across them"""
    rng = np.random.default_rng(11)
    posts, seqs, names = [], [], []

    def add(name, seq, post):
        names.append(name)
        seqs.append(np.asarray(seq, np.uint8))
        if post.shape[0] < len(seq) + 2:                     # (a made read of one or two bases can be too short to score)
            post = np.concatenate([post, rng.normal(-2, 1, size=(len(seq) + 2 - post.shape[0], 40))])
        posts.append(np.ascontiguousarray(post, np.float32))

    for n in (1, 2, 63, 64, 65, 130):                        # the 64-lane pass boundary; 130 unbanded: a band of three passes
        seq = rng.integers(0, 4, size=n).astype(np.uint8)
        add("len%d" % n, seq, synth.posteriors_from_bases(seq, rng, margin=4.0))
    run = np.array([0, 1, 1, 1, 2, 2, 3, 0, 0, 0, 0, 1], np.uint8)      # homopolymer runs: the only way into a flop by a step
    add("runs", run, synth.posteriors_from_bases(run, rng, margin=4.0))
    add("all_equal", np.full(12, 2, np.uint8), synth.posteriors_from_bases(np.full(12, 2, np.uint8), rng, margin=4.0))
    add("no_repeat", np.arange(12) % 4, synth.posteriors_from_bases((np.arange(12) % 4).astype(np.uint8), rng, margin=4.0))
    add("min_blocks", [3, 1, 1, 0, 2], rng.normal(-2, 1, size=(7, 40)))                 # len + 2 blocks, the fewest
    for nblk in (15, 16, 17, 33):                            # around the rows staged at a time (kScStage = 16)
        add("blocks%d" % nblk, rng.integers(0, 3, size=13), rng.normal(-2, 1, size=(nblk, 40)))
    add("short_on_long", [0, 0, 1], rng.normal(-2, 1, size=(150, 40)))                   # more than two runs of the walk, few entries
    add("zeros", [0, 0, 1, 2, 2, 2], np.zeros((20, 40)))    # everything ties
    holes = rng.normal(-2, 1, size=(40, 40))
    holes[rng.random(holes.shape) < 0.15] = -np.inf         # -inf entries: some candidates, some cells, maybe the end
    add("holes", rng.integers(0, 4, size=9), holes)
    dead = rng.normal(-2, 1, size=(30, 40))
    dead[14] = -np.inf                                       # a block that forbids everything: no path with the band off
    add("dead_row", rng.integers(0, 4, size=8), dead)
    pairs = [(i, i) for i in range(len(seqs))]
    for r, s in ((2, 0), (2, 1), (2, 6), (5, 3), (5, 7), (15, 9), (15, 6), (3, 2), (0, 0)):      # several per read, other lengths
        assert posts[r].shape[0] >= len(seqs[s]) + 2
        pairs.append((r, s))
    order = np.random.default_rng(2).permutation(len(pairs))
    return posts, seqs, [pairs[i] for i in order], names


READS = _reads()
_want = {}


def want(k, md, end):
    """the definition's answer for pair k, once"""
    posts, seqs, pairs, _ = READS
    if (k, md, end) not in _want:
        r, s = pairs[k]
        _want[(k, md, end)] = T.reference_trace(posts[r], seqs[s], md, end=end)
    return _want[(k, md, end)]


@pytest.mark.parametrize("end", [-1, 0, 1])
@pytest.mark.parametrize("md", BANDS)
def test_device_is_the_definition(dec, md, end):
    posts, seqs, pairs, names = READS
    got = dec.trace_bases(posts, seqs, pairs, max_deviation=md, end=end)
    assert got["enter"].shape == (len(pairs), 130) and got["kind"].shape == (len(pairs), 130)
    paths = stale = none = flops = 0
    for k, (r, s) in enumerate(pairs):
        w = want(k, md, end)
        assert same_trace(got, k, w, len(seqs[s])), (names[r], names[s], md, end, w,
                                                      {key: got[key][k][:len(seqs[s])] for key in got})
        paths += w["end_state"] >= 0
        none += w["end_state"] < 0
        stale += w["n_stale"] > 0
        flops += int((w["kind"] == 1).sum())
    print("md", md, "end", end, "pairs", len(pairs), "with a path", paths, "without", none, "with stale hops", stale, "flops", flops)
    assert np.asarray(got["score"]).tobytes() == dec.score_bases(posts, seqs, pairs, max_deviation=md).tobytes()
    assert paths > 0 and flops > 0                           # (what the cases hold was counted on the CPU when they were chosen)
    if md >= 10:                                             # (a narrow band's stale cells carry a path past the dead row)
        assert none > 0
    if md == 10:
        assert stale > 0


def test_ties_follow_the_tie_rule_and_a_dead_row_leaves_no_path(dec):
    posts, seqs, pairs, names = READS
    got = dec.trace_bases(posts, seqs, pairs, max_deviation=OFF)
    k = pairs.index((names.index("zeros"), names.index("zeros")))
    assert got["score"][k].tolist() == [0.0, NEG] and got["end_state"][k] == 0 and same_trace(got, k, want(k, OFF, -1), 6)
    k = pairs.index((names.index("dead_row"), names.index("dead_row")))
    assert got["score"][k].tolist() == [NEG, NEG] and got["end_state"][k] == -1 and got["start_state"][k] == -1
    assert (got["enter"][k] == -1).all() and (got["kind"][k] == 255).all() and got["n_stale"][k] == 0


def test_stale_band_fixture_and_the_decoders_own_band():
    c = case("m8_r3_L8_edge0")                               # the stale-hop case of tests/test_trellis_trace_host.py
    seq = truth_seq(c)
    w = T.reference_trace(c["post"], seq, c["md"])
    assert w["n_stale"] > 0 and w["end_state"] >= 0
    with pkg.Decoder(*c["code"], list_size=2, max_deviation=c["md_arg"], device=0, max_slots=2) as d:
        got = d.trace_bases([c["post"]], [seq], [(0, 0)])   # max_deviation None: the decoder's
    print("n_stale", w["n_stale"], int(got["n_stale"][0]))
    assert same_trace(got, 0, w, len(seq))


def _need(posts, seqs, pairs, md):
    return [(posts[r].shape[0] * min(2 * md, len(seqs[s]) + 1) + 15) // 16 * 16 for r, s in pairs]


@pytest.mark.parametrize("md", [10, OFF])
def test_chunks_change_nothing(dec, md):
    posts, seqs, pairs, _ = READS
    need = _need(posts, seqs, pairs, md)
    limit = max(need)
    assert sum(need) > 2 * limit                             # at least three chunks
    whole = dec.trace_bases(posts, seqs, pairs, max_deviation=md)
    cut = dec.trace_bases(posts, seqs, pairs, max_deviation=md, scratch_limit=limit)
    for key in whole:
        assert whole[key].tobytes() == cut[key].tobytes(), key
    with pytest.raises(pkg.LvaError) as e:
        dec.trace_bases(posts, seqs, pairs, max_deviation=md, scratch_limit=limit - 1)
    assert e.value.code == ARG
    small = [k for k, n in enumerate(need) if n < limit]     # without the largest pair the same limit is enough
    again = dec.trace_bases(posts, seqs, [pairs[k] for k in small], max_deviation=md, scratch_limit=limit - 1)
    assert again["enter"].tobytes() == whole["enter"][small].tobytes()


def test_resident_windows_agree_with_host_posteriors(dec):
    posts, seqs, pairs, _ = READS
    host = dec.trace_bases(posts, seqs, pairs, max_deviation=10, end=1)
    pad = np.zeros((5, 40), np.float32)
    with dec.resident([pad] + posts + [pad]) as (dev, off):
        res = dec.trace_bases_resident(dev, off[1:-2], np.diff(off)[1:-1], seqs, pairs, max_deviation=10, end=1)
    for key in host:
        assert host[key].tobytes() == res[key].tobytes(), key


def test_trace_messages_is_trace_bases_on_message_bases(dec):
    cs = [case("m6_r1_L4_sync_rc"), case("m6_r1_L4_indel")]  # (the code without its marker: any message is a message)
    msgs = np.array([pkg.str_to_bits(c["m"]["message"]) for c in cs], np.uint8)
    posts, rc = [c["post"] for c in cs], [True, False]
    pairs = np.array([[0, 0], [1, 1], [0, 1], [1, 0]], np.int32)
    kept = pairs.copy()
    got = dec.trace_messages(posts, msgs, pairs, rc=rc)
    assert np.array_equal(pairs, kept)
    seqs = [T.message_bases(6, 1, 60, msgs[m], rc[r]) for r, m in pairs]
    direct = dec.trace_bases(posts, seqs, [(r, k) for k, (r, _) in enumerate(pairs)])
    for key in got:
        assert got[key].tobytes() == direct[key].tobytes(), key
    for k, (r, m) in enumerate(pairs):
        assert same_trace(got, k, T.reference_trace(posts[r], seqs[k], 20), len(seqs[k]))
    assert got["end_state"][0] >= 0 and got["end_state"][1] >= 0


def test_refusals_in_order_and_the_decoder_stays_usable(dec):
    import ctypes
    posts, seqs, _, names = READS
    i = names.index("runs")
    post, seq = posts[i], seqs[i]
    good = dec.trace_bases([post], [seq], [(0, 0)])
    for code, kw in ((ARG, dict(pairs=[(1, 0)])), (ARG, dict(seqs=[np.zeros(1025, np.uint8)])), (-6, dict(posts=[post[:len(seq) + 1]])),
                     (ARG, dict(end=2)), (ARG, dict(end=-2)), (ARG, dict(scratch_limit=16))):
        a = dict(posts=[post], seqs=[seq], pairs=[(0, 0)])
        a.update(kw)
        with pytest.raises(pkg.LvaError) as e:
            dec.trace_bases(**a)
        assert e.value.code == code, (kw, e.value.code)
    # through the C ABI: the score's refusals first (a read too short wins over a bad end), then the call's own
    flat, off = np.ascontiguousarray(post), np.array([0, len(post)], np.int64)
    bases, first, lens = seq.copy(), np.zeros(1, np.int64), np.array([len(seq)], np.int32)
    pr = np.zeros(2, np.int32)
    score, info = np.zeros(2, np.float32), np.zeros(4, np.int32)
    enter, kind = np.zeros(len(seq), np.int32), np.zeros(len(seq), np.uint8)

    def call(n_blocks=len(post), end=-1, stride=len(seq), n_pairs=1, outs=None):
        o = np.array([0, n_blocks], np.int64)
        outs = outs or (score.ctypes.data, enter.ctypes.data, kind.ctypes.data, info.ctypes.data)
        return dec._L.lva_trace_bases(dec._h, flat.ctypes.data, o.ctypes.data, 1, bases.ctypes.data, first.ctypes.data, lens.ctypes.data,
                                      1, pr.ctypes.data, n_pairs, ctypes.c_uint32(20), end, ctypes.c_uint64(0), stride, *outs)

    assert call(n_blocks=len(seq) + 1, end=5) == -6
    assert call(end=5) == ARG and call(stride=len(seq) - 1) == ARG
    for missing in range(1, 4):
        outs = [score.ctypes.data, enter.ctypes.data, kind.ctypes.data, info.ctypes.data]
        outs[missing] = None
        assert call(outs=tuple(outs)) == ARG
    assert call(n_pairs=0, outs=(None, None, None, None)) == 0          # no pair: nothing is touched
    assert call() == 0 and np.array_equal(enter, good["enter"][0]) and np.array_equal(kind, good["kind"][0])
    assert dec.trace_bases([post], [seq], [])["enter"].shape[0] == 0
    assert dec.trace_bases([post], [seq], [(0, 0)])["enter"].tobytes() == good["enter"].tobytes()


def test_dev_needed_keeps_the_path_and_a_band_verdict_shows_where_it_left():
    q = INVARIANT
    kw = dict(INVARIANT_RUNS[1])
    seed = kw.pop("seed")
    n = q["n"]
    with pkg.Decoder(q["mem_conv"], q["rate"], q["msg_len"], list_size=q["list_size"], max_deviation=q["max_deviation"], device=0) as d:
        with d.simulate(n, seed, **kw) as (dev, off, truth):
            d.posteriors_resident(dev, off)
            lists = d.decode_resident(dev, off)
            first, count = off[:-1], np.diff(off)
            rows = T.truth_rows(d, dev, first, count, lists, truth["msgs"], None)
            seqs = list(T.message_bases(q["mem_conv"], q["rate"], q["msg_len"], truth["msgs"]))
            by_dev = {}
            for i, r in enumerate(rows):
                if r["trace"] is not None:
                    by_dev.setdefault(int(r["dev_needed"]), []).append(i)
            at_needed = {}
            for D, reads in sorted(by_dev.items()):
                got = d.score_bases_resident(dev, first, count, seqs, [(i, i) for i in reads], max_deviation=D)
                at_needed.update({i: np.float32(g.max()) for i, g in zip(reads, got)})
    assert len(at_needed) > n // 2
    for i, best in at_needed.items():
        print(i, rows[i]["verdict"], "dev_needed", rows[i]["dev_needed"], "left_band_at", rows[i]["left_band_at"], "banded",
              rows[i]["banded"], "unbanded", rows[i]["unbanded"], "at dev_needed", best)
        assert best >= rows[i]["unbanded"], (i, rows[i], best)
        assert (rows[i]["left_band_at"] == -1) == (rows[i]["dev_needed"] <= q["max_deviation"])
    band = [r for r in rows if r["verdict"] == "band"]
    print("band verdicts", len(band), "largest dev_needed", T.band_dev_needed(rows))
    for r in band:
        assert r["left_band_at"] >= 0 or r["banded"] == NEG, r


def test_the_tool_writes_the_new_columns_and_the_trace_file(tmp_path):
    prefix = str(tmp_path / "t")
    argv = ["--simulate", "64", "--seed", "3", "--mem_conv", "6", "--rate", "1", "--msg_len", "60", "--list_size", "4",
            "--max_deviation", "6", "--sub", "0.05", "--dele", "0.03", "--ins", "0.01", "--out", prefix, "--trace"]
    out = io.StringIO()
    assert T.main(argv, out=out) == 0
    table = [ln.split("\t") for ln in open(prefix + ".truth.tsv").read().splitlines()]
    trace = [ln.split("\t") for ln in open(prefix + ".trace.tsv").read().split("\n")[:-1]]
    assert len(table) == 65 and len(trace) == 65
    assert table[0] == ["read", "rank", "banded", "unbanded", "first", "last", "verdict", "dev_needed", "left_band_at"]
    assert trace[0] == ["read", "start_state", "end_state", "enter"]
    need = []
    for row, tr in zip(table[1:], trace[1:]):
        assert len(row) == 9 and len(tr) == 4 and row[0] == tr[0]
        if row[7] == "nan":
            assert tr[1:] == ["-1", "-1", ""] and row[8] == "-1"
            continue
        enter = [int(x) for x in tr[3].split(",")]
        assert len(enter) == 66 and enter == sorted(set(enter)) and 0 <= int(tr[1]) < 8 and tr[2] in ("0", "1")
        assert (int(row[8]) == -1) == (int(row[7]) <= 6)
        if row[6] == "band":
            need.append(int(row[7]))
    counts = {v: sum(r[6] == v for r in table[1:]) for v in T.VERDICTS}
    assert out.getvalue().strip() == ("truth score: 64 reads, " + ", ".join("%s %d" % (v, counts[v]) for v in T.VERDICTS)
                                      + ", band dev_needed %d" % (max(need) if need else 0))
