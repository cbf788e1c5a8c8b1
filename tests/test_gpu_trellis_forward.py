"""The forward score on the GPU (csrc/fw_kernels.hip through Decoder.forward_bases / forward_bases_resident /
forward_messages), held to trellis_score.reference_forward in float64.  A floating-point stage, so the yardstick is rule (A) of
tests/test_gpu_transpost.py: E_gpu(S) <= 2 E_f32(S), E the largest |x - float64| over the pairs and both states of a case
class S, E_f32 that of the definition's own float32 restatement (the same term order, every addition rounded to float32; the
device's expf / logf are specified to about twice glibc's error, which is what the factor 2 is for).  Both -inf counts as 0,
one -inf beside a finite value as a failure.  tests/test_trellis_forward_host.py checks on the CPU that E_f32 is not 0 on any
class.  Bit for bit where the definition leaves no rounding to choose: posteriors with a single path give score_bases' bits.

Single pairs on tiny shapes are held to a worst-case bound instead (_bound): E_f32 of one pair of a few blocks can be 0 or
small by luck, and twice that is no yardstick.

Measured once (one MI355X): E_gpu = E_f32 on every class -- S1 6.57e-4, S2 4.5e-4, S3 6.59e-3."""
import io

import numpy as np
import pytest

import nanopore_dna_storage_amd as pkg
from nanopore_dna_storage_amd import _lib, synth
from nanopore_dna_storage_amd import trellis_score as T
from trellis_forward_cases import NEG, OFF, SINGLE_PATH_SIZES, err, klass, narrow, single_path

pytestmark = pytest.mark.gpu

ARG, TOO_SHORT = -10, -6


def same_bits(a, b):
    return np.asarray(a, np.float32).tobytes() == np.asarray(b, np.float32).tobytes()


@pytest.fixture(scope="module")
def dec():
    with pkg.Decoder(6, 1, 60, list_size=4, max_deviation=20, device=0, max_slots=4) as d:
        yield d


def _rule_a(name, got, c):
    e_gpu = err(got, c["f64"])
    print("%s: E_gpu = %.3g, E_f32 = %.3g over %d pairs" % (name, e_gpu, c["e_f32"], len(c["pairs"])))
    assert got.dtype == np.float32 and got.shape == c["f64"].shape
    assert c["e_f32"] > 0 and e_gpu <= 2 * c["e_f32"], (name, "A", e_gpu, c["e_f32"])


def test_rule_a_reads_of_the_benchmark_code_with_true_and_wrong_messages():
    c = klass("S1")
    with pkg.Decoder(*c["code"], list_size=8, max_deviation=c["md"], device=0, max_slots=2) as d:
        got = d.forward_messages(c["posts"], c["msgs"], c["pairs"])             # the decoder's own band
        assert same_bits(got, d.forward_bases(c["posts"], c["seqs"], c["pairs"]))
    _rule_a("S1", got, c)
    tot = T.forward_total(got)
    assert (tot[:8] > tot[8:]).all()                                            # the truth outweighs its neighbour on every read


def test_rule_a_at_the_pass_boundaries(dec):
    c = klass("S2")
    assert sorted({len(s) for s in c["seqs"]}) == [63, 64, 65, 129]
    assert {c["posts"][r].shape[0] - len(c["seqs"][s]) for r, s in c["pairs"]} >= {2}
    _rule_a("S2", dec.forward_bases(c["posts"], c["seqs"], c["pairs"], max_deviation=c["md"]), c)


def test_rule_a_longest_sequence_in_a_window_of_a_resident_buffer(dec):
    c = klass("S3")
    pad = synth.posteriors_from_bases(np.array([0, 1, 2, 3] * 3, np.uint8), np.random.default_rng(6))
    assert len(c["seqs"][0]) == 1024 and c["posts"][0].shape[0] == 2200
    with dec.resident([pad] + c["posts"] + [pad]) as (dev, off):
        assert off[1] > 0
        got = dec.forward_bases_resident(dev, off[1:2], np.diff(off)[1:2], c["seqs"], c["pairs"], max_deviation=c["md"])
    _rule_a("S3", got, c)


@pytest.mark.parametrize("n, nblk", SINGLE_PATH_SIZES)
def test_single_path_gives_the_bits_of_the_score(dec, n, nblk):
    c = single_path(n, nblk)
    live = c["end_state"]
    fw = dec.forward_bases([c["post"]], [c["seq"]], [(0, 0)], max_deviation=OFF)[0]
    sc = dec.score_bases([c["post"]], [c["seq"]], [(0, 0)], max_deviation=OFF)[0]
    assert same_bits(sc, c["score"]) and np.isfinite(sc[live])
    assert same_bits(fw[live], sc[live]) and fw[1 - live] == NEG, (fw, sc)


def _bound(f64, nblk):
    """What float32 can lose on one pair at worst, device and restatement alike: per block a cell takes two roundings of a
    value (the addition of the posterior, the addition of the log: half a spacing of the value each) and the error of logf and
    of the expf under it (a unit of a logarithm below log 8 each, together below 1e-6); the values grow in size towards the
    result, so the spacing of the largest result stands for every block's."""
    return nblk * (float(np.spacing(np.float32(np.abs(f64[np.isfinite(f64)]).max()))) + 1e-6)


def _one(dec, post, seq, md):
    """one pair on the device beside the definition: -> (device, float64, the worst-case bound, the restatement's error)"""
    got = dec.forward_bases([post], [seq], [(0, 0)], max_deviation=md)[0]
    f64 = np.array(T.reference_forward(post, seq, md), np.float64)
    e32 = err(T.reference_forward(post, seq, md, dtype=np.float32), f64)
    assert np.isfinite(f64).any() and e32 <= _bound(f64, len(post))             # the bound holds for the restatement
    return got, f64, _bound(f64, len(post)), e32


@pytest.mark.parametrize("n, nblk", [(1, 3), (2, 4), (10, 15), (10, 16), (10, 17), (10, 32), (10, 33)])
def test_smallest_shapes_and_the_staged_chunk_edges(dec, n, nblk):
    rng = np.random.default_rng(10 * n + nblk)
    seq = rng.integers(0, 4, n).astype(np.uint8)
    post = rng.normal(-2.0, 1.0, size=(nblk, 40)).astype(np.float32)
    for md in (OFF, 3):
        got, f64, tol, e32 = _one(dec, post, seq, md)
        print(n, nblk, md, got.tolist(), f64.tolist(), "E_gpu %.3g E_f32 %.3g bound %.3g" % (err(got, f64), e32, tol))
        assert err(got, f64) <= tol


@pytest.mark.parametrize("md", [1, 2])
def test_band_narrower_than_a_pass_is_cleared_on_read(dec, md):
    post, seq = narrow()
    got, f64, tol, e32 = _one(dec, post, seq, md)
    sc = dec.score_bases([post], [seq], [(0, 0)], max_deviation=md)[0]
    print(md, got.tolist(), f64.tolist(), sc.tolist(), "E_gpu %.3g E_f32 %.3g bound %.3g" % (err(got, f64), e32, tol))
    assert err(got, f64) <= tol
    assert same_bits(sc, T.reference_score(post, seq, md))
    assert err(got, sc) > tol + 1e-2                                            # else the case shows nothing


def test_dead_rows_give_minus_inf_not_nan(dec):
    post, seq = narrow()
    dead = post.copy()
    dead[40:43] = NEG
    for md in (2, OFF):
        got = dec.forward_bases([dead, post], [seq], [(0, 0), (1, 0)], max_deviation=md)
        assert same_bits(got[0], [NEG, NEG]) and np.isfinite(got[1]).any() and not np.isnan(got).any()
    part = post.copy()
    part[40, [0, 9, 18, 27, 36, 37, 38, 39]] = NEG                              # a block that forbids every stay
    got, f64, tol, _ = _one(dec, part, seq, OFF)
    assert err(got, f64) <= tol


def test_same_numbers_by_three_routes():
    code = (6, 1, 60)
    reads = [synth.make_read(*code, 40 + i, rc=bool(i & 1), margin=4.0, sub=0.01, dele=0.01) for i in range(4)]
    posts, rc = [x["post"] for x in reads], [x["rc"] for x in reads]
    msgs = np.array([x["msg"] for x in reads], np.uint8)
    pairs = [(r, m) for r in range(4) for m in range(4) if (r + m) % 3 != 1]    # a message on several reads, both flags
    with pkg.Decoder(*code, list_size=4, max_deviation=20, device=0, max_slots=4) as d:
        a = d.forward_messages(posts, msgs, pairs, rc=rc)
        seqs = [T.message_bases(*code, msgs[m], rc[r]) for r, m in pairs]
        own = [(r, k) for k, (r, _) in enumerate(pairs)]
        b = d.forward_bases(posts, seqs, own)
        with d.resident(posts) as (dev, off):
            c = d.forward_bases_resident(dev, off[:-1], np.diff(off), seqs, own)
        order = np.random.default_rng(2).permutation(len(pairs))
        shuffled = d.forward_messages(posts, msgs, [pairs[i] for i in order], rc=rc)
    assert a.shape == (len(pairs), 2) and np.isfinite(a).any(axis=1).all()
    assert same_bits(a, b) and same_bits(a, c) and same_bits(shuffled, a[order])
    assert len({m for _, m in pairs}) < len(pairs) and len(set(rc)) == 2
    tot = T.forward_total(a)
    for r in range(4):                                                          # the read's own message outweighs the others
        mine = {m: tot[k] for k, (rr, m) in enumerate(pairs) if rr == r}
        if r in mine:
            assert max(mine, key=mine.get) == r


def test_contract_of_the_score_calls(dec):
    x = synth.make_read(6, 1, 60, 9, margin=4.0)
    post, seq = x["post"], x["oligo"]
    before = dec.decode([post])
    good = dec.forward_bases([post], [seq], [(0, 0)])
    assert np.isfinite(good).any()
    refused = [
        (ARG, dict(pairs=[(1, 0)])), (ARG, dict(pairs=[(-1, 0)])), (ARG, dict(pairs=[(0, 1)])), (ARG, dict(pairs=[(0, -1)])),
        (ARG, dict(seqs=[np.zeros(1025, np.uint8)])),
        (ARG, dict(seqs=[np.zeros(0, np.uint8)])),
        (ARG, dict(seqs=[np.zeros(1025, np.uint8)], posts=[post[:10]])),        # the sequence is judged before the window
        (TOO_SHORT, dict(posts=[post[:len(seq) + 1]])),
    ]
    for code, change in refused:
        a = dict(posts=[post], seqs=[seq], pairs=[(0, 0)])
        a.update(change)
        with pytest.raises(pkg.LvaError) as e:
            dec.forward_bases(a["posts"], a["seqs"], a["pairs"])
        assert e.value.code == code, (change, e.value.code)
        with dec.resident(a["posts"]) as (dev, off):
            with pytest.raises(pkg.LvaError) as e:
                dec.forward_bases_resident(dev, off[:-1], np.diff(off), a["seqs"], a["pairs"])
        assert e.value.code == code, (change, e.value.code)
        assert same_bits(dec.forward_bases([post], [seq], [(0, 0)]), good)
    # a base code above 3 (the Python layer refuses it first: through the C ABI), and nothing written for a refused call
    import ctypes
    bases, first, lens = np.array([0, 1, 4], np.uint8), np.zeros(1, np.int64), np.array([3], np.int32)
    pr, out, off = np.zeros(2, np.int32), np.full(2, 7.0, np.float32), np.array([0, len(post)], np.int64)
    flat = np.ascontiguousarray(post)
    call = lambda: dec._L.lva_forward_bases(dec._h, flat.ctypes.data, off.ctypes.data, 1, bases.ctypes.data, first.ctypes.data,
                                            lens.ctypes.data, 1, pr.ctypes.data, 1, ctypes.c_uint32(20), out.ctypes.data)
    assert call() == ARG and out.tolist() == [7.0, 7.0]
    bases[2] = ord("T")
    want = np.array(T.reference_forward(post, [0, 1, 3], 20))
    assert call() == 0 and err(out, want) <= _bound(want, len(post))
    # BUSY while a stream is open, after the call's own arguments
    with dec.stream():
        with pytest.raises(pkg.LvaError) as e:
            dec.forward_bases([post], [seq], [(0, 0)])
        assert e.value.code == _lib.ERR_BUSY
        with pytest.raises(pkg.LvaError) as e:
            dec.forward_bases([post], [seq], [(0, 1)])
        assert e.value.code == ARG
    # exactly npos + 1 blocks is taken, no pair is a no-op, and the decoder decodes as before
    assert np.isfinite(dec.forward_bases([post[:len(seq) + 2]], [seq], [(0, 0)])).any()
    assert dec.forward_bases([post], [seq], []).shape == (0, 2)
    assert same_bits(dec.forward_bases([post], [seq], [(0, 0)]), good)
    after = dec.decode([post])
    assert np.array_equal(before[0][0], after[0][0]) and same_bits(before[0][1], after[0][1])


def test_the_use_list_posterior_and_the_tool(tmp_path):
    code, L, md, n, seed = (6, 1, 60), 8, 20, 16, 3
    kw = dict(sub=0.05, dele=0.03, ins=0.01)
    with pkg.Decoder(*code, list_size=L, max_deviation=md, device=0) as d:
        def after(dev, off, truth, results, rc):
            fb, nb = off[:-1], np.diff(off)
            return (T.truth_rows(d, dev, fb, nb, results, truth["msgs"], rc, forward=True), T.list_rows(d, dev, fb, nb, results, rc),
                    T.truth_rows(d, dev, fb, nb, results, truth["msgs"], rc), d.download(dev, off), rc)
        truth, results, (rows, lists, plain, posts, rc) = d.simulate_and_decode(n, seed, after=after, **kw)
    assert len(rows) == len(lists) == n
    got, f64, f32 = [], [], []
    for i, (row, lst, res) in enumerate(zip(rows, lists, results)):
        assert {k: repr(v) for k, v in row.items() if k not in ("fwd_truth", "fwd_first", "fwd_best", "conf_first", "trace")} == \
               {k: repr(v) for k, v in plain[i].items() if k != "trace"}          # the default output is unchanged
        count = 0 if isinstance(res, int) else len(res[0])
        assert len(lst["totals"]) == len(lst["posterior"]) == len(lst["order"]) == count
        if not count:
            assert row["fwd_best"] == -1 and np.isnan(row["conf_first"])
            continue
        assert abs(lst["posterior"].sum() - 1.0) < 1e-6
        assert row["fwd_best"] == int(np.argmax(lst["totals"])) == int(lst["order"][0])
        assert row["fwd_first"] == lst["totals"][0] and row["conf_first"] == lst["posterior"][0]
        if row["rank"] >= 0:
            assert row["fwd_truth"] == lst["totals"][row["rank"]]                # the same call, the same sequence: the same bits
        flag = bool(rc[i]) if rc is not None else False
        for m in res[0]:
            seq = T.message_bases(*code, m, flag)
            f64.append(T.forward_total([T.reference_forward(posts[i], seq, md)])[0])
            f32.append(T.forward_total([T.reference_forward(posts[i], seq, md, dtype=np.float32)])[0])
        got += lst["totals"].tolist()
    e_gpu, e_f32 = err(got, f64), err(f32, f64)
    print("lists: %d entries, E_gpu = %.3g, E_f32 = %.3g" % (len(got), e_gpu, e_f32))
    assert len(got) >= 4 * L and e_f32 > 0 and e_gpu <= 2 * e_f32
    # the command line: the four columns and the extended summary line
    prefix, out = str(tmp_path / "t"), io.StringIO()
    argv = ["--simulate", str(n), "--seed", str(seed), "--mem_conv", "6", "--rate", "1", "--msg_len", "60", "--list_size", str(L),
            "--max_deviation", str(md), "--sub", "0.05", "--dele", "0.03", "--ins", "0.01", "--forward", "--out", prefix]
    assert T.main(argv, out=out) == 0
    lines = open(prefix + ".truth.tsv").read().splitlines()
    assert lines[0].split("\t")[-4:] == ["fwd_truth", "fwd_first", "fwd_best", "conf_first"] and len(lines) == n + 1
    cells = [ln.split("\t") for ln in lines[1:]]
    assert [int(c[-2]) for c in cells] == [r["fwd_best"] for r in rows]
    assert [c[-4] for c in cells] == [repr(r["fwd_truth"]) for r in rows]
    assert out.getvalue().strip() == T.summary_line(rows, forward=True)
    assert out.getvalue().strip().endswith("fwd_best != 0 %d, truth first by forward only %d" % T.forward_counts(rows))
