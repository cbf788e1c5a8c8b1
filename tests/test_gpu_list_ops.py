"""The list consumers on the GPU (csrc/ls_kernels.hip through lva_list_filter / lva_list_consensus / lva_list_stats)
against the host functions they stand in for -- helper.decode_list_CRC_index (pinned to the reference's own outputs by
tests/golden/crc_index_cases.json), rs_code.consensus, helper.hamming / helper.levenshtein and the block rule of
simulator.run -- and the opt-in wiring against the host paths.  Every comparison is equality of integers or bytes."""
import io
import json
import math
import os

import numpy as np
import pytest

import nanopore_dna_storage_amd as pkg
from nanopore_dna_storage_amd import decoder as decoder_mod
from nanopore_dna_storage_amd import helper, list_ops, rs_code, simulator, synth

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _entry(rng, index, bpo, pad, payload=None):
    payload = bytes(rng.integers(0, 256, size=bpo, dtype=np.uint8)) if payload is None else payload
    e = helper.attach_index_crc(int(index), payload, False)
    return e + str(int(rng.integers(2))) if pad else e


def _flip(e, k):
    return e[:k] + ("1" if e[k] == "0" else "0") + e[k + 1:]


def _junk(rng, bpo, pad):
    """a valid entry with one bit (not the pad bit) flipped: CRC-8 detects every single-bit error, so it never passes"""
    e = _entry(rng, rng.integers(4096), bpo, pad)
    return _flip(e, int(rng.integers(20 + 8 * bpo)))


def _host_filter(lists, bpo, num_oligos, pad, use=None):
    """helper.decode_list_CRC_index per read -> (index, rank, payload) arrays in the device's conventions"""
    n = len(lists)
    index, rank, payload = np.full(n, -1, np.int32), np.full(n, -1, np.int32), np.zeros((n, bpo), np.uint8)
    for i, lst in enumerate(lists):
        lst = lst if use is None else lst[:use]
        idx, pl, entry = helper.decode_list_CRC_index(lst, bpo, num_oligos, pad)
        if idx is not None:
            # the rank: decode_list_CRC_index returns the entry; the first entry that passes on its own is the same one
            r = next(k for k, e in enumerate(lst) if helper.decode_list_CRC_index([e], bpo, num_oligos, pad)[0] is not None)
            assert lst[r] == entry
            index[i], rank[i], payload[i] = idx, r, np.frombuffer(pl, np.uint8)
    return index, rank, payload


def _assert_filter(got, want):
    for g, w, name in zip(got, want, ("index", "rank", "payload")):
        assert g.dtype == w.dtype and np.array_equal(g, w), name


def test_filter_gives_the_reference_outputs_of_the_golden_file():
    with open(os.path.join(HERE, "golden", "crc_index_cases.json")) as f:
        cases = json.load(f)["filter"]
    hits = 0
    for x in cases:
        msgs, counts = list_ops.lists_to_array([x["list"]])
        index, rank, payload = list_ops.filter_lists(msgs, counts, x["bytes_per_oligo"], x["num_oligos"], pad=x["pad"])
        if x["index"] is None:
            assert index[0] == -1 and rank[0] == -1 and not payload.any() and x["entry"] is None
        else:
            assert index[0] == x["index"] and payload[0].tobytes().hex() == x["payload_hex"] and x["list"][rank[0]] == x["entry"]
            hits += 1
    assert 10 < hits < len(cases)


def _constructed(rng, bpo, pad, L, num_oligos, n=304):
    """n reads of eight kinds in turn; rows past a read's count hold VALID entries (a kernel that ignores the count accepts them)"""
    lists, counts = [], []
    spare = [_entry(rng, 0, bpo, pad) for _ in range(4)]
    pool = [_junk(rng, bpo, pad) for _ in range(256)]
    for i in range(n):
        kind = i % 8
        c = L if i % 5 else int(rng.integers(1, L + 1))          # every fifth read: a count below list_size
        lst = [pool[j] for j in rng.integers(256, size=c)]
        good = _entry(rng, rng.integers(num_oligos), bpo, pad)
        if kind == 0:
            lst[0] = good
        elif kind == 1:
            lst[min(1, c - 1)] = good
        elif kind in (2, 7):
            lst[c - 1] = good
            if kind == 7 and c > 2:                               # a second valid entry behind the first must not replace it
                lst[c - 2] = _entry(rng, rng.integers(num_oligos), bpo, pad)
        elif kind == 5:                                           # CRC fine, index out of range, in front of the accepted one
            for k in range(min(c - 1, 1 + int(rng.integers(3)))):
                lst[k] = _entry(rng, rng.integers(num_oligos, 4096), bpo, pad)
            if c > 1:
                lst[c - 1 if i % 16 == 5 else min(c - 1, 3)] = good
            else:
                lst[0] = _entry(rng, rng.integers(num_oligos, 4096), bpo, pad)
        elif kind == 6:                                           # no list: count 0 or an error code
            c, lst = (0 if i % 16 == 6 else -int(rng.integers(1, 14))), []
        lists.append(lst)
        counts.append(c)
    msg_len = 20 + 8 * bpo + int(pad)
    msgs = np.zeros((n, L, msg_len), np.uint8)
    for i, lst in enumerate(lists):
        rows = lst + [spare[(i + k) % 4] for k in range(L - len(lst))]
        msgs[i] = list_ops.bits_of("".join(rows)).reshape(L, msg_len)
    host_lists = [lst[:max(c, 0)] for lst, c in zip(lists, counts)]
    return msgs, np.array(counts, np.int32), host_lists


@pytest.mark.parametrize("L", [1, 8, 64, 65, 300])
@pytest.mark.parametrize("pad", [False, True])
@pytest.mark.parametrize("bpo", [2, 18, 29])
def test_filter_equals_the_host_filter_on_constructed_reads(bpo, pad, L):
    rng = np.random.default_rng(1000 * bpo + 10 * L + pad)
    num_oligos = 733
    msgs, counts, lists = _constructed(rng, bpo, pad, L, num_oligos)
    assert msgs.shape[2] == 20 + 8 * bpo + int(pad) and 36 <= msgs.shape[2] <= 253
    want = _host_filter(lists, bpo, num_oligos, pad)
    n = len(lists)
    # the draw: both outcomes are common, and a long list is accepted behind the first 64 entries
    assert (want[0] >= 0).sum() >= n / 2 and (want[0] < 0).sum() >= n / 4
    if L > 64:
        assert want[1].max() >= 64
    _assert_filter(list_ops.filter_lists(msgs, counts, bpo, num_oligos, pad=pad), want)
    if L > 1:                                                     # fewer entries than the counts: lst[:use]
        use = (L + 1) // 2
        cut = _host_filter(lists, bpo, num_oligos, pad, use=use)
        assert (counts > use).sum() > n / 2 and (cut[0] >= 0).any() and (cut[0] != want[0]).any()
        _assert_filter(list_ops.filter_lists(msgs, counts, bpo, num_oligos, pad=pad, list_size=use), cut)


@pytest.mark.parametrize("pad", [False, True])
@pytest.mark.parametrize("bpo", [2, 18, 29])
def test_no_single_bit_flip_of_a_valid_entry_passes(bpo, pad):
    rng = np.random.default_rng(7 + bpo)
    e = _entry(rng, 41, bpo, pad)
    bits = 20 + 8 * bpo                                           # (the pad bit is dropped before the check: not flipped)
    flips = [_flip(e, k) for k in range(bits)]
    L = 65
    lists = [flips[k:k + L] for k in range(0, bits, L)] + [[e]]
    assert all(helper.decode_list_CRC_index(lst, bpo, 4096, pad)[0] is None for lst in lists[:-1])
    msgs, counts = list_ops.lists_to_array(lists, list_size=L)
    index, rank, payload = list_ops.filter_lists(msgs, counts, bpo, 4096, pad=pad)
    assert (index[:-1] == -1).all() and (rank[:-1] == -1).all() and not payload[:-1].any()
    assert index[-1] == 41 and rank[-1] == 0


def test_every_index_once_with_4096_oligos():
    rng = np.random.default_rng(12)
    bpo, L = 18, 8
    order = rng.permutation(4096)
    lists = []
    for i, idx in enumerate(order):
        lst = [_junk(rng, bpo, False) for _ in range(L)]
        lst[i % L] = _entry(rng, idx, bpo, False)
        lists.append(lst)
    msgs, counts = list_ops.lists_to_array(lists)
    want = _host_filter(lists, bpo, 4096, False)
    assert np.array_equal(want[0], order) and np.array_equal(want[1], np.arange(4096) % L)
    _assert_filter(list_ops.filter_lists(msgs, counts, bpo, 4096), want)


# ---- consensus ----

def _first_seen(index, payload):
    d = {}
    for k, p in zip(index, payload):
        if k >= 0 and int(k) not in d:
            d[int(k)] = p.tobytes()
    return d


def _vote_cases():
    rng = np.random.default_rng(5)
    bpo = 6
    P = [bytes(rng.integers(0, 256, size=bpo, dtype=np.uint8)) for _ in range(8)]
    A, B, C = P[:3]
    cases = {}
    # index 3: A,B,B,A -> B reached 2 first; index 0: three-way tie -> the first; index 9: one vote; 1, 2, 4..8, 10, 11: never
    seq = [(3, A), (0, C), (3, B), (9, A), (0, A), (3, B), (0, B), (3, A)]
    cases["ties"] = (12, seq)
    # 300 votes on one index, three payloads 100 each in a shuffled order: more than one pass of 64 lanes, decided by who gets to 100 first
    votes = [A] * 100 + [B] * 100 + [C] * 100
    cases["long"] = (5, [(2, votes[k]) for k in rng.permutation(300)])
    # the same with a clear winner that starts late
    cases["late"] = (5, [(4, A)] * 40 + [(4, B)] * 39 + [(1, C)] + [(4, C)] * 41)
    big = []
    for _ in range(5000):
        k = int(rng.integers(-1, 733))                           # -1: a read that passed no entry
        big.append((k, P[(k * 7) % 5 + int(rng.integers(3))]))
    cases["big"] = (733, big)
    cases["one"] = (4, [(2, B)])
    cases["none"] = (16, [(-1, A)] * 70)
    out = {}
    for name, (num_oligos, seq) in cases.items():
        index = np.array([k for k, _ in seq], np.int32)
        payload = np.frombuffer(b"".join(p for _, p in seq), np.uint8).reshape(len(seq), bpo)
        out[name] = (num_oligos, index, payload)
    return out


VOTES = _vote_cases()


@pytest.mark.parametrize("name", sorted(VOTES))
def test_consensus_equals_the_reference_vote(name):
    num_oligos, index, payload = VOTES[name]
    want = dict((k, p) for k, p in rs_code.consensus([(int(k), p.tobytes()) for k, p in zip(index, payload) if k >= 0]))
    got = list_ops.consensus(index, payload, num_oligos)
    assert [k for k, _ in got] == sorted(want) and dict((k, p) for k, p in got) == want
    first = list_ops.consensus(index, payload, num_oligos, first_only=True)
    assert dict((k, p) for k, p in first) == _first_seen(index, payload) and len(first) == len(want)
    if name == "ties":
        A, B, C = (payload[i].tobytes() for i in (0, 2, 1))
        assert want == {3: B, 0: C, 9: A}
    if name == "none":
        assert got == [] and first == []
    # twice, byte for byte; the winner's count
    for fo in (False, True):
        a = list_ops.consensus_arrays(index, payload, num_oligos, first_only=fo)
        b = list_ops.consensus_arrays(index, payload, num_oligos, first_only=fo)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
        present, out, votes = a
        ref = dict((k, p) for k, p in (first if fo else got))
        assert np.nonzero(present)[0].tolist() == sorted(ref) and not votes[~present].any() and not out[~present].any()
        for k, p in ref.items():
            assert votes[k] == (payload[index == k] == np.frombuffer(p, np.uint8)).all(axis=1).sum()


# ---- statistics ----

# (191, 192, 193: ls_edit's switch from myers<3> to myers<4>, a full third ballot word; appended, so that the cases drawn for the
#  lengths before them stay what they were; 127: with 63 .. 65 and 128, 129 both sides of every word boundary of ls_edit's step)
STAT_LENS = [36, 63, 64, 65, 128, 129, 180, 255, 191, 192, 193, 127]


def _blocks(a, b, w):
    return sum(a[i * w:(i + 1) * w] != b[i * w:(i + 1) * w] for i in range(math.ceil(len(a) / w)))


@pytest.fixture(scope="module")
def stat_cases():
    """per msg_len 13 reads with lists of 4 -> {msg_len: (msgs, counts, truth, want)}; the host oracle is computed once"""
    rng = np.random.default_rng(99)
    L = 4
    out = {}
    for n in STAT_LENS:
        rnd = lambda: "".join(rng.choice(["0", "1"], size=n))
        comp = lambda s: "".join("1" if ch == "0" else "0" for ch in s)
        reads = []                                               # (truth, list or error code)
        t = rnd(); reads.append((t, [t, rnd(), rnd()]))                                         # equal, truth at rank 0
        t = rnd(); reads.append((t, [_flip(t, int(rng.integers(n))), rnd(), rnd(), t]))        # one substitution, truth at the last rank
        t = rnd(); reads.append((t, [_flip(_flip(t, 0), n - 1), rnd()]))                       # two substitutions (first and last bit), truth absent
        t = rnd(); reads.append((t, [str(int(rng.integers(2))) + t[:-1], t]))                  # shifted by one bit: insert in front, drop at the end
        t = rnd(); reads.append((t, [t[1:] + str(int(rng.integers(2))), rnd(), rnd(), rnd()]))  # shifted the other way, truth absent
        t = rnd(); reads.append((t, [comp(t), rnd(), t]))                                       # complement
        t = rnd(); reads.append((t, [rnd(), rnd(), rnd(), rnd()]))                              # random, truth absent
        t = rnd(); reads.append((t, [rnd(), rnd(), t, rnd()]))                                  # random, truth inside
        t = rnd(); reads.append((t, [rnd()]))
        t = "0" * n; reads.append((t, ["1" * n, t]))
        t = rnd(); reads.append((t, [t[:n // 2] + comp(t[n // 2:])]))                           # a burst over the second half
        reads.append((rnd(), 0))                                                                # no list
        reads.append((rnd(), -6))                                                               # an error code
        msgs = np.zeros((len(reads), L, n), np.uint8)
        counts = np.zeros(len(reads), np.int32)
        truth = np.zeros((len(reads), n), np.uint8)
        want = np.zeros(len(reads), list_ops.STAT_DTYPE)
        for i, (t, lst) in enumerate(reads):
            truth[i] = list_ops.bits_of(t)
            if isinstance(lst, int):
                counts[i] = lst
                msgs[i] = truth[i]                               # (rows past the count must not be looked at)
                want[i] = (-1,) * 6
                continue
            counts[i] = len(lst)
            msgs[i, :len(lst)] = list_ops.bits_of("".join(lst)).reshape(len(lst), n)
            msgs[i, len(lst):] = truth[i]
            want[i] = (lst[0] == t, t in lst, helper.hamming(t, lst[0]), _blocks(lst[0], t, 8), _blocks(lst[0], t, 16),
                       helper.levenshtein(t, lst[0]))
        out[n] = (msgs, counts, truth, want)
    return out


def test_stat_cases_cover_the_distances(stat_cases):
    edits = np.concatenate([w["edit"] for _, _, _, w in stat_cases.values()])
    assert len(edits) >= 100
    assert all((edits == d).any() for d in (-1, 0, 1, 2)) and (edits > 20).any()
    flags = np.concatenate([np.stack([w["top_correct"], w["list_correct"]], 1) for _, _, _, w in stat_cases.values()])
    assert {tuple(x) for x in flags.tolist()} == {(1, 1), (0, 1), (0, 0), (-1, -1)}


@pytest.mark.parametrize("msg_len", STAT_LENS)
def test_statistics_equal_the_host_functions(stat_cases, msg_len):
    msgs, counts, truth, want = stat_cases[msg_len]
    got = list_ops.list_stats(msgs, counts, truth)
    for k in list_ops.STAT_FIELDS:
        assert np.array_equal(got[k], want[k]), (k, got[k].tolist(), want[k].tolist())


# ---- the opt-in wiring ----

def _data_file(tmp_path, n=1000, seed=5):
    p = tmp_path / "myfile_1K"
    p.write_bytes(bytes(np.random.default_rng(seed).integers(0, 256, size=n, dtype=np.uint8)))
    return str(p)


def test_simulate_and_decode_device_equals_host(tmp_path):
    """the configuration of tests/test_gpu_chain.py: 1 kB file, m=8, rate 3/4, 18 bytes per oligo, 30 % RS, list 8"""
    infile = _data_file(tmp_path)
    helper.encode(data_file=infile, oligo_file=infile + ".oligos", bytes_per_oligo=18, RS_redundancy=0.3, conv_m=8, conv_r=3,
                  pad=False, out=io.StringIO())
    res = {}
    with pkg.Decoder(8, 3, 164, list_size=8, max_deviation=20) as dec:
        for mode in ("host", "device"):
            out = io.StringIO()
            r = helper.simulate_and_decode(oligo_file=infile + ".oligos", decoded_data_file=infile + "." + mode, num_reads=300,
                                           data_file_size=1000, bytes_per_oligo=18, RS_redundancy=0.3, conv_m=8, conv_r=3, pad=False,
                                           list_size=8, seed=77, margin=4.3, out=out, decoder=dec, list_ops=mode)
            res[mode] = (r, out.getvalue(), open(infile + "." + mode, "rb").read())
    assert res["host"] == res["device"]
    r = res["host"][0]
    assert 0 < r["num_success"] < 300 and 0 < r["num_unique"] <= 72


def test_simulator_device_statistics_print_the_same_text():
    argv = ["--num_trials", "20", "--list_size", "4", "--mem_conv", "6", "--rate", "1", "--msg_len", "180", "--seed", "3",
            "--margin", "3.5"]
    got = {}
    with pkg.Decoder(6, 1, 180, list_size=4, max_deviation=20) as dec:
        for mode in ("host", "device"):
            out = io.StringIO()
            stats = simulator.run(simulator.build_parser().parse_args(argv + ["--stats", mode]), out=out, decoder=dec)
            got[mode] = (out.getvalue(), stats)
    assert got["host"][0] == got["device"][0] and got["host"][1] == got["device"][1]
    assert got["host"][1]["Number total"] == 20 and "Edit distance" in got["host"][0]


def test_decode_payloads_equals_the_host_filter_on_the_decoded_lists():
    rng = np.random.default_rng(31)
    m, r, bpo, L, num_oligos = 6, 1, 4, 4, 20
    msg_len = 20 + 8 * bpo
    sent = [helper.attach_index_crc(i, bytes(rng.integers(0, 256, size=bpo, dtype=np.uint8))) for i in range(num_oligos)]
    bases = decoder_mod.encode(m, r, msg_len, np.array([[int(ch) for ch in s] for s in sent], dtype=np.uint8))
    posts = []
    for i in range(40):
        seq = synth.mutate(np.atleast_2d(bases)[i % num_oligos], rng, 0.01, 0.01, 0.001)
        posts.append(synth.posteriors_from_bases(seq, rng, margin=3.5 if i % 2 else 6.0))
    rc = [False] * len(posts)
    with pkg.Decoder(m, r, msg_len, list_size=L, max_deviation=20) as dec:
        lists = [[] if isinstance(res, int) else ["".join(map(str, row)) for row in res[0]] for res in dec.decode(posts, rc=rc)]
        got = dec.decode_payloads(posts, rc, bpo, num_oligos)
    want = _host_filter(lists, bpo, num_oligos, False)
    assert (want[0] >= 0).sum() >= 10
    _assert_filter((got["index"], got["rank"], got["payload"]), want)
    assert got["counts"].tolist() == [len(lst) for lst in lists]


def test_tally_and_outer_decode_device_equal_host():
    rng = np.random.default_rng(17)
    bpo, n_data, n_rs = 6, 20, 10
    data = [bytes(rng.integers(0, 256, size=bpo, dtype=np.uint8)) for _ in range(n_data)]
    enc = rs_code.MainEncoder(data, n_rs)
    conv_in = [helper.attach_index_crc(i, p) for i, p in enumerate(enc)]
    lists = []
    for i in range(90):
        k = int(rng.integers(len(conv_in)))
        lst = [_junk(rng, bpo, False) for _ in range(int(rng.integers(1, 9)))]
        if i % 4:
            lst[int(rng.integers(len(lst)))] = conv_in[k]
        elif i % 8 == 0:                                          # passes the filter with a wrong payload
            lst[-1] = helper.attach_index_crc(k, bytes(bpo))
        lists.append(lst)
    lists.append([])
    for list_size in (8, 2):
        host = helper.tally_decoded_lists(lists, conv_in, bpo, False, list_size)
        assert helper.tally_decoded_lists(lists, conv_in, bpo, False, list_size, device=0) == host
        assert min(host.values()) > 0
        h = rs_code.decode_from_lists(lists, bpo, n_rs, n_data + n_rs, list_size=list_size)
        assert rs_code.decode_from_lists(lists, bpo, n_rs, n_data + n_rs, list_size=list_size, list_ops="device") == h
    assert h[1] > 0
    assert rs_code.decode_from_lists(lists, bpo, n_rs, n_data + n_rs)[0] == b"".join(data)
