"""The error profile on the GPU (csrc/ep_kernels.hip through lva_align_profile, error_profile.align_profile) against its
definition (error_profile.reference_profile): every comparison is bit-equality of all four arrays.  Shapes sit at what the
kernels distinguish: stripes of 64 reference rows, an empty window, windows shorter and longer than the reference, the
limits of both lengths.  A reference is computed once per set of reads and shared."""
import numpy as np
import pytest

import nanopore_dna_storage_amd as pkg
from nanopore_dna_storage_amd import _lib, error_profile as ep, helper, list_ops, simulate as S
from nanopore_dna_storage_amd.decoder import encode

pytestmark = pytest.mark.gpu

SB, EB = "CACCTGTGCTGCGTCAGGCTGTGTC", "GCTGTCCGTTCCGCATTGACACGGC"
FIELDS = ("read", "pos", "conf", "ins")


def channel(rng, ref, sub=0.1, dele=0.1, ins=0.1):
    read = []
    for b in ref:
        while rng.random() < ins:
            read.append(rng.integers(0, 4))
        if rng.random() < dele:
            continue
        read.append((b + rng.integers(1, 4)) % 4 if rng.random() < sub else b)
    return np.array(read, np.uint8)


def fit(rng, read, n):
    """the read cut, or continued with random bases, to n bases"""
    return np.concatenate([read, rng.integers(0, 4, max(n - len(read), 0)).astype(np.uint8)])[:n]


def pack(reads):
    off = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.int64)
    return np.concatenate(list(reads) + [np.zeros(0, np.uint8)]).astype(np.uint8), np.stack([off[:-1], np.diff(off)], axis=1)


def same(got, want):
    for k in FIELDS:
        a, b = getattr(got, k), getattr(want, k)
        assert a.dtype == b.dtype and a.shape == b.shape, k
        assert np.array_equal(a, b), "%s: %d entries differ" % (k, int((a != b).sum()))


def check(bases, win, refs, ref_id, rc=None, **kw):
    want = ep.reference_profile(bases, win, refs, ref_id, rc)
    same(ep.align_profile(bases, win, refs, ref_id, rc, **kw), want)
    return want


@pytest.mark.parametrize("ref_len", [1, 2, 63, 64, 65, 127, 128, 129, 200])
def test_stripe_and_word_boundaries(ref_len):
    rng = np.random.default_rng(1000 + ref_len)
    refs = rng.integers(0, 4, (3, ref_len)).astype(np.uint8)
    reads, ref_id = [], []
    for n in sorted({0, 1, 63, 64, 65, max(ref_len - 3, 0), ref_len + 3}):
        for k in range(3):
            reads.append(fit(rng, channel(rng, refs[k]), n))
            ref_id.append(k)
    bases, win = pack(reads)
    want = check(bases, win, refs, ref_id)
    assert want.reads == len(reads) and want.aligned() == len(reads) * ref_len


def test_homopolymer_and_two_letter_references():
    """full of ties: the move order decides where every edit goes"""
    rng = np.random.default_rng(7)
    m = 130
    refs = np.stack([np.zeros(m, np.uint8), np.full(m, 3, np.uint8), np.resize([0, 1], m), np.resize([2, 2, 3], m), np.resize([0, 0, 1, 1], m)])
    refs = refs.astype(np.uint8)
    reads, ref_id = [], []
    for k in range(len(refs)):
        for n in (m - 7, m, m + 9):
            reads += [fit(rng, channel(rng, refs[k]), n), np.resize(refs[k], n).astype(np.uint8), np.resize(refs[k][::-1], n).astype(np.uint8)]
            ref_id += [k, k, k]
    bases, win = pack(reads)
    check(bases, win, refs, ref_id)
    check(bases, win, refs, ref_id, rc=np.arange(len(reads)) % 2)


def test_characters_codes_and_n():
    rng = np.random.default_rng(11)
    refs = rng.integers(0, 4, (2, 90)).astype(np.uint8)
    reads = [channel(rng, refs[k % 2], 0.05, 0.05, 0.05) for k in range(12)]
    bases, win = pack(reads)
    letters = np.frombuffer(b"ACGT", np.uint8)[bases].copy()
    letters[rng.integers(0, len(letters), 40)] = ord("N")
    letters[rng.integers(0, len(letters), 10)] = 200
    ref_letters = np.frombuffer(b"ACGT", np.uint8)[refs].copy()
    ref_letters[0, [0, 44, 89]] = ord("N")
    ref_id = np.arange(12) % 2
    want = check(letters, win, ref_letters, ref_id, rc=np.arange(12) % 3 == 0)
    assert want.ins[4] + want.conf[:, 4].sum() > 0 and want.conf.sum() < want.pos[:, :3].sum()
    same(ep.align_profile(bases, win, refs, ref_id), ep.align_profile(np.frombuffer(b"ACGT", np.uint8)[bases], win, refs, ref_id))


def test_limit_shapes():
    rng = np.random.default_rng(13)
    ref = rng.integers(0, 4, (1, 1024)).astype(np.uint8)
    read = fit(rng, channel(rng, ref[0], 0.05, 0.05, 0.05), 1100)
    check(read, [[0, 1100]], ref, [0])
    ref = rng.integers(0, 4, (1, 16)).astype(np.uint8)
    read = rng.integers(0, 4, 4096).astype(np.uint8)
    read[2000:2016] = ref[0]
    check(read, [[0, 4096]], ref, [0], rc=[1])


# ---------------------------------------------------------------- bookkeeping

@pytest.fixture(scope="module")
def many():
    """300 reads over 7 references, a third of them rc, some skipped, windows that overlap in the buffer"""
    rng = np.random.default_rng(17)
    refs = rng.integers(0, 4, (7, 70)).astype(np.uint8)
    ref_id = rng.integers(0, 7, 300).astype(np.int32)
    rc = (np.arange(300) % 3 == 0).astype(np.uint8)
    reads = []
    for i in range(300):
        r = channel(rng, refs[ref_id[i]], 0.03, 0.03, 0.03)
        reads.append((3 - r)[::-1].astype(np.uint8) if rc[i] else r)
    bases, win = pack(reads)
    for i in range(5, 295, 10):                      # a window that runs into its neighbours'
        win[i] = (win[i, 0] - 20, win[i, 1] + 35)
    win[7] = win[8]
    ref_id[::11] = -1
    want = ep.reference_profile(bases, win, refs, ref_id, rc)
    assert want.reads == 300 - len(range(0, 300, 11)) and (want.read[::11] == -1).all()
    return bases, win, refs, ref_id, rc, want


@pytest.mark.parametrize("chunk_reads", [0, 1, 7])
def test_the_result_does_not_depend_on_the_chunk(many, chunk_reads):
    bases, win, refs, ref_id, rc, want = many
    same(ep.align_profile(bases, win, refs, ref_id, rc, chunk_reads=chunk_reads), want)


def test_the_same_call_twice_gives_the_same_bytes(many):
    bases, win, refs, ref_id, rc, want = many
    a, b = ep.align_profile(bases, win, refs, ref_id, rc), ep.align_profile(bases, win, refs, ref_id, rc)
    for k in FIELDS:
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes() == getattr(want, k).tobytes(), k


@pytest.mark.parametrize("absent", FIELDS + ("rc",))
def test_each_output_may_be_null(many, absent):
    bases, win, refs, ref_id, rc, want = many
    if absent == "rc":
        want = ep.reference_profile(bases, win, refs, ref_id)
    first, count = np.ascontiguousarray(win[:, 0]), np.ascontiguousarray(win[:, 1], dtype=np.int32)
    out = dict(read=np.full((300, 4), 77, np.int32), pos=np.full((71, 4), 77, np.int64), conf=np.full((4, 6), 77, np.int64),
               ins=np.full(5, 77, np.int64))
    ptr = [None if k == absent else out[k].ctypes.data for k in FIELDS]
    st = _lib.load_library().lva_align_profile(0, bases.ctypes.data, first.ctypes.data, count.ctypes.data, 300, refs.ctypes.data, 7, 70,
                                               ref_id.ctypes.data, None if absent == "rc" else rc.ctypes.data, 0, *ptr)
    assert st == 0
    for k in FIELDS:
        assert (out[k] == 77).all() if k == absent else np.array_equal(out[k], getattr(want, k)), k


def test_no_read_and_only_skipped_reads():
    refs = np.zeros((1, 5), np.uint8)
    p = ep.align_profile(np.zeros(4, np.uint8), np.zeros((0, 2), np.int64), refs, np.zeros(0, np.int32))
    assert p.reads == 0 and not p.pos.any()
    same(ep.align_profile(np.zeros(4, np.uint8), [[0, 4], [1, 2]], refs, [-1, -1]),
         ep.reference_profile(np.zeros(4, np.uint8), [[0, 4], [1, 2]], refs, [-1, -1]))


# ---------------------------------------------------------------- with the simulator

CODE = (6, 1, 60)
SET = dict(sub=0.02, dele=0.02, ins=0.01)


def test_the_simulators_channel_has_the_rates_it_was_given():
    """200 reads of a pool of 12 messages, a coin per read for the orientation; the truth's bases are what the channel emitted,
    so a reverse-complemented strand is passed with its rc flag.  Alignment re-attributes a few edits; for this seed the
    definition alone (simulate.reference_reads + reference_profile, no GPU) gives, over N = 13 200 reference bases,
    sub 0.021288 (z = 1.06), dele 0.019015 (z = -0.81), ins 0.009394 (z = -0.70): inside five standard deviations."""
    pool = np.random.default_rng(7).integers(0, 2, size=(12, CODE[2]), dtype=np.uint8)
    oligos = encode(*CODE, pool)
    ref = S.reference_reads(*CODE, 200, 2026, scores=False, pool=pool, rc_mode=3, **SET)
    with pkg.Decoder(*CODE, list_size=1, max_deviation=20) as dec:
        with dec.simulate(200, 2026, pool=pool, rc_mode=3, **SET) as (_, _, truth):
            bases, off, source, rc = truth["bases"].copy(), truth["base_offsets"].copy(), truth["source"].copy(), truth["rc"].copy()
    assert np.array_equal(bases, ref["bases"]) and np.array_equal(source, ref["source"]) and rc.any() and not rc.all()
    win = np.stack([off[:-1], np.diff(off)], axis=1)
    want = ep.reference_profile(ref["bases"], win, oligos, ref["source"], ref["rc"])
    got = ep.align_profile(bases, win, oligos, source, rc)
    same(got, want)
    n = got.aligned()
    assert n == 200 * oligos.shape[1]
    for where in (want, got):
        rates = where.rates()
        for k, p in SET.items():
            sd = (p * (1 - p) / n) ** 0.5
            print(k, rates[k], "set", p, "z = %.2f" % ((rates[k] - p) / sd))
            assert abs(rates[k] - p) <= 5 * sd, (k, rates[k])


def test_profile_decoded_equals_the_definition_on_host_side_basecalls():
    """40 barcoded reads of a file's oligos: locate, decode, filter on the device, then profile_decoded against the
    definition applied to the oracle's basecalls of the downloaded posteriors and the windows cut from them"""
    from oracle import oracle as O
    bpo = 4
    rng = np.random.default_rng(23)
    strings = [helper.attach_index_crc(i, bytes(rng.integers(0, 256, bpo, dtype=np.uint8))) for i in range(9)]
    pool = np.array([list_ops.bits_of(s) for s in strings], np.uint8)
    code = (6, 1, pool.shape[1])
    oligos = encode(*code, pool)
    with pkg.Decoder(*code, list_size=4, max_deviation=20) as dec:
        with dec.simulate(40, 5, pool=pool, rc_mode=3, start_barcode=SB, end_barcode=EB, flank=(4, 12), sub=0.01, dele=0.01, ins=0.005) as (dev, off, truth):
            dec.posteriors_resident(dev, off)
            chain = dec.decode_located(dev, off, dec.locate_payload_resident(dev, off, SB, EB))
            msgs, counts = list_ops.results_to_array([-100 if r is None else r for _, r in chain], 4, code[2])
            index, _, _ = list_ops.filter_lists(msgs, counts, bpo, len(pool))
            got = ep.profile_decoded(dec, dev, off, chain, index, oligos)
            posts = dec.download(dev, off)
    calls = [O.basecall(p)[:2] for p in posts]
    locs = [lc for lc, _ in chain]
    win = ep.payload_windows([t for _, t in calls], locs)
    base_off = np.concatenate([[0], np.cumsum([len(b) for b, _ in calls])])
    win[:, 0] += base_off[:-1]
    ok = np.array([lc["ok"] for lc in locs])
    ref_id = np.where(ok, index, -1)
    want = ep.reference_profile("".join(b for b, _ in calls), win, oligos, ref_id, rc=[lc["rc"] and lc["ok"] for lc in locs])
    same(got, want)
    assert want.reads >= 30 and (ref_id[ref_id >= 0] == truth["source"][ref_id >= 0]).all()
    assert np.array_equal(np.array([lc["rc"] for lc in locs])[ref_id >= 0], truth["rc"][ref_id >= 0].astype(bool))
    assert np.median(want.read[ref_id >= 0, 0]) <= 6                  # the windows are the payloads: a few channel errors each


def test_roundtrip_error_profile_whatever_the_chunk_and_as_the_definition(tmp_path):
    """roundtrip --error_profile: the reads as the channel emitted them against the truth's source and rc"""
    import io
    from nanopore_dna_storage_amd import roundtrip
    data = bytes(np.random.default_rng(29).integers(0, 256, 90, dtype=np.uint8))
    path = tmp_path / "data.bin"
    path.write_bytes(data)

    def run(chunk, prefix):
        argv = ["--data_file", str(path), "--bytes_per_oligo", "6", "--RS_redundancy", "0.2", "--mem_conv", "6", "--rate_conv", "1",
                "--list_size", "4", "--num_reads", "60", "--seed", "3", "--chunk", str(chunk), "--sub", "0.02", "--dele", "0.02", "--ins", "0.01",
                "--num_reads_to_use", "30", "--num_trials", "1", "--out", str(tmp_path / (prefix + ".txt")), "--error_profile", str(tmp_path / prefix)]
        res = roundtrip.main(argv, out=io.StringIO())
        return res["error_profile"], (tmp_path / (prefix + ".error_stats.csv")).read_text()

    a, csv_a = run(7, "a")
    b, csv_b = run(1000, "b")
    same(a, b)
    assert csv_a == csv_b and csv_a.startswith("subs_pos,subs_rate\n0,") and a.reads == 60
    oligo_file = str(tmp_path / "oligos")                # the pool is what helper.encode writes: made again from the same file
    helper.encode(str(path), oligo_file, 6, 0.2, 6, 1, out=io.StringIO())
    msgs = helper.read_conv_input(oligo_file + ".conv_input")
    code = (6, 1, msgs.shape[1])
    ref = S.reference_reads(*code, 60, 3, scores=False, pool=msgs, rc_mode=3, sub=0.02, dele=0.02, ins=0.01)
    off = ref["base_offsets"]
    same(a, ep.reference_profile(ref["bases"], np.stack([off[:-1], np.diff(off)], axis=1), encode(*code, msgs), ref["source"], ref["rc"]))
