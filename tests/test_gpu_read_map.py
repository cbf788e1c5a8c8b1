"""Read mapping on the GPU (csrc/mp_kernels.hip through lva_map_reads, read_map.map_reads) against its definition
(read_map.reference_map): every comparison is bit-equality of out.  Shapes sit at what the kernels distinguish: the 64-row
words of the distance and its register and LDS forms, windows around a 64-column tile, the vote ranges, ties."""
import io

import numpy as np
import pytest

import nanopore_dna_storage_amd as pkg
from nanopore_dna_storage_amd import error_profile as ep, helper, list_ops, read_map as rm, simulate as S
from nanopore_dna_storage_amd.decoder import encode

pytestmark = pytest.mark.gpu

SB, EB = "CACCTGTGCTGCGTCAGGCTGTGTC", "GCTGTCCGTTCCGCATTGACACGGC"
R = rm.VOTE_RANGE


def channel(rng, ref, sub=0.05, dele=0.05, ins=0.05):
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


def flip(read):
    return (3 - read)[::-1].astype(np.uint8)


def pack(reads):
    off = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.int64)
    return np.concatenate(list(reads) + [np.zeros(0, np.uint8)]).astype(np.uint8), np.stack([off[:-1], np.diff(off)], axis=1)


def same(got, want):
    assert got.out.dtype == want.out.dtype == np.int32 and got.out.shape == want.out.shape
    bad = np.nonzero((got.out != want.out).any(axis=1))[0]
    assert not len(bad), "%d rows differ, the first: read %d got %s want %s" % (len(bad), bad[0], got.out[bad[0]], want.out[bad[0]])


def check(bases, win, refs, k=10, max_occ=64, **kw):
    """the device against the definition, for these parameters and chunk_reads -> the definition's result"""
    chunk = kw.pop("chunk_reads", 0)
    want = rm.reference_map(bases, win, refs, k=k, max_occ=max_occ, **kw)
    with rm.MapIndex(refs, k, max_occ) as index:
        same(rm.map_reads(bases, win, index, chunk_reads=chunk, **kw), want)
    return want


@pytest.mark.parametrize("ref_len", [8, 9, 63, 64, 65, 127, 128, 129, 256, 257, 1024])
def test_word_boundaries_of_the_distance(ref_len):
    """k = 8: ref_len k and k + 1, the last word full and nearly empty, both register forms and the LDS form"""
    k = 8
    rng = np.random.default_rng(2000 + ref_len)
    refs = rng.integers(0, 4, (4, ref_len)).astype(np.uint8)
    reads = []
    for n in sorted({0, k - 1, k, 63, 64, 65, max(ref_len - 3, 0), ref_len + 40}):
        for o in range(4):
            read = fit(rng, np.concatenate([rng.integers(0, 4, o).astype(np.uint8), channel(rng, refs[o], 0.03, 0.03, 0.03)]), n)
            reads.append(flip(read) if (o + n) % 2 else read)
    bases, win = pack(reads)
    want = check(bases, win, refs, k=k, min_votes=1, cands=4)
    assert ref_len < 63 or want.mapped >= 8


def test_the_longest_windows_at_the_longest_oligo():
    rng = np.random.default_rng(31)
    refs = rng.integers(0, 4, (3, 1024)).astype(np.uint8)
    reads = []
    for o in range(3):
        read = np.concatenate([rng.integers(0, 4, 700 * o + 5).astype(np.uint8), channel(rng, refs[o], 0.03, 0.03, 0.03)])
        reads.append(fit(rng, flip(read) if o == 1 else read, 4096))
    bases, win = pack(reads)
    want = check(bases, win, refs)
    assert want.ref.tolist() == [0, 1, 2] and want.rc.tolist() == [0, 1, 0] and (want.count > 900).all()


def test_ties():
    """homopolymer and two-letter oligos, duplicates, a palindrome: the order of the candidates decides, strand 0 first"""
    rng = np.random.default_rng(37)
    m = 70
    pal = rng.integers(0, 4, m // 2).astype(np.uint8)
    pal = np.concatenate([pal, flip(pal)])
    uniq = rng.integers(0, 4, m).astype(np.uint8)
    refs = np.stack([np.zeros(m, np.uint8), np.full(m, 3, np.uint8), np.resize([0, 1], m), np.resize([2, 2, 3], m), np.resize([0, 0, 1, 1], m),
                     uniq, pal, uniq, pal]).astype(np.uint8)
    reads = []
    for o in range(len(refs)):
        for n in (m - 7, m, m + 9):
            reads += [fit(rng, channel(rng, refs[o]), n), np.resize(refs[o], n).astype(np.uint8), flip(np.resize(refs[o], n).astype(np.uint8))]
    bases, win = pack(reads)
    for k in (6, 10):
        want = check(bases, win, refs, k=k, cands=8, min_votes=1)
    exact = want.out[[3 * 3 * 6 + 3 + 1, 3 * 3 * 6 + 3 + 2]]                       # the palindrome as it is, and flipped: itself
    assert exact[:, :4].tolist() == [[6, 6, 0, 0], [6, 6, 0, 0]] and (exact[:, 7] == 0).all()
    dup = want.out[3 * 3 * 5 + 3 + 1]                                              # the duplicated oligo: the lower id, second == dist
    assert dup[:4].tolist() == [5, 5, 0, 0] and dup[7] == 0


@pytest.fixture(scope="module")
def noisy():
    """240 reads over 9 oligos of 115 bases, a third of them reverse strands, flanks, some junk, windows that overlap"""
    rng = np.random.default_rng(41)
    refs = rng.integers(0, 4, (9, 115)).astype(np.uint8)
    reads = []
    for i in range(240):
        if i % 17 == 0:
            reads.append(rng.integers(0, 4, int(rng.integers(0, 200))).astype(np.uint8))
            continue
        r = np.concatenate([rng.integers(0, 4, int(rng.integers(0, 30))), channel(rng, refs[rng.integers(0, 9)], 0.04, 0.04, 0.03),
                            rng.integers(0, 4, int(rng.integers(0, 30)))]).astype(np.uint8)
        reads.append(flip(r) if i % 3 == 0 else r)
    bases, win = pack(reads)
    letters = np.frombuffer(b"ACGT", np.uint8)[bases].copy()
    letters[rng.integers(0, len(letters), 60)] = ord("N")
    for i in range(5, 235, 10):
        win[i] = (win[i, 0] - 20, win[i, 1] + 35)
    return letters, win, refs, rm.reference_map(letters, win, refs)


@pytest.mark.parametrize("kw", [dict(cands=1), dict(cands=8), dict(cands=3, min_votes=1), dict(min_votes=5000), dict(max_dist=0),
                                dict(cands=2, max_dist=1000)], ids=str)
def test_parameters(noisy, kw):
    bases, win, refs, _ = noisy
    want = check(bases[:6000], win[win.sum(axis=1) <= 6000][:40], refs, **kw)
    assert want.mapped == 0 if kw.get("min_votes") == 5000 else want.mapped >= 0


@pytest.mark.parametrize("chunk_reads", [0, 1, 7])
def test_the_result_does_not_depend_on_the_chunk(noisy, chunk_reads):
    bases, win, refs, want = noisy
    with rm.MapIndex(refs) as index:
        same(rm.map_reads(bases, win, index, chunk_reads=chunk_reads), want)
    assert want.mapped >= 200


def test_the_same_call_twice_and_the_identity_with_align_profile(noisy):
    bases, win, refs, want = noisy
    with rm.MapIndex(refs) as index:
        a, b = rm.map_reads(bases, win, index), rm.map_reads(bases, win, index)
    assert a.out.tobytes() == b.out.tobytes() == want.out.tobytes()
    prof = ep.align_profile(bases, a.windows(win), refs, a.ref, a.rc)
    ok = a.ref >= 0
    assert ok.sum() >= 200 and np.array_equal(prof.read[ok, 0], a.dist[ok]) and (prof.read[~ok] == -1).all()
    assert a.coverage(9).sum() == ok.sum()


def test_an_empty_call_and_empty_windows():
    refs = np.random.default_rng(3).integers(0, 4, (2, 30)).astype(np.uint8)
    with rm.MapIndex(refs) as index:
        assert rm.map_reads(np.zeros(4, np.uint8), np.zeros((0, 2), np.int64), index).out.shape == (0, 8)
        got = rm.map_reads(np.zeros(0, np.uint8), [[0, 0], [0, 0], [0, 0]], index)
    assert got.out.tolist() == [list(rm.UNMAPPED)] * 3


@pytest.mark.parametrize("n_refs", [R - 1, R, R + 1, 2 * R + 3])
def test_vote_ranges(n_refs):
    """ref_len 12, k 6: every oligo is distinct from the others, reads are drawn from the first, the last and a middle
    range and across a range boundary; duplicated oligos on both sides of a boundary tie and the lower id wins"""
    rng = np.random.default_rng(n_refs)
    ids = rng.permutation(4 ** 8)[:n_refs]
    refs = np.concatenate([(ids[:, None] >> (2 * np.arange(8))) & 3, rng.integers(0, 4, (n_refs, 4))], axis=1).astype(np.uint8)
    if n_refs > R:
        refs[n_refs - 1] = refs[0]                                                 # a tie between the first and the last range
        refs[R] = refs[R - 1]                                                      # a tie across the boundary
    pick = sorted(o for o in {0, 1, R // 2, R - 2, R - 1, R, R + 1, n_refs - 2, n_refs - 1, n_refs // 2} if o < n_refs)
    reads = []
    for o in pick:
        reads += [refs[o], flip(refs[o]), fit(rng, np.concatenate([[1, 2], refs[o]]).astype(np.uint8), 20)]
    bases, win = pack(reads)
    want = check(bases, win, refs, k=6, max_occ=64, min_votes=1, cands=8, max_dist=3)
    assert want.mapped == len(reads)
    if n_refs > R:
        row = want.out[3 * pick.index(R - 1)]
        assert row[:4].tolist() == [R - 1, R - 1, 0, 0] and row[7] == 0            # its duplicate R is the runner-up


# ---------------------------------------------------------------- with the simulator

CODE = (6, 1, 60)
SET = dict(sub=0.02, dele=0.02, ins=0.01)


def test_simulated_reads_are_mapped_to_their_source():
    """the truth's bases as whole reads: equality with the definition, and the recovery of tests/test_read_map_host.py"""
    pool = np.random.default_rng(7).integers(0, 2, size=(12, CODE[2]), dtype=np.uint8)
    oligos = encode(*CODE, pool)
    with pkg.Decoder(*CODE, list_size=1, max_deviation=20) as dec:
        with dec.simulate(200, 2026, pool=pool, rc_mode=3, **SET) as (_, _, truth):
            bases, off, source, rc = truth["bases"].copy(), truth["base_offsets"].copy(), truth["source"].copy(), truth["rc"].copy()
    win = np.stack([off[:-1], np.diff(off)], axis=1)
    with rm.MapIndex(oligos) as index:
        got = rm.map_reads(bases, win, index)
    same(got, rm.reference_map(bases, win, oligos))
    assert np.array_equal(got.ref, source) and np.array_equal(got.rc, rc.astype(np.int32))


@pytest.fixture(scope="module")
def barcoded(tmp_path_factory):
    """40 barcoded reads of 9 indexed oligos at a rate that makes some lists fail the CRC, resident as posteriors for the
    length of the module's tests; the first 20 also as .post files with a manifest and the oligo file"""
    bpo = 4
    rng = np.random.default_rng(23)
    strings = [helper.attach_index_crc(i, bytes(rng.integers(0, 256, bpo, dtype=np.uint8))) for i in range(9)]
    pool = np.array([list_ops.bits_of(s) for s in strings], np.uint8)
    code = (6, 1, pool.shape[1])
    oligos = encode(*code, pool)
    d = tmp_path_factory.mktemp("barcoded")
    with pkg.Decoder(*code, list_size=4, max_deviation=20) as dec, rm.MapIndex(oligos) as index:
        with dec.simulate(40, 5, pool=pool, rc_mode=3, start_barcode=SB, end_barcode=EB, flank=(4, 12), sub=0.04, dele=0.04, ins=0.02) as (dev, off, truth):
            dec.posteriors_resident(dev, off)
            posts = dec.download(dev, off)
            (d / "oligos").write_text("".join("".join("ACGT"[b] for b in o) + "\n" for o in oligos))
            lines = []
            for i, p in enumerate(posts[:20]):
                p.astype(np.float32).tofile(str(d / ("r%d.post" % i)))
                lines.append("read%d\tx\t%s\n" % (i, d / ("r%d.post" % i)))
            (d / "manifest").write_text("".join(lines))
            yield dict(dec=dec, index=index, dev=dev, off=off, truth=truth, posts=posts, oligos=oligos, code=code, bpo=bpo, dir=d,
                       files=["--oligos", str(d / "oligos"), "--post_manifest", str(d / "manifest")])


def filtered_profile(b, dev, off):
    """locate, decode, filter, profile_decoded over a resident buffer -> (profile, reads that named an oligo)"""
    dec = b["dec"]
    chain = dec.decode_located(dev, off, dec.locate_payload_resident(dev, off, SB, EB))
    msgs, counts = list_ops.results_to_array([-100 if r is None else r for _, r in chain], 4, b["code"][2])
    fidx, _, _ = list_ops.filter_lists(msgs, counts, b["bpo"], len(b["oligos"]))
    return ep.profile_decoded(dec, dev, off, chain, fidx, b["oligos"]), np.array([bool(lc["ok"]) for lc, _ in chain]) & (fidx >= 0)


def test_profile_mapped_counts_the_reads_the_filter_rejects(barcoded):
    """profile_mapped against the definition applied to the oracle's basecalls of the downloaded posteriors, whole reads; it
    counts reads that the filtered profile leaves out"""
    from oracle import oracle as O
    b = barcoded
    oligos = b["oligos"]
    filtered, ok = filtered_profile(b, b["dev"], b["off"])
    mapped, res = ep.profile_mapped(b["dec"], b["dev"], b["off"], b["index"])
    calls = [O.basecall(p)[0] for p in b["posts"]]
    win = rm.whole_windows(calls)
    want = rm.reference_map("".join(calls), win, oligos)
    same(res, want)
    wp = ep.reference_profile("".join(calls), want.windows(win), oligos, want.ref, want.rc)
    for f in ("read", "pos", "conf", "ins"):
        assert np.array_equal(getattr(mapped, f), getattr(wp, f)), f
    rejected = ~ok & (res.ref >= 0)
    assert rejected.sum() >= 1 and (mapped.read[rejected, 0] >= 0).all() and (filtered.read[rejected, 0] == -1).all()
    assert mapped.reads > filtered.reads and np.array_equal(res.ref[res.ref >= 0], b["truth"]["source"][res.ref >= 0])


def test_the_read_map_command_line(barcoded):
    """20 reads: both files parse and agree with map_reads"""
    from oracle import oracle as O
    b = barcoded
    prefix = str(b["dir"] / "m")
    text = io.StringIO()
    cli = rm.main(b["files"] + ["--out_prefix", prefix, "--chunk", "7"], out=text, decoder=b["dec"])
    calls = [O.basecall(p)[0] for p in b["posts"][:20]]
    want = rm.map_reads("".join(calls), rm.whole_windows(calls), b["index"])
    assert np.array_equal(cli.out, want.out) and text.getvalue().split() == ["reads:", "20", "mapped:", str(cli.mapped)] and cli.mapped >= 15
    rows = [ln.split("\t") for ln in open(prefix + ".map.tsv").read().splitlines()]
    assert rows[0] == ["readid"] + list(rm.FIELDS) and [r[0] for r in rows[1:]] == ["read%d" % i for i in range(20)]
    assert np.array_equal(np.array([[int(v) for v in r[1:]] for r in rows[1:]]), cli.out)
    cov = np.loadtxt(prefix + ".coverage.tsv", dtype=np.int64, skiprows=1)
    assert np.array_equal(cov[:, 0], np.arange(len(b["oligos"]))) and np.array_equal(cov[:, 1:], cli.coverage(len(b["oligos"])))


@pytest.mark.parametrize("assign", ["filter", "map"])
def test_the_error_profile_command_line_in_chunks(barcoded, assign):
    """error_profile.main over the 20 reads in chunks of 7, with its default (--assign filter) and with --assign map: the
    profile of one pass over all 20, the CSV, and the summary line (reads / aligned, or reads / mapped / aligned)"""
    b = barcoded
    dec = b["dec"]
    prefix = str(b["dir"] / assign)
    argv = b["files"] + ["--start_barcode", SB, "--end_barcode", EB, "--mem_conv", "6", "--rate_conv", "1", "--msg_len", str(b["code"][2]),
                         "--list_size", "4", "--out_prefix", prefix, "--chunk", "7"] + ([] if assign == "filter" else ["--assign", "map"])
    text = io.StringIO()
    got = ep.main(argv, out=text, decoder=dec)
    with dec.resident(b["posts"][:20]) as (dev, off):
        if assign == "filter":
            want, ok = filtered_profile(b, dev, off)
            line = ["reads:", "20", "aligned:", str(int(ok.sum()))]
        else:
            want, res = ep.profile_mapped(dec, dev, off, b["index"])
            line = ["reads:", "20", "mapped:", str(res.mapped), "aligned:", str(res.mapped)]
    assert got == want and got.reads == int(line[-1]) >= 10
    assert text.getvalue().splitlines()[0].split() == line and text.getvalue().splitlines()[1].startswith("sub ")
    assert open(prefix + ".error_stats.csv").read().startswith("subs_pos,subs_rate\n0,")


def test_an_empty_index_maps_nothing_and_is_no_error():
    """ref_len < k: no pair, every list empty; the device agrees with the definition that nothing maps"""
    rng = np.random.default_rng(43)
    refs = rng.integers(0, 4, (3, 9)).astype(np.uint8)
    bases, win = pack([refs[0], rng.integers(0, 4, 40).astype(np.uint8), flip(refs[2])])
    want = check(bases, win, refs, k=10)
    assert want.out.tolist() == [list(rm.UNMAPPED)] * 3
