"""A pooled run mapped on the GPU (csrc/mq_kernels.hip through lva_map_reads_pooled, read_map.map_reads) against its
definition (read_map.reference_map): every comparison is bit-equality of out and of supp, no tolerance anywhere.  Shapes sit
at what the kernels distinguish: oligos on both sides of a 64-row word in the lanes of one read, the two register forms and
the LDS form, windows around a 64-column tile, wavefronts partly empty, the flank length at min_flank."""
import io

import numpy as np
import pytest

import nanopore_dna_storage_amd as pkg
from nanopore_dna_storage_amd import error_profile as ep, read_map as rm
from nanopore_dna_storage_amd.decoder import encode
from nanopore_dna_storage_amd.error_profile import MAX_READ

import pooled_map_util as U
from test_gpu_read_map import channel, fit

pytestmark = pytest.mark.gpu


def same(got, want):
    for name, g, w in (("out", got.out, want.out),) + ((("supp", got.supp.out, want.supp.out),) if want.supp is not None else ()):
        assert g.dtype == w.dtype == np.int32 and g.shape == w.shape
        bad = np.nonzero((g != w).any(axis=1))[0]
        assert not len(bad), "%s: %d rows differ, the first: read %d got %s want %s" % (name, len(bad), bad[0], g[bad[0]], w[bad[0]])
    assert (got.supp is None) == (want.supp is None)


def check(bases, win, refs, k=10, max_occ=64, groups=None, chunk_reads=0, **kw):
    """the device against the definition -> the definition's result"""
    want = rm.reference_map(bases, win, refs, k=k, max_occ=max_occ, groups=groups, **kw)
    with rm.MapIndex(refs, k, max_occ, groups) as index:
        same(rm.map_reads(bases, win, index, chunk_reads=chunk_reads, **kw), want)
    return want


@pytest.mark.parametrize("longest", [128, 256, 1024])
def test_nested_prefixes_in_every_form(longest):
    """the prefixes of one 1024-mer up to 128, 256 and 1024 bases: the 2-word, the 4-word and the LDS form of mq_verify; the
    eight candidates of a read are oligos of 63, 64 and 65 (127, 128, 129; 255, 256, 257) bases side by side"""
    oligos, reads, front = U.nested(longest)
    reads = reads + [U.flip(r) for r in reads[::2]]
    bases, win = U.pack(reads)
    want = check(bases, win, oligos, **U.NESTED)
    n = len(oligos)
    assert want.ref[:n].tolist() == list(range(n)) and (want.dist[:n] == 0).all() and want.start[:n].tolist() == front
    assert (want.rc[n:] == 1).all() and want.ref[n:].tolist() == list(range(0, n, 2))
    check(bases, win, oligos, min_flank=8, **U.NESTED)


@pytest.fixture(scope="module")
def mixed():
    """oligos of 30 .. 200 bases in three groups, 40 noisy reads of them on both strands between junk, some junk alone"""
    rng = np.random.default_rng(51)
    lens = [30, 64, 65, 70, 128, 129, 140, 200, 33, 191]
    oligos = [rng.integers(0, 4, m).astype(np.uint8) for m in lens]
    groups = np.array([0, 0, 0, 1, 1, 1, 1, 2, 2, 2], np.int32)
    reads = []
    for i in range(40):
        if i % 13 == 5:
            reads.append(rng.integers(0, 4, int(rng.integers(0, 90))).astype(np.uint8))
            continue
        r = np.concatenate([rng.integers(0, 4, int(rng.integers(0, 40))), channel(rng, oligos[i % 10], 0.03, 0.03, 0.03),
                            rng.integers(0, 4, int(rng.integers(0, 40)))]).astype(np.uint8)
        reads.append(U.flip(r) if i % 3 == 0 else r)
    bases, win = U.pack(reads)
    return bases, win, oligos, groups


def test_window_length_extremes(mixed):
    _, _, oligos, groups = mixed
    rng = np.random.default_rng(52)
    k = 8
    reads = []
    for n in (0, k - 1, k, 63, 64, 65, MAX_READ):
        for o in (0, 2, 7):
            read = fit(rng, np.concatenate([rng.integers(0, 4, o).astype(np.uint8), channel(rng, oligos[o], 0.02, 0.02, 0.02)]), n)
            reads.append(U.flip(read) if (o + n) % 2 else read)
    reads[-1][500:500 + len(oligos[4])] = oligos[4]              # an exact oligo in the longest window: the primary; the noisy one is far down its right flank
    bases, win = U.pack(reads)
    want = check(bases, win, oligos, k=k, groups=groups, min_votes=1, min_flank=15)
    assert want.mapped >= 7 and want.out[-1, :6].tolist() == [4, 4, 0, 0, 500, 128] and want.supp.out[-1, :3].tolist() == [7, 7, 1]
    assert want.supp.start[-1] > 3800


@pytest.mark.parametrize("cands", [1, 3, 8])
def test_one_wavefront_of_mixed_work(mixed, cands):
    bases, win, oligos, groups = mixed
    want = check(bases, win, oligos, groups=groups, cands=cands, min_votes=1, min_flank=15)
    assert want.mapped >= 30 and 0 < (want.rc == 1).sum() < want.mapped and len(set(want.group.tolist())) == 4


@pytest.mark.parametrize("chunk_reads", [0, 1, 7])
def test_batch_edges(mixed, chunk_reads):
    bases, win, oligos, groups = mixed
    for n in (1, 15, 17, 33):
        check(bases, win[:n], oligos, groups=groups, chunk_reads=chunk_reads, min_flank=15)


@pytest.mark.parametrize("min_flank, chunk_reads", [(U.MIN_FLANK, 0), (U.MIN_FLANK, 1), (U.MIN_FLANK + 1, 3)])
def test_the_supplementary_pass_on_constructed_reads(mixed, min_flank, chunk_reads):
    """the chimeric reads of tests/test_read_map_pooled_host.py with the reads of `mixed` cut to 60 bases between them"""
    oligos, groups = U.chimeric_pool()
    made, want_rows, want_supp = U.chimeric_reads()
    other = [mixed[0][f:f + min(c, 60)] for f, c in mixed[1][:len(made)]]
    bases, win = U.pack([r for pair in zip(made, other) for r in pair])
    want = check(bases, win, oligos, groups=groups, chunk_reads=chunk_reads, min_flank=min_flank, **U.CHIM)
    U.expect(want.out[::2], want_rows)
    if min_flank > U.MIN_FLANK:
        want_supp = want_supp[:6] + [None] + want_supp[7:]
    U.expect(want.supp.out[::2], want_supp)


def test_equality_with_the_equal_length_path():
    """a rectangular index, max_dist constant, no supplementary pass: lva_map_reads_pooled returns the bytes of lva_map_reads"""
    rng = np.random.default_rng(41)
    refs = rng.integers(0, 4, (9, 115)).astype(np.uint8)
    reads = []
    for i in range(120):
        r = np.concatenate([rng.integers(0, 4, int(rng.integers(0, 30))), channel(rng, refs[rng.integers(0, 9)], 0.04, 0.04, 0.03),
                            rng.integers(0, 4, int(rng.integers(0, 30)))]).astype(np.uint8)
        reads.append(rng.integers(0, 4, 50).astype(np.uint8) if i % 17 == 0 else U.flip(r) if i % 3 == 0 else r)
    bases, win = U.pack(reads)
    with rm.MapIndex(refs) as index:
        for md in (28, 3):
            old = rm.map_reads(bases, win, index, max_dist=md)
            new = rm.map_reads(bases, win, index, max_dist=np.full(9, md))
            assert old.out.tobytes() == new.out.tobytes() and new.supp is None
            assert (old.ref >= 0).sum() >= (90 if md == 28 else 0) and (old.best >= 0).sum() >= 100


def test_other_parameters(mixed):
    bases, win, oligos, groups = mixed
    per_oligo = np.array([0, 3, 0, 50, 1, 0, 2, 9, 0, 4])
    want = check(bases, win, oligos, max_dist=per_oligo, min_flank=15)
    assert 0 < want.mapped < (want.best >= 0).sum()
    want = check(bases, win, oligos, max_dist=0, min_flank=15)
    assert want.mapped <= 2 and not want.chimeric.any()
    with rm.MapIndex(oligos, groups=groups) as index:
        got = rm.map_reads(np.zeros(4, np.uint8), np.zeros((0, 2), np.int64), index, min_flank=5)
        assert got.out.shape == got.supp.out.shape == (0, 8) and all(len(s) == 0 for s in got.split())
        got = rm.map_reads(np.zeros(0, np.uint8), [[0, 0], [0, 0]], index, min_flank=5)
        assert got.out.tolist() == got.supp.out.tolist() == [list(rm.UNMAPPED)] * 2
    short = [o[:m] for o, m in zip(oligos, (9, 3, 8, 1, 9, 7, 2, 9, 5, 6))]          # every oligo shorter than k = 10
    want = check(bases, win[:9], short, min_flank=5)
    assert want.out.tolist() == [list(rm.UNMAPPED)] * 9


# ---------------------------------------------------------------- with the simulator: error profile and command line

CODES = ((6, 1, 60), (6, 1, 72))


@pytest.fixture(scope="module")
def two_pools(tmp_path_factory):
    """12 reads of each of two pools whose oligo lengths differ, as posteriors; an oligo file per pool and a manifest"""
    d = tmp_path_factory.mktemp("pooled")
    rng = np.random.default_rng(29)
    posts, oligos, groups, files = [], [], [], []
    for g, code in enumerate(CODES):
        pool = rng.integers(0, 2, size=(5, code[2]), dtype=np.uint8)
        with pkg.Decoder(*code, list_size=1, max_deviation=20) as dec:
            with dec.simulate(12, 7 + g, pool=pool, rc_mode=3, **U.SET) as (dev, off, _):
                dec.posteriors_resident(dev, off)
                posts += dec.download(dev, off)
        mine = encode(*code, pool)
        oligos += list(mine)
        groups += [g] * len(mine)
        (d / ("exp%d.oligos" % g)).write_text("".join("".join("ACGT"[b] for b in o) + "\n" for o in mine))
        files.append(str(d / ("exp%d.oligos" % g)))
    lines = []
    for i, p in enumerate(posts):
        p.astype(np.float32).tofile(str(d / ("r%d.post" % i)))
        lines.append("read%d\tx\t%s\n" % (i, d / ("r%d.post" % i)))
    (d / "manifest").write_text("".join(lines))
    with pkg.Decoder(*CODES[0], list_size=1, max_deviation=20) as dec:
        yield dict(dec=dec, posts=posts, oligos=oligos, groups=np.array(groups, np.int32), files=files, dir=d)


def test_profile_mapped_per_group(two_pools):
    t = two_pools
    dec = t["dec"]
    with rm.MapIndex(t["oligos"], groups=t["groups"]) as index, dec.resident(t["posts"]) as (dev, off):
        profiles, res = ep.profile_mapped(dec, dev, off, index, min_flank=int(index.lens.min()) // 2)
        calls = [b for b, _ in dec.basecall_resident(dev, off)]
    bases, win = "".join(calls), rm.whole_windows(calls)
    same(res, rm.reference_map(bases, win, t["oligos"], groups=t["groups"], min_flank=int(index.lens.min()) // 2))
    assert len(profiles) == 2 and res.mapped >= 20
    for g, reads in enumerate(res.split()):
        members = np.nonzero(t["groups"] == g)[0]
        refs = np.stack([t["oligos"][o] for o in members])
        by_hand = ep.align_profile(bases, res.windows(win)[reads], refs, res.ref[reads] - members[0], res.rc[reads])
        got = profiles[g]
        assert got.reads == len(reads) >= 8 and np.array_equal(got.read[reads], by_hand.read) and (np.delete(got.read, reads, axis=0) == -1).all()
        for f in ("pos", "conf", "ins"):
            assert np.array_equal(getattr(got, f), getattr(by_hand, f)), (g, f)
    with rm.MapIndex(t["oligos"], groups=np.zeros(len(t["oligos"]), np.int32)) as index, dec.resident(t["posts"][:2]) as (dev, off):
        with pytest.raises(ValueError):
            ep.profile_mapped(dec, dev, off, index)                               # one group, two lengths


def test_the_command_line_with_two_oligo_files(two_pools):
    t = two_pools
    prefix = str(t["dir"] / "m")
    text = io.StringIO()
    res = rm.main(["--oligos"] + t["files"] + ["--post_manifest", str(t["dir"] / "manifest"), "--out_prefix", prefix, "--chunk", "7"],
                  out=text, decoder=t["dec"])
    n = len(t["posts"])
    rows = [ln.split("\t") for ln in open(prefix + ".map.tsv").read().splitlines()]
    assert len(rows) == n + 1 and len(rows[0]) == 1 + 8 + 2 + 8 and rows[0][9:11] == ["group", "chimeric"]
    assert np.array_equal(np.array([[int(v) for v in r[1:9]] for r in rows[1:]]), res.out)
    assert np.array_equal(np.array([[int(v) for v in r[11:]] for r in rows[1:]]), res.supp.out)
    cov = [ln.split("\t") for ln in open(prefix + ".coverage.tsv").read().splitlines()]
    assert cov[0] == ["group", "oligo", "forward", "reverse"] and len(cov) == len(t["oligos"]) + 1
    split = res.split()
    for g, reads in enumerate(split):
        assert open("%s.exp%d.readids.txt" % (prefix, g)).read().split() == ["read%d" % i for i in reads]
        assert [r[9] for r in rows[1:]].count("exp%d" % g) == int((res.group == g).sum())
    assert text.getvalue().split() == ["reads:", str(n), "mapped:", str(res.mapped), "chimeric:", str(int(res.chimeric.sum())),
                                       "exp0:", str(len(split[0])), "exp1:", str(len(split[1]))]
    assert res.mapped >= 20 and len(split[0]) >= 8 and len(split[1]) >= 8
    got = ep.main(["--oligos"] + t["files"] + ["--post_manifest", str(t["dir"] / "manifest"), "--out_prefix", prefix, "--assign", "map",
                   "--start_barcode", "A", "--end_barcode", "A", "--mem_conv", "6", "--rate_conv", "1", "--msg_len", "60", "--list_size", "1"],
                  out=io.StringIO(), decoder=t["dec"])
    assert [p.reads for p in got] == [len(s) for s in split]
    assert open(prefix + ".exp1.error_stats.csv").read().startswith("subs_pos,subs_rate\n0,")
