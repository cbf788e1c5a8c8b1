"""The forward score without a GPU: trellis_score.reference_forward, the definition of csrc/fw_kernels.hip, held to a float64
enumeration of the full flip-flop trellis (band off and banded), to reference_score on posteriors with a single path (bit for
bit) and from below on random reads; its refusals; the helpers of the list posterior; the table; and the check that the float32
restatement's error -- the yardstick of tests/test_gpu_trellis_forward.py -- is not 0 on any of that file's case classes."""
import warnings

import numpy as np
import pytest

from nanopore_dna_storage_amd import _lib, synth
from nanopore_dna_storage_amd import trellis_score as T
from trellis_forward_cases import NEG, OFF, SINGLE_PATH_SIZES, brute_force, err, klass, narrow, single_path


def _random_post(rng, nblk, holes):
    post = rng.normal(-2.0, 1.5, size=(nblk, 40)).astype(np.float32)
    post[rng.random((nblk, 40)) < holes] = NEG
    return post


def _close(a, b):
    if a == NEG or b == NEG:
        return a == b
    return abs(a - b) <= 1e-12 * max(1.0, abs(b))


@pytest.mark.parametrize("md", [None, 1])
@pytest.mark.parametrize("n, extra", [(1, 2), (1, 3), (2, 2), (2, 3), (3, 3)])
def test_float64_is_the_sum_over_every_path(n, extra, md):
    rng = np.random.default_rng(100 * n + extra)
    finite = 0
    for trial in range(6):
        seq = rng.integers(0, 4, n) if trial else np.zeros(n, np.int64)       # a homopolymer among them: flip -> flop steps
        post = _random_post(rng, n + extra, 0.15 if trial % 2 else 0.0)
        got = T.reference_forward(post, seq, OFF if md is None else md)
        want = brute_force(post, seq, md)
        assert got[0].dtype == np.float64
        assert _close(float(got[0]), want[0]) and _close(float(got[1]), want[1]), (seq, got, want)
        finite += np.isfinite(want).sum()
    assert finite > 0


def test_the_band_of_the_enumeration_bites():
    """max_deviation = 1 drops paths on a 3-base sequence over 6 blocks: the banded sum is below the unbanded one"""
    rng = np.random.default_rng(7)
    post, seq = _random_post(rng, 6, 0.0), [0, 1, 1]
    assert max(brute_force(post, seq, 1)) < max(brute_force(post, seq, None))
    assert max(T.reference_forward(post, seq, 1)) < max(T.reference_forward(post, seq, OFF))


@pytest.mark.parametrize("n, nblk", SINGLE_PATH_SIZES)
def test_single_path_is_the_score_bit_for_bit(n, nblk):
    c = single_path(n, nblk)
    live = c["end_state"]
    assert np.isfinite(c["score"][live]) and c["score"][1 - live] == NEG
    for dtype in (np.float32, np.float64):
        got = T.reference_forward(c["post"], c["seq"], OFF, dtype=dtype)
        assert got[1 - live] == NEG
    got = T.reference_forward(c["post"], c["seq"], OFF, dtype=np.float32)
    assert got[live].dtype == np.float32 and got[live].tobytes() == np.float32(c["score"][live]).tobytes()


def test_unbanded_forward_is_at_least_the_best_path():
    for seed in range(4):
        x = synth.make_read(6, 1, 40, 300 + seed, margin=3.0, sub=0.03, dele=0.03, ins=0.01)
        fw = T.reference_forward(x["post"], x["oligo"], OFF)
        sc = T.reference_score(x["post"], x["oligo"], OFF)
        for k in range(2):
            assert fw[k] >= np.float64(sc[k]) - 1e-4, (seed, k, fw, sc)
        assert np.isfinite(max(fw)) and max(fw) > max(sc)                   # more than one alignment carries weight


def test_all_minus_inf_and_the_refusals():
    post = np.full((10, 40), NEG, np.float32)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for dtype in (np.float64, np.float32):
            for md in (2, OFF):
                got = T.reference_forward(post, [0, 1, 1, 2], md, dtype=dtype)
                assert got[0] == NEG and got[1] == NEG
        part = np.zeros((10, 40), np.float32)
        part[4] = NEG                                                       # one dead block kills every path
        assert T.reference_forward(part, "ACG", OFF) == (NEG, NEG)
    ok = np.zeros((10, 40), np.float32)
    assert T.reference_forward(ok, "ACG", 5) == T.reference_forward(ok, [0, 1, 2], 5) == T.reference_forward(ok, b"ACG", 5)
    for bad in ([], [0, 4], "ACGN"):
        with pytest.raises(ValueError):
            T.reference_forward(ok, bad, 5)
    with pytest.raises(ValueError):
        T.reference_forward(ok[:4], [0, 1, 2], 5)                           # 4 blocks < 4 positions + 1
    for v in (np.nan, np.inf):
        p = ok.copy()
        p[3, 7] = v
        with pytest.raises(ValueError):
            T.reference_forward(p, [0, 1, 2], 5)
    with pytest.raises(ValueError):
        T.reference_forward(ok, [0, 1, 2], 5, dtype=np.float16)


def test_a_cell_outside_the_band_is_cleared():
    """a band of 2 positions on 40 bases: the forward score differs from what never-cleared buffers give, and reading the band
    of the block before is what makes it the sum over the paths inside the band (the enumeration above)"""
    post, seq = narrow()
    assert post.shape == (90, 40) and len(seq) == 40
    for md in (1, 2):
        fw, sc = T.reference_forward(post, seq, md), T.reference_score(post, seq, md)
        assert np.isfinite(max(fw)) and abs(max(fw) - np.float64(max(sc))) > 1e-2, (md, fw, sc)


def test_helpers_of_the_list_posterior():
    tot = np.array([-10.0, -9.0, NEG, -9.0, -12.5])
    p = T.list_posterior(tot)
    assert abs(p.sum() - 1.0) < 1e-12 and p[2] == 0.0 and p[1] == p[3] > p[0] > p[4] > 0
    assert abs(p[1] / p[0] - np.e) < 1e-12
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert np.isnan(T.list_posterior([NEG, NEG])).all() and len(T.list_posterior([NEG, NEG])) == 2
        assert T.list_posterior([-3.0]).tolist() == [1.0] and T.list_posterior([]).shape == (0,)
    assert T.forward_order(tot).tolist() == [1, 3, 0, 4, 2]
    assert T.forward_order([NEG, NEG, -1.0, -1.0]).tolist() == [2, 3, 0, 1] and T.forward_order([]).shape == (0,)
    ff = np.array([[-1.0, NEG], [NEG, NEG], [np.log(0.25), np.log(0.75)]])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        t = T.forward_total(ff)
    assert t.dtype == np.float64 and t[0] == -1.0 and t[1] == NEG and abs(t[2]) < 1e-15


def test_table_with_and_without_the_forward_columns(tmp_path):
    rows = [dict(rank=0, banded=np.float32(-5), unbanded=np.float32(-5), first=-5.0, last=-9.0, verdict="in_list"),
            dict(rank=-1, banded=None, unbanded=None, first=float("nan"), last=float("nan"), verdict="short_read")]
    path = str(tmp_path / "t.tsv")
    T.write_table(rows, path)
    old = ("read\trank\tbanded\tunbanded\tfirst\tlast\tverdict\n"
           "0\t0\t-5.0\t-5.0\t-5.0\t-9.0\tin_list\n"
           "1\t-1\tnan\tnan\tnan\tnan\tshort_read\n")
    assert open(path).read() == old
    assert T.summary_line(rows) == "truth score: 2 reads, in_list 1, list_too_short 0, band 0, short_read 1"
    rows[0].update(fwd_truth=-4.5, fwd_first=-4.5, fwd_best=0, conf_first=0.75)
    T.write_table(rows, path)                                               # not every row carries them: the old bytes
    assert open(path).read() == old
    rows[1].update(fwd_truth=float("nan"), fwd_first=float("nan"), fwd_best=-1, conf_first=float("nan"))
    T.write_table(rows, path)
    assert open(path).read() == ("read\trank\tbanded\tunbanded\tfirst\tlast\tverdict\tfwd_truth\tfwd_first\tfwd_best\tconf_first\n"
                                 "0\t0\t-5.0\t-5.0\t-5.0\t-9.0\tin_list\t-4.5\t-4.5\t0\t0.75\n"
                                 "1\t-1\tnan\tnan\tnan\tnan\tshort_read\tnan\tnan\t-1\tnan\n")
    rows.append(dict(rank=2, banded=np.float32(-6), unbanded=np.float32(-6), first=-5.0, last=-9.0, verdict="in_list",
                     fwd_truth=-4.0, fwd_first=-4.2, fwd_best=2, conf_first=0.4))
    rows.append(dict(rank=1, banded=np.float32(-6), unbanded=np.float32(-6), first=-5.0, last=-9.0, verdict="in_list",
                     fwd_truth=-4.4, fwd_first=-4.2, fwd_best=3, conf_first=0.4))
    assert T.forward_counts(rows) == (2, 1)
    assert T.summary_line(rows, forward=True).endswith("short_read 1, fwd_best != 0 2, truth first by forward only 1")


@pytest.mark.parametrize("name", ["S1", "S2", "S3"])
def test_the_yardstick_of_the_gpu_classes_is_not_zero(name):
    c = klass(name)
    print(name, "E_f32 = %.3g over %d pairs, |value| up to %.4g" % (c["e_f32"], len(c["pairs"]), np.abs(c["f64"][np.isfinite(c["f64"])]).max()))
    assert np.isfinite(c["f64"]).any(axis=1).all()                          # every pair has a path
    assert 0 < c["e_f32"] < np.inf
    assert err(c["f64"], c["f64"]) == 0.0 and err([NEG, 1.0], [NEG, NEG]) == np.inf and err([np.nan], [1.0]) == np.inf


@pytest.mark.parametrize("name", ["lva_forward_bases", "lva_forward_bases_device"])
def test_null_decoder_is_an_argument_error(name):
    fn = getattr(_lib.load_library(), name)
    buf = np.zeros(64, np.int64)
    p = buf.ctypes.data
    where = (p, p) if name == "lva_forward_bases" else (p, p, p)
    assert fn(None, *where, 0, p, p, p, 0, p, 0, 5, p) == -10
    assert fn(None, *(None,) * len(where), 0, None, None, None, 0, None, 0, 5, None) == -10


def test_the_build_lists_the_kernel():
    import os
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nanopore_dna_storage_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert " fw_kernels.hip" in mk and " fw_kernels.h " in mk
