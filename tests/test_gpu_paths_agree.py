"""Every path through the located chain -- locate, keep the reads that were found, decode their windows where they lie,
put the results back at their reads' positions -- gives the same lists, bit for bit, as a yardstick that shares none of it:
locate_payload on the posteriors, then decode() of helper.truncate_post's copies with the orientation that was found.
(The lists themselves are pinned to the reference by the golden tests; this pins the paths to each other.)"""
import numpy as np
import pytest

import nanopore_dna_storage_amd as pkg
from nanopore_dna_storage_amd import generate_decoded_lists, helper, pooled, synth

pytestmark = pytest.mark.gpu

SB, EB = "CACCTGTGCTGCGTCAGGCTGTGTC", "GCTGTCCGTTCCGCATTGACACGGC"
CODE = dict(mem_conv=6, rate_conv=1, msg_len=60, list_size=4)          # max deviation 20 throughout
EXPERIMENT = dict(name="only", start_barcode=SB, end_barcode=EB, **CODE)


def _plain(seed):
    """a read without barcodes: 66 bases, so whatever the search settles on is shorter than the code (67 blocks)"""
    return synth.make_read_scores(6, 1, 60, seed, rc=bool(seed & 1), margin=6.0)["scores"]


def _mixed():
    """six barcoded reads in alternating orientation, as tests/test_gpu_scores_chain.py makes them, and two reads whose
    barcodes cannot be found: second and last"""
    reads = [synth.make_barcoded_read_scores(6, 1, 60, 300 + i, SB, EB, rc=bool(i & 1), margin=6.0, flank=(8, 30))["scores"]
             for i in range(6)]
    return reads[:1] + [_plain(700)] + reads[1:] + [_plain(703)], [True, False] + [True] * 5 + [False]


def _nothing():
    noise = np.random.default_rng(51).normal(0, 1, (30, 40)).astype(np.float32)       # shorter than a barcode pair
    return [_plain(701), noise, _plain(702)], [False] * 3


def _same(got, want):
    assert (got is None) == (want is None)
    if want is not None:
        assert not isinstance(got, (int, np.integer)) and not isinstance(want, (int, np.integer)), (got, want)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


def _rows(tmp_path, kind, mats):
    rows = []
    for i, a in enumerate(mats):
        path = str(tmp_path / ("read%d.%s" % (i, kind)))
        a.astype("<f4").tofile(path)
        rows.append(("read%d" % i, "ref", path, None, None, None))
    return rows


@pytest.mark.parametrize("batch", [_mixed, _nothing], ids=["six_found_two_not", "nothing_found"])
def test_every_path_gives_the_yardsticks_lists(batch, tmp_path):
    scores, expect_found = batch()
    n = len(scores)
    with pkg.Decoder(6, 1, 60, list_size=4, max_deviation=20) as dec:
        posts = dec.posteriors(scores)
        # the yardstick
        loc = dec.locate_payload(posts, SB, EB)
        assert [lc["ok"] for lc in loc] == expect_found          # the batch is what this test means it to be
        found = [i for i in range(n) if loc[i]["ok"]]
        want = [None] * n
        if found:
            lists = dec.decode([helper.truncate_post(posts[i], loc[i]["start_pos"], loc[i]["end_pos"]) for i in found],
                               rc=[loc[i]["rc"] for i in found])
            for i, res in zip(found, lists):
                assert not isinstance(res, (int, np.integer)), res
                want[i] = res

        for name, got in (("decode_with_barcodes", dec.decode_with_barcodes(posts, SB, EB)),
                          ("decode_from_scores", dec.decode_from_scores(scores, start_barcode=SB, end_barcode=EB))):
            assert len(got) == n, name
            for i, (g_loc, g_res) in enumerate(got):
                assert g_loc == loc[i], (name, i)
                _same(g_res, want[i])

        for kind, mats in (("post", posts), ("scores", scores)):
            args = generate_decoded_lists.build_parser().parse_args(
                ["--post_manifest", "-", "--out_prefix", "-", "--info_file", "-", "--mem_conv", "6", "--msg_len", "60",
                 "--rate_conv", "1", "--list_size", "4", "--input_kind", kind, "--start_barcode", SB, "--end_barcode", EB])
            results, located = generate_decoded_lists.decode_rows(args, _rows(tmp_path, kind, mats), dec)
            assert len(results) == n and sorted(located) == list(range(n)), kind
            for i in range(n):
                assert located[i] == {k: loc[i][k] for k in ("start_pos", "end_pos", "rc")}, (kind, i)
                if want[i] is None:
                    assert results[i] == generate_decoded_lists.BARCODE_FAILURE, (kind, i)      # this path's "not found"
                else:
                    _same(results[i], want[i])

    for kind, mats in (("post", posts), ("scores", scores)):
        got = pooled.decode_pooled(mats, [EXPERIMENT], input_kind=kind)
        assert len(got) == n, kind
        for i, (g_loc, g_res) in enumerate(got):
            assert (g_loc["reason"] == 0) == expect_found[i] == g_loc["ok"], (kind, i)
            if expect_found[i]:
                assert g_loc["experiment"] == 0 and {k: g_loc[k] for k in loc[i]} == loc[i], (kind, i)
            _same(g_res, want[i])
