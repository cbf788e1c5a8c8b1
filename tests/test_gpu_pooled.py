"""A pooled run end to end on the GPU (pooled.decode_pooled and the command line): three experiments with different codes
share one chunk; every read is assigned to its experiment and decoded with that experiment's code, bit for bit what the
single-experiment chain gives for it."""
import os

import numpy as np
import pytest

import nanopore_dna_storage_amd as pkg
from nanopore_dna_storage_amd import compute_error_rate_from_decoded_lists as cer
from nanopore_dna_storage_amd import pooled, synth

from demux_util import random_experiments

pytestmark = pytest.mark.gpu

CODES = [(6, 1, 60, 4), (6, 3, 48, 8), (8, 1, 24, 2)]          # mem_conv, rate_conv, msg_len, list_size


def _experiments():
    exps = random_experiments(49, 3)
    for x, (m, r, ml, ls) in zip(exps, CODES):
        x.update(mem_conv=m, rate_conv=r, msg_len=ml, list_size=ls)
    return exps


def _pool(scores):
    """four reads per experiment, shuffled, both strands"""
    exps = _experiments()
    assign = [int(e) for e in np.random.default_rng(50).permutation(np.repeat(np.arange(3), 4))]
    reads, truth = synth.make_pooled_reads(exps, 12, seed0=5000, assign=assign, rc_mode="odd", scores=scores, flank=(4, 12))
    assert truth == assign and sorted(truth) == [0] * 4 + [1] * 4 + [2] * 4
    return exps, reads, truth


def _same(a, b):
    assert (a is None) == (b is None)
    if a is None:
        return
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


def _check_against_single_chain(exps, posts, reads, truth, got):
    for e, x in enumerate(exps):
        mine = [i for i in range(len(posts)) if truth[i] == e]
        with pkg.Decoder(x["mem_conv"], x["rate_conv"], x["msg_len"], list_size=x["list_size"], max_deviation=20) as dec:
            want = dec.decode_with_barcodes([posts[i] for i in mine], x["start_barcode"], x["end_barcode"])
        for i, (loc, res) in zip(mine, want):
            g_loc, g_res = got[i]
            assert g_loc["experiment"] == e and g_loc["reason"] == 0 and g_loc["rc"] == reads[i]["rc"]
            assert {k: g_loc[k] for k in loc} == loc and loc["ok"]
            _same(g_res, res)
            assert np.array_equal(g_res[0][0], reads[i]["msg"])          # and the pooled chain recovers the message


def test_decode_pooled_posteriors():
    exps, reads, truth = _pool(scores=False)
    posts = [x["post"] for x in reads]
    got = pooled.decode_pooled(posts, exps)
    assert len(got) == 12
    _check_against_single_chain(exps, posts, reads, truth, got)
    assert pooled.decode_pooled([], exps) == []


def test_decode_pooled_scores():
    exps, reads, truth = _pool(scores=True)
    scores = [x["scores"] for x in reads]
    got = pooled.decode_pooled(scores, exps, input_kind="scores")
    with pkg.Decoder(6, 1, 60, max_slots=1) as front:
        posts = front.posteriors(scores)
    _check_against_single_chain(exps, posts, reads, truth, got)


def test_command_line(tmp_path, capsys):
    exps, reads, truth = _pool(scores=False)
    posts = [x["post"] for x in reads]
    posts.insert(5, np.random.default_rng(51).normal(0, 1, (30, 40)).astype(np.float32))      # flanks only: nothing to find
    truth = truth[:5] + [-1] + truth[5:]
    rows = []
    for i, p in enumerate(posts):
        path = str(tmp_path / ("read%d.post" % i))
        p.astype("<f4").tofile(path)
        rows.append("id%d\tref%d\t%s\n" % (i, i, path))
    (tmp_path / "reads.tsv").write_text("".join(rows))
    (tmp_path / "exp.tsv").write_text("\t".join(pooled.COLUMNS) + "\n" + "".join(
        "\t".join(str(x[c]) for c in pooled.COLUMNS) + "\n" for x in exps))
    out_dir = str(tmp_path / "out")
    assert pooled.main(["--experiments", str(tmp_path / "exp.tsv"), "--post_manifest", str(tmp_path / "reads.tsv"),
                        "--out_dir", out_dir, "--chunk", "8"]) == 0
    want = pooled.decode_pooled([p for i, p in enumerate(posts) if i != 5], exps)
    want.insert(5, None)
    for e, x in enumerate(exps):
        d = os.path.join(out_dir, x["name"])
        mine = [i for i in range(13) if truth[i] == e]
        assert sorted(f for f in os.listdir(d)) == sorted(["info.txt"] + ["list_%d" % i for i in mine])
        assert open(os.path.join(d, "info.txt")).read() == "".join("id%d\tref%d\n" % (i, i) for i in mine)
        lists = dict(cer.read_lists(d))                                   # what the list consumers read
        assert sorted(lists) == sorted("list_%d" % i for i in mine)
        for i in mine:
            assert lists["list_%d" % i] == ["".join(str(int(b)) for b in row) for row in want[i][1][0]]
    assert open(os.path.join(out_dir, "unassigned.tsv")).read() == "5\tid5\t1\t-1\tinf\t-1\tinf\n"
    text = capsys.readouterr().out
    for x in exps:
        assert "experiment %s 4" % x["name"] in text
    assert "reason 0 (assigned) 12" in text and "reason 1 (no barcode pair located) 1" in text
