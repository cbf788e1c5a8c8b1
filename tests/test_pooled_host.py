"""The host side of a pooled run (no GPU): the experiment table, the yardstick helper.demux_barcodes against a loop of the
oracle's locate_payload plus a restatement of the selection rule, and synthetic pooled reads."""
import numpy as np
import pytest

from nanopore_dna_storage_amd import helper, pooled, synth

from demux_util import FIELDS, INF, random_experiments, select

HEADER = "\t".join(pooled.COLUMNS) + "\n"
SB0, EB0, SB1, EB1 = "ACGGTCAT", "TTGACCGA", "GGATCCAA", "CATTGGCT"


def _table(tmp_path, body, header=HEADER):
    p = tmp_path / "exp.tsv"
    p.write_text(header + body)
    return str(p)


def test_read_experiments_good(tmp_path):
    exps = pooled.read_experiments(_table(tmp_path, "a\tACGT\tTTGCA\t6\t1\t60\t4\nb.2\tACGTN\tGG\t8\t3\t44\t8\n\n"))
    assert exps == [dict(name="a", start_barcode="ACGT", end_barcode="TTGCA", mem_conv=6, rate_conv=1, msg_len=60, list_size=4),
                    dict(name="b.2", start_barcode="ACGTN", end_barcode="GG", mem_conv=8, rate_conv=3, msg_len=44, list_size=8)]
    assert helper.experiment_barcodes(exps[1]) == ("ACGTN", "GG", 8 + 44 + 1)


@pytest.mark.parametrize("body,what", [
    ("a\tACGT\tTTGCA\t6\t1\t60\t4\na\tACGT\tTTGCA\t6\t1\t60\t4\n", "duplicate"),
    ("a\tACGT\tTTGCA\t7\t1\t60\t4\n", "code"),                     # mem_conv 7 does not exist
    ("a\tACGT\tTTGCA\t6\t3\t44\t4\n", "code"),                     # odd output length
    ("a\tACXT\tTTGCA\t6\t1\t60\t4\n", "barcode"),
    ("a\tacgt\tTTGCA\t6\t1\t60\t4\n", "barcode"),
    ("a\t\tTTGCA\t6\t1\t60\t4\n", "barcode"),
    ("a\t" + "A" * 65 + "\tTTGCA\t6\t1\t60\t4\n", "barcode"),
    ("../a\tACGT\tTTGCA\t6\t1\t60\t4\n", "name"),
    ("a\tACGT\tTTGCA\t6\t1\t60\n", "columns"),
    ("a\tACGT\tTTGCA\t6\t1\t60\t0\n", "list_size"),
    ("", "experiments"),
])
def test_read_experiments_bad(tmp_path, body, what):
    with pytest.raises(ValueError) as e:
        pooled.read_experiments(_table(tmp_path, body))
    assert what in str(e.value)


def test_read_experiments_bad_header(tmp_path):
    with pytest.raises(ValueError):
        pooled.read_experiments(_table(tmp_path, "a\tACGT\tTTGCA\t6\t1\t60\t4\n", header="name\tstart\tend\n"))


def test_yardstick_on_pooled_reads(oracle):
    """5 experiments of seeded 25-mers, 12 clean reads, both strands: helper.demux_barcodes = the oracle's locate_payload per
    experiment + the restated rule, and every read goes to its true experiment"""
    exps = random_experiments(41, 5)
    reads, truth = synth.make_pooled_reads(exps, 12, seed0=4100, flank=(5, 14))
    assert len(set(truth)) >= 3 and len({x["rc"] for x in reads}) == 2
    for x, t in zip(reads, truth):
        bc, trans, _, _ = oracle.basecall(x["post"])
        got, table = helper.demux_barcodes(bc, trans, exps, all=True)
        cands = [oracle.locate_payload(x["post"], e["start_barcode"], e["end_barcode"], 6 + 60 + 1) for e in exps]
        cands = [{f: c[f] for f in FIELDS} for c in cands]
        assert table == cands
        assert got == select(cands)
        assert got["experiment"] == t and got["reason"] == 0 and got["ok"] and got["rc"] == x["rc"]
        assert got["runner_up_dist"] > got["dist_start"] + got["dist_end"]


def _read(sb, eb, payload=40, seed=0, f5=6, f3=7):
    rng = np.random.default_rng(seed)
    word = lambda n: "".join("ACGT"[int(v)] for v in rng.integers(0, 4, n))
    s = word(f5) + sb + word(payload) + eb + word(f3)
    return s, np.arange(1, len(s) + 1) * 3


def _loop(s, t, exps):
    out = []
    for sb, eb, min_len in exps:
        f = helper.find_barcode_pos(s, t, sb, eb)
        r = helper.find_barcode_pos(s, t, helper.reverse_complement(eb), helper.reverse_complement(sb))
        sp, ep, ds, de = r if f[2] + f[3] > r[2] + r[3] else f
        out.append(dict(ok=not (sp == -1 or ep - sp + 1 < min_len), start_pos=sp, end_pos=ep, rc=f[2] + f[3] > r[2] + r[3],
                        dist_start=ds, dist_end=de))
    return out


def test_reasons_by_hand():
    exps = [(SB0, EB0, 20), (SB1, EB1, 20)]
    s, t = _read(SB0, EB0)
    r0 = helper.demux_barcodes(s, t, exps)
    assert r0 == select(_loop(s, t, exps)) and r0["reason"] == 0 and r0["experiment"] == 0 and r0["ok"] and not r0["rc"]
    assert (r0["dist_start"], r0["dist_end"], r0["runner_up"]) == (0, 0, 1)
    # the other strand of experiment 1
    s1, t1 = _read(SB1, EB1, seed=1)
    s1 = helper.reverse_complement(s1)
    r = helper.demux_barcodes(s1, t1, exps)
    assert r == select(_loop(s1, t1, exps)) and (r["experiment"], r["reason"], r["rc"]) == (1, 0, True)
    # 1: too short for any pair
    r = helper.demux_barcodes("ACGTACGT", np.arange(1, 9), exps)
    assert r == dict(ok=False, start_pos=-1, end_pos=-1, rc=False, dist_start=INF, dist_end=INF, experiment=-1, reason=1,
                     runner_up=-1, runner_up_dist=INF)
    # 2: one substitution in the start barcode, max_dist 0 refuses, 1 accepts (total == max_dist passes)
    sm, tm = _read(SB0[:3] + "T" + SB0[4:], EB0, seed=2)
    assert SB0[3] != "T"
    r = helper.demux_barcodes(sm, tm, exps, max_dist=0)
    assert (r["reason"], r["experiment"], r["ok"], r["dist_start"] + r["dist_end"]) == (2, 0, False, 1)
    assert helper.demux_barcodes(sm, tm, exps, max_dist=1)["reason"] == 0
    assert helper.demux_barcodes(sm, tm, exps, max_dist=-1)["reason"] == 0
    # 3: the lead over the runner-up is lead; min_margin == lead passes, lead + 1 does not
    lead = r0["runner_up_dist"] - 0
    assert 0 < lead < INF
    assert helper.demux_barcodes(s, t, exps, min_margin=lead)["reason"] == 0
    r = helper.demux_barcodes(s, t, exps, min_margin=lead + 1)
    assert (r["reason"], r["experiment"], r["ok"], r["start_pos"]) == (3, 0, False, r0["start_pos"])
    # 4: the window is shorter than the winner's min_len
    width = r0["end_pos"] - r0["start_pos"] + 1
    assert helper.demux_barcodes(s, t, [(SB0, EB0, width), (SB1, EB1, 20)])["reason"] == 0
    r = helper.demux_barcodes(s, t, [(SB0, EB0, width + 1), (SB1, EB1, 20)])
    assert (r["reason"], r["experiment"], r["ok"], r["end_pos"]) == (4, 0, False, r0["end_pos"])
    # the order of the reasons: 2 before 3 before 4
    assert helper.demux_barcodes(sm, tm, [(SB0, EB0, 10 ** 6), (SB1, EB1, 20)], max_dist=0, min_margin=10 ** 6)["reason"] == 2
    assert helper.demux_barcodes(sm, tm, [(SB0, EB0, 10 ** 6), (SB1, EB1, 20)], max_dist=1, min_margin=10 ** 6)["reason"] == 3


def test_tie_and_single_experiment():
    s, t = _read(SB0, EB0, seed=3)
    twins = [(SB0, EB0, 20), (SB0, EB0, 20), (SB1, EB1, 20)]
    r = helper.demux_barcodes(s, t, twins)
    assert (r["experiment"], r["reason"], r["runner_up"], r["runner_up_dist"]) == (0, 0, 1, 0)
    assert r == select(_loop(s, t, twins))
    r = helper.demux_barcodes(s, t, twins, min_margin=1)
    assert (r["experiment"], r["reason"], r["ok"]) == (0, 3, False) and r == select(_loop(s, t, twins), None, 1)
    # K = 1: no runner-up, never ambiguous
    r = helper.demux_barcodes(s, t, [(SB0, EB0, 20)], min_margin=10 ** 9)
    assert (r["experiment"], r["reason"], r["runner_up"], r["runner_up_dist"]) == (0, 0, -1, INF)
    with pytest.raises(ValueError):
        helper.demux_barcodes(s, t, [])
    with pytest.raises(ValueError):
        helper.demux_barcodes(s, t, [(SB0, EB0, 20)] * 65)
    with pytest.raises(ValueError):
        helper.demux_barcodes(s, t, [(SB0, EB0, 20)], min_margin=-1)


def test_make_pooled_reads_assign_and_scores():
    exps = random_experiments(42, 3, msg_len=20)
    reads, truth = synth.make_pooled_reads(exps, 4, seed0=7, assign=[2, 0, 1, 2], rc_mode="odd", scores=True, flank=(2, 5))
    assert truth == [2, 0, 1, 2] and [x["rc"] for x in reads] == [False, True, False, True]
    assert all(x["scores"].shape[1] == 40 for x in reads)
    again, truth2 = synth.make_pooled_reads(exps, 4, seed0=7)
    assert truth2 == synth.make_pooled_reads(exps, 4, seed0=7)[1] and all("post" in x for x in again)
