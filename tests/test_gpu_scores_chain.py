"""scores -> posteriors -> basecall -> barcode -> window -> lists -> RS on the device: Decoder.decode_from_scores and the
drivers that start from a network's raw transition scores."""
import filecmp
import io
import os

import numpy as np
import pytest

import nanopore_dna_storage_amd as pkg
from nanopore_dna_storage_amd import generate_decoded_lists, helper, synth, viterbi_nanopore
from transpost_cases import CLEAN_CASES, clean_reads

pytestmark = pytest.mark.gpu

SB, EB = "CACCTGTGCTGCGTCAGGCTGTGTC", "GCTGTCCGTTCCGCATTGACACGGC"


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert not isinstance(x, int) and not isinstance(y, int), (x, y)
        assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1])


@pytest.mark.parametrize("case", CLEAN_CASES, ids=lambda c: "m%d" % c["mem_conv"])
def test_clean_reads_decode_from_scores(case):
    """the seeds tests/test_transpost_ref.py holds the CPU oracle to"""
    reads = clean_reads(case)
    scores, rc = [x["scores"] for x in reads], [x["rc"] for x in reads]
    with pkg.Decoder(case["mem_conv"], case["rate"], case["msg_len"], list_size=case["list_size"],
                     max_deviation=case["max_deviation"]) as dec:
        got = dec.decode_from_scores(scores, rc=rc)
        two_steps = dec.decode(dec.posteriors(scores), rc=rc)
    for x, g in zip(reads, got):
        assert not isinstance(g, int), g
        assert np.array_equal(g[0][0], x["msg"]), x["seed"]
    _same(got, two_steps)


def _barcoded(n=6):
    return [synth.make_barcoded_read_scores(6, 1, 60, 300 + i, SB, EB, rc=bool(i & 1), margin=6.0, flank=(8, 30)) for i in range(n)]


def test_barcoded_reads_decode_from_scores():
    reads = _barcoded()
    scores = [x["scores"] for x in reads]
    with pkg.Decoder(6, 1, 60, list_size=4, max_deviation=20) as dec:
        got = dec.decode_from_scores(scores, start_barcode=SB, end_barcode=EB)
        want = dec.decode_with_barcodes(dec.posteriors(scores), SB, EB)
    for x, (loc, res), (wloc, wres) in zip(reads, got, want):
        assert loc == wloc and loc["ok"] and loc["rc"] == x["rc"]
        assert res is not None and not isinstance(res, int)
        assert np.array_equal(res[0][0], x["msg"]), x["seed"]
        assert np.array_equal(res[0], wres[0]) and np.array_equal(res[1], wres[1])


_TORCH_WORKER = r"""
import sys
import torch
torch.cuda.init()                  # torch first: the decoder library then joins the HIP runtime torch has loaded (INTEGRATION section 2)
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import numpy as np
import nanopore_dna_storage_amd as pkg
from nanopore_dna_storage_amd import synth
from transpost_cases import CLEAN_CASES, clean_reads
SB, EB = sys.argv[3], sys.argv[4]
case = CLEAN_CASES[1]
reads = clean_reads(case)
scores, rc = [x["scores"] for x in reads], [x["rc"] for x in reads]
breads = [synth.make_barcoded_read_scores(6, 1, 60, 300 + i, SB, EB, rc=bool(i & 1), margin=6.0, flank=(8, 30)) for i in range(4)]
with pkg.Decoder(case["mem_conv"], case["rate"], case["msg_len"], list_size=case["list_size"],
                 max_deviation=case["max_deviation"], device=0) as dec:
    flat, off = dec.pack(scores)
    t = torch.from_numpy(flat).to("cuda:0")
    before = t.clone()
    got = dec.decode_from_scores(t, rc=rc, offsets=off)
    want = dec.decode_from_scores(scores, rc=rc)
    assert torch.equal(t, before), "the caller's tensor was modified"
    assert len(got) == len(want) == len(reads)
    for x, g, w in zip(reads, got, want):
        assert np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]) and np.array_equal(g[0][0], x["msg"])
    flat, off = dec.pack([x["scores"] for x in breads])
    t = torch.from_numpy(flat).to("cuda:0")
    got = dec.decode_from_scores(t, offsets=torch.from_numpy(off), start_barcode=SB, end_barcode=EB)
    want = dec.decode_from_scores([x["scores"] for x in breads], start_barcode=SB, end_barcode=EB)
    for (l1, r1), (l2, r2) in zip(got, want):
        assert l1 == l2 and l1["ok"] and np.array_equal(r1[0], r2[0]) and np.array_equal(r1[1], r2[1])
    for bad in (t.double(), t.cpu(), t[:, :39]):
        try:
            dec.decode_from_scores(bad, offsets=off)
        except ValueError:
            continue
        raise AssertionError("a tensor the call cannot take was accepted")
print("torch path ok")
"""


def test_torch_tensor_input():
    """a float32 tensor on the decoder's device goes in by pointer: same lists as the numpy path, the tensor unchanged.  In a
    fresh child process that initialises torch before the decoder library, as a caller with a network of its own does."""
    pytest.importorskip("torch")
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-c", _TORCH_WORKER, os.path.dirname(here), here, SB, EB], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and "torch path ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def _lists(d, prefix="list"):
    return {n: open(os.path.join(d, n)).read() for n in sorted(os.listdir(d)) if n.startswith(prefix + "_")}


def test_generate_decoded_lists_from_scores(tmp_path):
    """--input_kind scores writes the list files --input_kind post writes from the .post files `-m posterior` made of the same
    scores: rows with a block range, rows that go through the barcode search, and a --resume over a half-finished directory"""
    n = 10
    rows_s, rows_p, rows_bs, rows_bp = [], [], [], []
    for i in range(n):
        x = synth.make_read_scores(6, 1, 60, 400 + i, rc=bool(i & 1), margin=5.0, sub=0.01)
        sp, pp = tmp_path / ("r%d.scores" % i), tmp_path / ("r%d.post" % i)
        x["scores"].tofile(sp)
        assert viterbi_nanopore.main(["-m", "posterior", "-i", str(sp), "-o", str(pp)], out=io.StringIO()) == 0
        lo, hi = (3, x["scores"].shape[0] - 4) if i % 3 == 0 else (0, x["scores"].shape[0] - 1)
        rows_s.append("read%d\tref\t%s\t%d\t%d\t%d" % (i, sp, lo, hi, int(x["rc"])))
        rows_p.append("read%d\tref\t%s\t%d\t%d\t%d" % (i, pp, lo, hi, int(x["rc"])))
        b = synth.make_barcoded_read_scores(6, 1, 60, 500 + i, SB, EB, rc=bool(i & 1), margin=6.0, flank=(8, 30))
        sp, pp = tmp_path / ("b%d.scores" % i), tmp_path / ("b%d.post" % i)
        b["scores"].tofile(sp)
        assert viterbi_nanopore.main(["-m", "posterior", "-i", str(sp), "-o", str(pp)], out=io.StringIO()) == 0
        rows_bs.append("bread%d\tref\t%s" % (i, sp))
        rows_bp.append("bread%d\tref\t%s" % (i, pp))

    def run(name, rows, kind, extra=()):
        d = tmp_path / name
        d.mkdir(exist_ok=True)
        man = tmp_path / (name + ".tsv")
        man.write_text("\n".join(rows) + "\n")
        args = generate_decoded_lists.build_parser().parse_args(
            ["--post_manifest", str(man), "--out_prefix", str(d / "list"), "--info_file", str(tmp_path / (name + ".info")),
             "--mem_conv", "6", "--msg_len", "60", "--rate_conv", "1", "--list_size", "4", "--chunk", "4", "--input_kind", kind,
             "--start_barcode", SB, "--end_barcode", EB] + list(extra))
        out = io.StringIO()
        return generate_decoded_lists.run(args, out=out), str(d), out.getvalue()

    w_p, d_p, _ = run("post", rows_p, "post")
    w_s, d_s, _ = run("scores", rows_s, "scores")
    assert w_p == w_s == n and _lists(d_s) == _lists(d_p) and len(_lists(d_p)) == n
    w_bp, d_bp, t_bp = run("bpost", rows_bp, "post")
    w_bs, d_bs, t_bs = run("bscores", rows_bs, "scores")
    assert w_bp == w_bs and w_bs > n // 2 and _lists(d_bs) == _lists(d_bp) and t_bs == t_bp
    # a mixed manifest, half finished, then --resume
    mixed_s = [r for pair in zip(rows_s, rows_bs) for r in pair]
    mixed_p = [r for pair in zip(rows_p, rows_bp) for r in pair]
    w_mp, d_mp, _ = run("mpost", mixed_p, "post")
    w_ms, d_ms, _ = run("mscores", mixed_s, "scores")
    assert w_mp == w_ms == n + w_bs and _lists(d_ms) == _lists(d_mp)
    full = _lists(d_ms)
    gone = list(full)[1::2]
    for name in gone:
        os.remove(os.path.join(d_ms, name))
    w_again, _, _ = run("mscores", mixed_s, "scores", extra=["--resume"])
    assert w_again == len(gone) and _lists(d_ms) == full


def test_simulate_and_decode_with_crf_posteriors(tmp_path):
    """test_gpu_chain.py's 1 kB round trip (m=8, rate 3/4, 18 bytes per oligo, 30 % RS, list 8, 400 reads, the channel's default
    substitutions / deletions / insertions) with posterior_source='crf'.  That test's margin 4.3 was tuned for log-softmax
    posteriors; forward-backward posteriors of clipped scores are another channel, so the margin is fixed here at 5.0, where
    the CPU oracle (list 8, max deviation 20, on the float32 cast of the float64 posteriors) has the message in the list for
    11 of 12 sample reads drawn the same way -- as at margin 4.0; RS needs 56 of the 72 oligos, about 0.4 of 400 reads."""
    p = tmp_path / "myfile_1K"
    p.write_bytes(bytes(np.random.default_rng(5).integers(0, 256, size=1000, dtype=np.uint8)))
    infile = str(p)
    helper.encode(data_file=infile, oligo_file=infile + ".oligos", bytes_per_oligo=18, RS_redundancy=0.3, conv_m=8, conv_r=3,
                  pad=False, out=io.StringIO())
    r = helper.simulate_and_decode(oligo_file=infile + ".oligos", decoded_data_file=infile + ".decoded", num_reads=400,
                                   data_file_size=1000, bytes_per_oligo=18, RS_redundancy=0.3, conv_m=8, conv_r=3, pad=False,
                                   list_size=8, seed=77, margin=5.0, out=io.StringIO(), posterior_source="crf")
    assert filecmp.cmp(infile, infile + ".decoded", shallow=False)
    assert r["num_attempted"] == 400 and r["num_unique"] >= 56
    with pytest.raises(ValueError):
        helper.simulate_and_decode(infile + ".oligos", infile + ".x", 1, 1000, 18, 0.3, 8, 3, posterior_source="flappie")
