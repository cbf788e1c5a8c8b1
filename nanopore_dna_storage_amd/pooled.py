"""A pooled run: one sequencing run that holds several experiments, each with its own barcode pair and its own code.

The reference's real data is such a run -- thirteen experiments, the table of encode_experiments.py (:3-33, used at
:117-128).  It sorts the pooled reads by aligning them to every experiment's oligos (util/align_compute_stats.sh,
util/generate_read_id_file.py: minimap2 + samtools) and then runs generate_decoded_lists.py once per experiment with that
experiment's --start_barcode / --end_barcode and code.  Neither tool exists here; instead the barcodes themselves sort the
reads, on the device:

    upload a chunk once -> (scores: posteriors in place) -> ONE basecall per read, ONE search over every experiment's
    barcodes, ONE decision per read (Decoder.demux_resident: experiment, orientation, payload window)
    -> per experiment that won reads: its own Decoder decodes the winners' windows from the same resident buffer.

The experiments come from a tab-separated table with the header
    name  start_barcode  end_barcode  mem_conv  rate_conv  msg_len  list_size
(the reference's table is program text of the reference and is not shipped: write the TSV from encode_experiments.py).
Output per experiment, in the layout of generate_decoded_lists.py so that compute_error_rate_from_decoded_lists.py and
decode_RS_from_decoded_lists.py work on DIR/<name>/ unchanged:
    DIR/<name>/list_<i>    the decoded list of manifest row i
    DIR/<name>/info.txt    readid <TAB> ref of the reads assigned to the experiment
    DIR/unassigned.tsv     i, readid, reason, experiment, total, runner_up, runner_up_dist (tab-separated, no header) of
                           every read that was not assigned (reasons: helper.DEMUX_REASONS; `inf`: no such distance)

Out of scope here: --gpus, --resume, decode streams and the decode server for pooled input (generate_decoded_lists.py has
them for a single experiment; a pooled run can be demultiplexed here and its groups handed to them).
"""
import argparse
import os
import re
import sys

import numpy as np

from . import helper
from .decoder import Decoder, code_info
from .generate_decoded_lists import publish_list_files, write_list_temp

COLUMNS = ["name", "start_barcode", "end_barcode", "mem_conv", "rate_conv", "msg_len", "list_size"]
_NAME = re.compile(r"^[A-Za-z0-9][A-Za-z0-9._-]*$")
FRONT_CODE = (6, 1, 60)             # the front decoder only basecalls and searches: any valid code, one slot


def read_experiments(path):
    """The experiment table -> [dict(name, start_barcode, end_barcode, mem_conv, rate_conv, msg_len, list_size)].
    ValueError on: a wrong header, a wrong column count, a name that is not unique or not usable as a directory name,
    a barcode that is empty, longer than 64 or has a character outside ACGTN, a code code_info refuses, list_size < 1,
    no experiment or more than 64."""
    with open(path) as f:
        lines = [ln.rstrip("\n").rstrip("\r") for ln in f]
    lines = [ln for ln in lines if ln.strip()]
    if not lines or lines[0].split("\t") != COLUMNS:
        raise ValueError("%s: the first line must be %s" % (path, "<TAB>".join(COLUMNS)))
    exps, seen = [], set()
    for no, ln in enumerate(lines[1:], 2):
        cols = ln.split("\t")
        if len(cols) != len(COLUMNS):
            raise ValueError("%s line %d: %d columns, expected %d" % (path, no, len(cols), len(COLUMNS)))
        name, sb, eb = cols[:3]
        if not _NAME.match(name) or name in (".", ".."):
            raise ValueError("%s line %d: name %r is not usable as a directory name" % (path, no, name))
        if name in seen:
            raise ValueError("%s line %d: duplicate name %r" % (path, no, name))
        seen.add(name)
        for bc in (sb, eb):
            if not 1 <= len(bc) <= 64 or any(ch not in "ACGTN" for ch in bc):
                raise ValueError("%s line %d: barcode %r (1..64 characters out of ACGTN)" % (path, no, bc))
        try:
            m, r, ml, ls = (int(x) for x in cols[3:])
        except ValueError:
            raise ValueError("%s line %d: mem_conv, rate_conv, msg_len, list_size are integers" % (path, no))
        try:
            code_info(m, r, ml)
        except Exception as e:
            raise ValueError("%s line %d: code (m %d, rate %d, msg_len %d): %s" % (path, no, m, r, ml, e))
        if not 1 <= ls <= 65535:
            raise ValueError("%s line %d: list_size %d" % (path, no, ls))
        exps.append(dict(name=name, start_barcode=sb, end_barcode=eb, mem_conv=m, rate_conv=r, msg_len=ml, list_size=ls))
    if not 1 <= len(exps) <= 64:
        raise ValueError("%s: %d experiments (1..64)" % (path, len(exps)))
    return exps


def decode_pooled(inputs, experiments, device=0, input_kind="post", max_dist=None, min_margin=0, max_deviation=20):
    """inputs: float32 [nblk_i, 40] matrices of one chunk (posteriors, or input_kind="scores": a network's transition
    scores); experiments: what read_experiments returns.  -> [(demux dict, list | negative code | None)] per read: the
    second item is what Decoder.decode gives for the read's payload window under ITS experiment's code, None when the read
    was not assigned (demux dict's reason != 0).
    The chunk is uploaded once; at most two decoders are alive at a time: the front decoder, which only reserves one slot
    of a small trellis, and the decoder of the experiment being decoded.  All calls are complete on return and a buffer of
    lva_device_alloc is a plain device allocation, so the decoders share it."""
    if input_kind not in ("post", "scores"):
        raise ValueError("input_kind: 'post' or 'scores'")
    n = len(inputs)
    out = [None] * n
    if n == 0:
        return []
    with Decoder(*FRONT_CODE, list_size=1, device=device, max_slots=1) as front, front.resident(inputs) as (dev, off):
        if input_kind == "scores":
            front.posteriors_resident(dev, off)
        loc = front.demux_resident(dev, off, experiments, max_dist=max_dist, min_margin=min_margin)
        out = [(lc, None) for lc in loc]
        for e, x in enumerate(experiments):
            mine = [i for i in range(n) if loc[i]["reason"] == 0 and loc[i]["experiment"] == e]
            if not mine:
                continue
            with Decoder(x["mem_conv"], x["rate_conv"], x["msg_len"], list_size=x["list_size"], max_deviation=max_deviation,
                         device=device) as dec:
                res = dec.decode_located(dev, off, loc, mine)
            for i in mine:
                out[i] = res[i]
    return out


def build_parser():
    p = argparse.ArgumentParser(description="demultiplex a pooled run by barcode pair and decode every experiment's reads")
    p.add_argument("--experiments", type=str, required=True, help="TSV: " + " ".join(COLUMNS))
    p.add_argument("--post_manifest", type=str, required=True, help="TSV rows: readid ref post_path")
    p.add_argument("--out_dir", type=str, required=True)
    p.add_argument("--input_kind", choices=["post", "scores"], default="post")
    p.add_argument("--max_dist", type=int, default=None, help="largest start + end barcode distance that is still assigned")
    p.add_argument("--min_margin", type=int, default=0, help="smallest lead over the next experiment that is still assigned")
    p.add_argument("--max_deviation", type=int, default=20)
    p.add_argument("--chunk", type=int, default=4096, help="reads uploaded, demultiplexed and decoded per pass")
    p.add_argument("--device", type=int, default=0)
    return p


def read_manifest(path):
    rows = []
    with open(path) as f:
        for no, line in enumerate(f, 1):
            line = line.rstrip("\n")
            if not line:
                continue
            cols = line.split("\t")
            if len(cols) != 3:
                raise SystemExit("%s line %d: rows are readid<TAB>ref<TAB>post_path" % (path, no))
            rows.append(tuple(cols))
    return rows


def _num(x):
    return "inf" if x == float("inf") else str(int(x))


def run(args, out=None):
    out = sys.stdout if out is None else out
    exps = read_experiments(args.experiments)
    rows = read_manifest(args.post_manifest)
    os.makedirs(args.out_dir, exist_ok=True)
    for x in exps:
        os.makedirs(os.path.join(args.out_dir, x["name"]), exist_ok=True)
    infos = [open(os.path.join(args.out_dir, x["name"], "info.txt"), "w") for x in exps]
    per_exp, per_reason, written = [0] * len(exps), {r: 0 for r in helper.DEMUX_REASONS}, 0
    chunk = max(1, int(args.chunk))
    try:
        with open(os.path.join(args.out_dir, "unassigned.tsv"), "w") as un:
            for k in range(0, len(rows), chunk):
                part = rows[k:k + chunk]
                res = decode_pooled([helper.read_post_file(r[2]) for r in part], exps, device=args.device,
                                    input_kind=args.input_kind, max_dist=args.max_dist, min_margin=args.min_margin,
                                    max_deviation=args.max_deviation)
                pending = []
                for j, ((rid, ref, _), (loc, lst)) in enumerate(zip(part, res)):
                    i = k + j
                    per_reason[loc["reason"]] += 1
                    if loc["reason"] != 0:
                        un.write("\t".join([str(i), rid, str(loc["reason"]), str(loc["experiment"]),
                                            _num(loc["dist_start"] + loc["dist_end"]), str(loc["runner_up"]),
                                            _num(loc["runner_up_dist"])]) + "\n")
                        continue
                    e = loc["experiment"]
                    per_exp[e] += 1
                    infos[e].write(rid + "\t" + ref + "\n")
                    if isinstance(lst, (int, np.integer)):
                        continue       # (the reference decoder aborts on such a read: no list file)
                    pending.append(write_list_temp(os.path.join(args.out_dir, exps[e]["name"], "list_" + str(i)), lst[0]))
                written += publish_list_files(pending)
                for f in infos:
                    f.flush()
    finally:
        for f in infos:
            f.close()
    print("reads", len(rows), "lists written", written, file=out)
    for x, c in zip(exps, per_exp):
        print("experiment", x["name"], c, file=out)
    for r in sorted(per_reason):
        print("reason", r, "(%s)" % helper.DEMUX_REASONS[r], per_reason[r], file=out)
    return written


def main(argv=None):
    args = build_parser().parse_args(argv)
    run(args)
    return 0


if __name__ == "__main__":
    sys.exit(main())
