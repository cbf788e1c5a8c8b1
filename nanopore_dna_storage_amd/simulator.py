"""Counterpart of the reference's simulator.py for this path: same CLI flags, same per-trial
and summary statistics (simulator.py:15-27, :86-126), with the scrappy + flappie signal chain
replaced by the deterministic synthetic posterior generator (synth.py; neither dependency can
run here) and all trials decoded in one GPU batch.

    python -m nanopore_dna_storage_amd.simulator --num_trials 100 --list_size 1 --mem_conv 6 \
        --rate 1 --msg_len 180
"""
import argparse
import math
import sys

import numpy as np

from . import helper, synth
from .decoder import Decoder, bases_to_str, encode


def build_parser():
    p = argparse.ArgumentParser(description="Simulation for convolutional code.")
    p.add_argument("--num_trials", type=int, default=100)
    p.add_argument("--list_size", type=int, default=1)
    p.add_argument("--num_thr", type=int, default=8)          # accepted, unused on the GPU
    p.add_argument("--mem_conv", type=int, default=6)
    p.add_argument("--rate", type=int, default=1)
    p.add_argument("--msg_len", type=int, default=100)
    p.add_argument("--deepsimdwell", type=str, default="False")   # accepted, unused (no signal simulator)
    p.add_argument("--reversecomp", type=str, default="False")
    p.add_argument("--syn_sub_prob", type=float, default=0.002)
    p.add_argument("--syn_del_prob", type=float, default=0.0085)
    p.add_argument("--syn_ins_prob", type=float, default=0.0005)
    # extensions
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--margin", type=float, default=6.0)
    p.add_argument("--max_deviation", type=int, default=20)
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--synth", choices=["host", "device"], default="host",
                   help="where the reads are made: synth.py on the host, or the counter-based simulator on the GPU "
                        "(Decoder.simulate: the reference's insertion / deletion / substitution rules, transition scores)")
    p.add_argument("--stats", choices=["host", "device"], default="host",
                   help="where the per-trial statistics are computed: Python loops, or the GPU (list_ops.list_stats); same output")
    p.add_argument("--truth_score", action="store_true",
                   help="score every trial's true message on the decoder's trellis (trellis_score.py) and add to the summary, "
                        "per verdict, why a list missed it: the list was too short, or the band cut its path")
    return p


def run(args, out=sys.stdout, decoder=None):
    revcomp = args.reversecomp != "False"
    on_device = getattr(args, "synth", "host") == "device"
    if not on_device:
        reads = [synth.make_read(args.mem_conv, args.rate, args.msg_len, args.seed + i, rc=revcomp,
                                 margin=args.margin, sub=args.syn_sub_prob, dele=args.syn_del_prob,
                                 ins=args.syn_ins_prob) for i in range(args.num_trials)]
    own = decoder is None
    if own:
        decoder = Decoder(args.mem_conv, args.rate, args.msg_len, list_size=args.list_size,
                          max_deviation=args.max_deviation, device=args.device)
    rows = None
    try:
        if on_device and getattr(args, "truth_score", False):      # the same chain, the truth scored on the buffer the decode read
            from . import trellis_score
            truth, results, rows = trellis_score.simulate_rows(decoder, args.num_trials, args.seed, margin=args.margin,
                                                               sub=args.syn_sub_prob, dele=args.syn_del_prob, ins=args.syn_ins_prob,
                                                               rc_mode=int(revcomp))
            oligos = encode(args.mem_conv, args.rate, args.msg_len, truth["msgs"]) if args.num_trials else []
            reads = [dict(msg=m, oligo=o) for m, o in zip(truth["msgs"], oligos)]
        elif on_device:      # reads made, turned into posteriors and decoded on the device: the truth is all that comes back
            truth, results = decoder.simulate_and_decode(args.num_trials, args.seed, margin=args.margin, sub=args.syn_sub_prob,
                                                         dele=args.syn_del_prob, ins=args.syn_ins_prob, rc_mode=int(revcomp))
            oligos = encode(args.mem_conv, args.rate, args.msg_len, truth["msgs"]) if args.num_trials else []
            reads = [dict(msg=m, oligo=o) for m, o in zip(truth["msgs"], oligos)]
        else:
            if getattr(args, "truth_score", False):
                from . import trellis_score
                with decoder.resident([r["post"] for r in reads]) as (dev, off):
                    results = decoder.decode_resident(dev, off, [revcomp] * len(reads))
                    rows = trellis_score.truth_rows(decoder, dev, off[:-1], np.diff(off), results,
                                                    np.array([r["msg"] for r in reads], dtype=np.uint8).reshape(len(reads), -1),
                                                    [revcomp] * len(reads))
            else:
                results = decoder.decode([r["post"] for r in reads], rc=[revcomp] * len(reads))
    finally:
        if own:
            decoder.close()
    return report(args, reads, results, out, truth_rows=rows)


def report(args, reads, results, out=sys.stdout, truth_rows=None):
    """The per-trial and summary statistics (simulator.py:92-126) of decoded reads: reads = dicts with msg and oligo, results
    = what Decoder.decode returns for them.  Prints the reference's text to `out` -> the summary statistics.  truth_rows
    (--truth_score: trellis_score.truth_rows of the same reads): the count per verdict joins the summary."""
    top, lst, ham, ham8, ham16, edit = [], [], [], [], [], []
    n = args.msg_len
    dev = None
    if getattr(args, "stats", "host") == "device" and reads and not any(isinstance(res, int) or not len(res[0]) for res in results):
        from . import list_ops
        msgs, counts = list_ops.results_to_array(results, max(len(res[0]) for res in results), n)
        dev = list_ops.list_stats(msgs, counts, np.array([rd["msg"] for rd in reads], dtype=np.uint8), device=args.device)
    for t, (rd, res) in enumerate(zip(reads, results)):
        msg = "".join(map(str, rd["msg"]))
        print(msg, file=out)
        print("len(seq):", len(bases_to_str(rd["oligo"])), file=out)
        decoded = ["".join(map(str, row)) for row in res[0]] if not isinstance(res, int) else []
        if not decoded:
            raise RuntimeError("decoder produced no list (the reference would crash reading its output file)")
        print("Top message:", file=out)
        print(decoded[0], file=out)
        print("List size:", len(decoded), file=out)
        if dev is not None:
            top.append(bool(dev["top_correct"][t]))
            lst.append(bool(dev["list_correct"][t]))
        else:
            top.append(decoded[0] == msg)
            lst.append(msg in decoded)
        print("Top correct:", top[-1], file=out)
        print("List correct:", lst[-1], file=out)
        if dev is not None:
            ham.append(int(dev["hamming"][t]))
            ham8.append(int(dev["hamming8"][t]))
            ham16.append(int(dev["hamming16"][t]))
        else:
            ham.append(helper.hamming(msg, decoded[0]))
            ham8.append(sum(decoded[0][i * 8:(i + 1) * 8] != msg[i * 8:(i + 1) * 8] for i in range(math.ceil(n / 8))))
            ham16.append(sum(decoded[0][i * 16:(i + 1) * 16] != msg[i * 16:(i + 1) * 16] for i in range(math.ceil(n / 16))))
        print("Hamming distance of top:", ham[-1], file=out)
        print("Hamming distance of top (8 blocks):", ham8[-1], file=out)
        print("Hamming distance of top (16 blocks):", ham16[-1], file=out)
        edit.append(int(dev["edit"][t]) if dev is not None else helper.levenshtein(msg, decoded[0]))
        print("Edit distance", edit[-1], file=out)
        if not top[-1]:
            print("Error pattern (original, errors):", file=out)
            print(msg, file=out)
            print("".join(m if m == d else "*" for m, d in zip(msg, decoded[0])), file=out)
    T = args.num_trials
    stats = {
        "Number total": T,
        "Number top correct": sum(top),
        "Number list correct": sum(lst),
        "Average bit error rate of top": sum(ham) / (n * T) if T else 0.0,
        "Average 8 block error rate of top": sum(ham8) / (math.ceil(n / 8) * T) if T else 0.0,
        "Average 16 block error rate of top": sum(ham16) / (math.ceil(n / 16) * T) if T else 0.0,
        "Average edit distance rate of top": sum(edit) / (n * T) if T else 0.0,
    }
    if truth_rows is not None:
        from . import trellis_score
        for verdict, count in trellis_score.count_verdicts(truth_rows).items():
            stats["Number truth " + verdict] = count
        stats["Number truth band dev_needed"] = trellis_score.band_dev_needed(truth_rows)    # the max_deviation that keeps them all
    print("Summary statistics:", file=out)
    for k, v in stats.items():
        print(k + ":", v, file=out)
    return stats


def main(argv=None):
    args = build_parser().parse_args(argv)
    print(args)
    run(args)
    return 0


if __name__ == "__main__":
    sys.exit(main())
