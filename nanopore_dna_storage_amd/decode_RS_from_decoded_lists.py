"""Counterpart of the reference's decode_RS_from_decoded_lists.py (:1-66): NUM_TRIALS times draw NUM_READS_TO_USE of the
NUM_READS_TOTAL read numbers, run the CRC-8 / index filter over `list_<i>` of every drawn read that has a list, take the
per-index consensus payload (:37-51), RS-decode (rs_code.MainDecoder on the GPU) and compare with the original file.
The reference's constants are flags here (same names, lower case); --seed fixes the draws.

--num_reads_to_use takes one sample size or an ascending comma-separated list of them (a reading-cost curve); the
reference's lines are printed once per size.  --trials host: the loop above, the draws Python's random.sample.
--trials device: every list file is read and filtered once, then all sizes and trials are one call (trials.run_trials:
the draws are trials.py's keyed permutation of the read numbers under --seed, the samples of one trial nested)."""
import argparse
import math
import os
import random
import sys

import numpy as np

from . import helper, rs_code


def sample_sizes(text):
    """'300' or '100,200,300' -> [300] / [100, 200, 300]"""
    try:
        sizes = [int(x) for x in text.split(",")]
    except ValueError:
        raise argparse.ArgumentTypeError("an integer or a comma-separated list of integers: %r" % (text,))
    if any(b < a for a, b in zip(sizes, sizes[1:])):
        raise argparse.ArgumentTypeError("sample sizes must be ascending: %r" % (text,))
    return sizes


def build_parser():
    p = argparse.ArgumentParser(description="outer-code decoding from decoded lists")
    p.add_argument("--num_trials", type=int, default=10)
    p.add_argument("--list_size", type=int, default=8)
    p.add_argument("--num_reads_total", type=int, required=True)
    p.add_argument("--num_reads_to_use", type=sample_sizes, required=True, help="a sample size, or an ascending comma-separated list")
    p.add_argument("--bytes_per_oligo", type=int, default=18)
    p.add_argument("--decoded_lists_dir", type=str, required=True)
    p.add_argument("--rs_redundancy", type=float, default=0.3)
    p.add_argument("--pad", action="store_true")
    p.add_argument("--original_file", type=str, required=True)
    p.add_argument("--seed", type=int, default=None)
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--list_ops", choices=["host", "device"], default="host", help="filter and consensus as Python loops, or on the GPU; same output")
    p.add_argument("--trials", choices=["host", "device"], default="host",
                   help="host: one filter / consensus / RS call per trial, draws by random.sample; device: all trials and sample "
                        "sizes in one call, draws by the keyed permutation of trials.py (needs --seed)")
    return p


def read_list(a, i):
    """list_<i> cut to --list_size, or None when the read has no list file"""
    list_file = os.path.join(a.decoded_lists_dir, "list_" + str(i))
    if not os.path.isfile(list_file):
        return None
    with open(list_file) as f:
        return [ln.rstrip("\n") for ln in f.readlines()][:a.list_size]


def filter_all(a, num_oligos):
    """the filter over every read number, once: (index int32 [n] with -1 for no list or no passing entry, payload uint8 [n, b])"""
    n = a.num_reads_total
    lists = [read_list(a, i) or [] for i in range(n)]
    if a.list_ops == "device":
        from . import list_ops as lo
        msg_len = helper.index_len + helper.crc_len + 8 * a.bytes_per_oligo + int(bool(a.pad))
        msgs, counts = lo.lists_to_array(lists, msg_len=msg_len)
        index, _, payload = lo.filter_lists(msgs, counts, a.bytes_per_oligo, num_oligos, pad=a.pad, device=a.device)
        return index, payload
    index = np.full(n, -1, np.int32)
    payload = np.zeros((n, a.bytes_per_oligo), np.uint8)
    for i, lst in enumerate(lists):
        k, p, _ = helper.decode_list_CRC_index(lst, a.bytes_per_oligo, num_oligos, a.pad)
        if k is not None:
            index[i] = k
            payload[i] = np.frombuffer(p, np.uint8)
    return index, payload


def print_curve(sizes, list_size, num_trials, trial, out):
    """the reference's lines, once per sample size: trial(k, t) -> whether trial t of sizes[k] recovered the file, asked in
    the order printed.  -> the successes of the last size"""
    num_successes = 0
    for k, num_reads_to_use in enumerate(sizes):
        print("NUM_READS_TO_USE:", num_reads_to_use, file=out)
        print("list size:", list_size, file=out)
        num_successes = 0
        for t in range(num_trials):
            ok = trial(k, t)
            num_successes += int(ok)
            print("Success" if ok else "Failure", file=out)
        print("NUM_TRIALS", num_trials, file=out)
        print("num_successes", num_successes, file=out)
    return num_successes


def main(argv=None, out=sys.stdout):
    parser = build_parser()
    a = parser.parse_args(argv)
    if a.trials == "device" and a.seed is None:
        parser.error("--trials device needs --seed: the draws are a function of the seed and the trial number")
    rnd = random.Random(a.seed)
    with open(a.original_file, "rb") as f:
        original = f.read()
    data_file_size = len(original)
    data_size_padded = math.ceil(data_file_size / a.bytes_per_oligo) * a.bytes_per_oligo
    msg_len, num_oligos_data, num_oligos_RS, num_oligos = helper.compute_parameters(a.bytes_per_oligo, a.rs_redundancy, data_size_padded, a.pad)
    if a.trials == "device":
        from . import trials
        index, payload = filter_all(a, num_oligos)
        stats = trials.run_trials(index, payload, original, a.bytes_per_oligo, num_oligos_RS, num_oligos, a.num_reads_to_use,
                                  a.num_trials, a.seed, device=a.device)

    def trial(k, t):
        if a.trials == "device":
            return bool(stats[k, t, 3])
        lists = [lst for lst in (read_list(a, i) for i in rnd.sample(list(range(a.num_reads_total)), a.num_reads_to_use[k]))
                 if lst is not None]
        data, passed = rs_code.decode_from_lists(lists, a.bytes_per_oligo, num_oligos_RS, num_oligos, pad=a.pad, device=a.device,
                                                 list_ops=a.list_ops)
        return passed > 0 and data[:data_file_size] == original     # no read passed the filter: the reference dies in MainDecoder

    return print_curve(a.num_reads_to_use, a.list_size, a.num_trials, trial, out)


if __name__ == "__main__":
    main()
