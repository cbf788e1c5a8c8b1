"""From a data file to a recovered file, or to a reading-cost curve, in one process and without intermediate files:

    file -> RS -> index / CRC (helper.encode)
         -> on the device: pick an oligo per read -> encode -> channel -> scores -> posteriors -> lists (Decoder.simulate_and_decode
            with the encoded file's bit strings as the pool: simulate.py, stream 6) -> CRC / index filter (list_ops.filter_lists)
         -> consensus + RS -> file, or with --num_reads_to_use the trials of decode_RS_from_decoded_lists --trials device
            (trials.run_trials) over the filtered reads, printed as that tool prints them.

Reads are made and decoded --chunk at a time, so that the scores in HBM stay bounded; read number k depends on (--seed, k)
alone, so nothing that is written or printed depends on --chunk.  --error_profile PREFIX: the reads as the channel emitted
them are aligned to the oligos they were drawn from (error_profile.align_profile; the reference of a read is the truth's
source, its orientation the truth's rc) and PREFIX.error_stats.csv is written: what the channel did, measured.  --coverage_weights FILE: one non-negative weight per oligo
(whitespace-separated, in the oligo file's order), uneven coverage; without it every oligo is as likely as any other.  Every
read's orientation is a coin (rc_mode 3) and is handed to the decoder as drawn."""
import argparse
import io
import math
import os
import sys
import tempfile

import numpy as np

from . import error_profile, helper, list_ops, rs_code, simulate
from .decode_RS_from_decoded_lists import print_curve, sample_sizes
from .decoder import Decoder, encode


def build_parser():
    p = argparse.ArgumentParser(description="data file -> simulated reads on the GPU -> recovered file or reading-cost curve")
    p.add_argument("--data_file", type=str, required=True)
    p.add_argument("--bytes_per_oligo", type=int, default=18)
    p.add_argument("--RS_redundancy", type=float, default=0.3)
    p.add_argument("--mem_conv", type=int, default=8)
    p.add_argument("--rate_conv", type=int, default=3)
    p.add_argument("--list_size", type=int, default=8)
    p.add_argument("--num_reads", type=int, required=True)
    p.add_argument("--seed", type=int, required=True, help="the Philox seed of the reads, and of the trial order")
    p.add_argument("--chunk", type=int, default=4096, help="reads made and decoded per pass; the output does not depend on it")
    p.add_argument("--sub", type=float, default=0.005)
    p.add_argument("--dele", type=float, default=0.005)
    p.add_argument("--ins", type=float, default=0.0005)
    p.add_argument("--margin", type=float, default=6.0)
    p.add_argument("--coverage_weights", type=str, default=None, help="file of one non-negative weight per oligo")
    p.add_argument("--num_reads_to_use", type=sample_sizes, default=None,
                   help="a sample size or an ascending comma-separated list: print the reading-cost curve instead of recovering the file")
    p.add_argument("--num_trials", type=int, default=10)
    p.add_argument("--out", type=str, default=None, help="the recovered file (default: DATA_FILE.recovered), or the file the curve is written to")
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--error_profile", type=str, default=None, metavar="PREFIX",
                   help="also align the simulated reads to their oligos and write PREFIX.error_stats.csv")
    return p


def filtered_reads(a, pool, pool_cdf, num_oligos, decoder=None, profiles=None):
    """reads 0 .. num_reads - 1 of the pool, made, decoded and filtered --chunk at a time
    -> (index int32 [num_reads] with -1 where no entry passed, payload uint8 [num_reads, bytes_per_oligo]);
    profiles: a list that receives every chunk's ErrorProfile against the truth (--error_profile)"""
    msg_len = pool.shape[1]
    oligos = encode(a.mem_conv, a.rate_conv, msg_len, pool) if profiles is not None else None
    own = decoder is None
    dec = Decoder(a.mem_conv, a.rate_conv, msg_len, list_size=a.list_size, max_deviation=20, device=a.device) if own else decoder
    index, payload = [np.zeros(0, np.int32)], [np.zeros((0, a.bytes_per_oligo), np.uint8)]
    try:
        for first in range(0, a.num_reads, a.chunk):
            truth, results = dec.simulate_and_decode(min(a.chunk, a.num_reads - first), a.seed, first_read=first, pool=pool,
                                                 pool_cdf=pool_cdf, rc_mode=3, sub=a.sub, dele=a.dele, ins=a.ins, margin=a.margin)
            msgs, counts = list_ops.results_to_array(results, dec.list_size, msg_len)
            k, _, p = list_ops.filter_lists(msgs, counts, a.bytes_per_oligo, num_oligos, device=a.device)
            index.append(k)
            payload.append(p)
            if profiles is not None:
                base = truth["base_offsets"]
                profiles.append(error_profile.align_profile(truth["bases"], np.stack([base[:-1], np.diff(base)], axis=1), oligos,
                                                            truth["source"], rc=truth["rc"], device=a.device))
    finally:
        if own:
            dec.close()
    return np.concatenate(index), np.concatenate(payload, axis=0)


def main(argv=None, out=sys.stdout, decoder=None):
    """-> dict(index, payload: the filtered reads; stats int32 [sizes, trials, 4] and table (the printed text), or data: the
    recovered bytes)"""
    parser = build_parser()
    a = parser.parse_args(argv)
    if a.chunk < 1 or a.num_reads < 1:
        parser.error("--chunk and --num_reads: at least 1")
    with open(a.data_file, "rb") as f:
        original = f.read()
    padded = math.ceil(len(original) / a.bytes_per_oligo) * a.bytes_per_oligo
    msg_len, num_oligos_data, num_oligos_RS, num_oligos = helper.compute_parameters(a.bytes_per_oligo, a.RS_redundancy, padded, False)
    with tempfile.TemporaryDirectory() as tmp:            # helper.encode's two files, read back as the pool
        oligo_file = os.path.join(tmp, "oligos")
        helper.encode(a.data_file, oligo_file, a.bytes_per_oligo, a.RS_redundancy, a.mem_conv, a.rate_conv, device=a.device, out=io.StringIO())
        pool = helper.read_conv_input(oligo_file + ".conv_input")
    pool_cdf = None
    if a.coverage_weights is not None:
        weights = np.loadtxt(a.coverage_weights, dtype=np.float64).reshape(-1)
        if len(weights) != len(pool):
            parser.error("--coverage_weights: %d weights for %d oligos" % (len(weights), len(pool)))
        pool_cdf = simulate.weights_to_cdf(weights)
    profiles = [] if a.error_profile is not None else None
    index, payload = filtered_reads(a, pool, pool_cdf, num_oligos, decoder, profiles)
    res = dict(index=index, payload=payload)
    if profiles is not None:
        profile = profiles[0]
        for part in profiles[1:]:
            profile = profile + part
        profile.write_csv(a.error_profile)
        res.update(error_profile=profile)
    if a.num_reads_to_use is not None:
        from . import trials
        stats = trials.run_trials(index, payload, original, a.bytes_per_oligo, num_oligos_RS, num_oligos, a.num_reads_to_use,
                                  a.num_trials, a.seed, device=a.device)
        table = io.StringIO()
        print_curve(a.num_reads_to_use, a.list_size, a.num_trials, lambda k, t: bool(stats[k, t, 3]), table)
        if a.out is None:
            out.write(table.getvalue())
        else:
            with open(a.out, "w") as f:
                f.write(table.getvalue())
        res.update(stats=stats, table=table.getvalue())
        return res
    print("num_attempted:", a.num_reads, file=out)
    print("num success:", int((index >= 0).sum()), file=out)
    decoded = list_ops.consensus(index, payload, num_oligos, device=a.device)
    print("num_unique", len(decoded), file=out)
    if num_oligos_RS:
        segments = rs_code.MainDecoder(decoded, num_oligos_RS, num_oligos, device=a.device)
    else:
        have = dict((k, v) for k, v in decoded)
        segments = [have.get(i, b"0" * a.bytes_per_oligo) for i in range(num_oligos_data)]
    data = b"".join(segments)[:len(original)]
    with open(a.out or a.data_file + ".recovered", "wb") as f:
        f.write(data)
    print("recovered" if data == original else "not recovered", file=out)
    res.update(data=data)
    return res


if __name__ == "__main__":
    main()
