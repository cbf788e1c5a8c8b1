"""Timing of DESIGN.md row N3': demultiplexing a pooled run on the device.  4 096 synthetic barcoded reads (512 distinct
ones, each 8 times; code m = 6 r = 1 msg_len 60, 25-base barcodes, 13 experiments drawn from a seed), posteriors resident:
  (a) one Decoder.demux_resident call: one basecall, one search over all 52 patterns, one decision per read,
  (b) thirteen Decoder.locate_payload_resident calls on the same buffer, one per experiment -- the only way before,
  (c) the basecall alone (lva_basecall_batch_device without the copies of bases and positions to the host).
Host clock around whole calls, each complete on return (allocation, launches, copy of the results, synchronisation).
Writes profiles/demux.json and prints it.  No threshold and no ratio: the file records what was measured.

    python scripts/demux_bench.py [--warmup 2] [--repeats 10] [--out profiles/demux.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nanopore_dna_storage_amd import Decoder, _lib, synth  # noqa: E402

N_READS, N_DISTINCT, N_EXPS, BARCODE = 4096, 512, 13, 25
CODE = (6, 1, 60)


def spread(xs):
    xs = sorted(xs)
    return dict(median=xs[len(xs) // 2], min=xs[0], max=xs[-1], n=len(xs))


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return spread(ms)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "demux.json"))
    a = ap.parse_args(argv)
    rng = np.random.default_rng(1313)
    exps = [dict(start_barcode=synth.random_barcode(rng, BARCODE), end_barcode=synth.random_barcode(rng, BARCODE),
                 mem_conv=CODE[0], rate_conv=CODE[1], msg_len=CODE[2]) for _ in range(N_EXPS)]
    reads, truth = synth.make_pooled_reads(exps, N_DISTINCT, seed0=13000)
    posts = [x["post"] for x in reads] * (N_READS // N_DISTINCT)
    truth = truth * (N_READS // N_DISTINCT)
    with Decoder(*CODE, list_size=1, device=a.device, max_slots=1) as dec:
        dev, off = dec.upload(posts)
        try:
            L, n = dec._L, len(posts)
            nb = np.zeros(n, np.int32)
            got = dec.demux_resident(dev, off, exps)
            each = [dec.locate_payload_resident(dev, off, x["start_barcode"], x["end_barcode"]) for x in exps]
            # the two ways agree on every read that is assigned: the winner's window is that experiment's locate_payload
            agree = sum(1 for i, g in enumerate(got)
                        if g["reason"] == 0 and {k: g[k] for k in each[0][0]} == each[g["experiment"]][i])
            res = dict(
                build=_lib.build_id(), reads=n, distinct_reads=N_DISTINCT, experiments=N_EXPS, barcode_len=BARCODE,
                blocks=int(off[-1]), bases=None, clock="host clock around whole calls, ms",
                assigned=sum(g["reason"] == 0 for g in got), assigned_to_truth=sum(g["experiment"] == t for g, t in zip(got, truth)),
                agree_with_locate_payload=agree,
                demux_resident=timed(lambda: dec.demux_resident(dev, off, exps), a.warmup, a.repeats),
                locate_payload_resident_x13=timed(lambda: [dec.locate_payload_resident(dev, off, x["start_barcode"], x["end_barcode"])
                                                           for x in exps], a.warmup, a.repeats),
                basecall_only=timed(lambda: dec._check(L.lva_basecall_batch_device(dec._h, dev, off.ctypes.data, n, None, None,
                                                                                   nb.ctypes.data)), a.warmup, a.repeats))
            res["bases"] = int(nb.sum())
        finally:
            dec.free(dev)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
