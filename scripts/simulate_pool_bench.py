"""Timing of the file-level experiment (pool source): helper.simulate_and_decode for one encoded file and one
read count, with posterior_source="crf" (a Python loop over reads makes the scores on the host: synth.mutate,
synth.scores_from_bases) and with posterior_source="device" (the reads are made on the GPU from the file's oligos as the pool).
Host clock around whole calls, the same decoder for both, list_ops="device" for both.  Two figures side by side: no ratio is
asserted and nothing selects a path by them.  Writes profiles/simulate_pool.json and prints it.

    python scripts/simulate_pool_bench.py [--bytes 10000] [--reads 2000] [--repeats 3] [--out profiles/simulate_pool.json]
"""
import argparse
import io
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nanopore_dna_storage_amd as pkg                     # noqa: E402
from nanopore_dna_storage_amd import _lib, helper          # noqa: E402

M, R, BYTES_PER_OLIGO, REDUNDANCY, LIST_SIZE = 8, 3, 18, 0.3, 8


def spread(xs):
    xs = sorted(xs)
    return dict(median=xs[len(xs) // 2], min=xs[0], max=xs[-1], n=len(xs))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=10000)
    ap.add_argument("--reads", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "simulate_pool.json"))
    a = ap.parse_args(argv)
    res = dict(build=_lib.build_id(), what="helper.simulate_and_decode, host clock around the whole call, one warm-up call first",
               shape=dict(mem_conv=M, rate=R, bytes_per_oligo=BYTES_PER_OLIGO, RS_redundancy=REDUNDANCY, list_size=LIST_SIZE,
                          file_bytes=a.bytes, reads=a.reads, sub=0.005, dele=0.005, ins=0.0005))
    with tempfile.TemporaryDirectory() as tmp:
        data_file, oligo_file = os.path.join(tmp, "data.bin"), os.path.join(tmp, "oligos")
        with open(data_file, "wb") as f:
            f.write(bytes(np.random.default_rng(1).integers(0, 256, size=a.bytes, dtype=np.uint8)))
        oligos = helper.encode(data_file, oligo_file, BYTES_PER_OLIGO, REDUNDANCY, M, R, out=io.StringIO())
        msg_len = helper.index_len + helper.crc_len + 8 * BYTES_PER_OLIGO
        res["shape"].update(num_oligos=len(oligos), msg_len=msg_len)
        with pkg.Decoder(M, R, msg_len, list_size=LIST_SIZE, max_deviation=20) as dec:
            for source in ("crf", "device"):
                wall, last = [], None
                for k in range(1 + a.repeats):
                    t0 = time.perf_counter()
                    last = helper.simulate_and_decode(oligo_file, os.path.join(tmp, "decoded.bin"), a.reads, a.bytes, BYTES_PER_OLIGO,
                                                      REDUNDANCY, M, R, list_size=LIST_SIZE, seed=7, out=io.StringIO(), decoder=dec,
                                                      posterior_source=source, list_ops="device")
                    if k:
                        wall.append(time.perf_counter() - t0)
                w = spread(wall)
                res[source] = dict(wall_s=w, reads_per_s=a.reads / w["median"], num_success=last["num_success"],
                                   num_unique=last["num_unique"])
    text = json.dumps(res, indent=1)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
