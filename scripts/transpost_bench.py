"""Timing of DESIGN.md row N0 on the GPU: lva_transpost_batch_device (scores resident in HBM, posteriors in place) on
  * the benchmark's 512 reads (bench.py's pool: m=11 r=5/6 msg_len=180, seeds 1000.., every 5th read noisy, odd reads
    reverse-complemented) as score matrices, and
  * 4096 reads of 2000 blocks, scores uniform in the network's range,
and, in the same session, the reads/s of the fastest decoder shape (m=6 r=1/2 L=1 at default slots) on resident posteriors
of its own reads -- the posterior stage must stay above it.  Times are HIP events around the two kernels on the decoder's
stream (lva_profile.total_ms after the call).  Writes profiles/transpost.json and prints it.

    python scripts/transpost_bench.py [--warmup 3] [--repeats 20] [--out profiles/transpost.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nanopore_dna_storage_amd as pkg                     # noqa: E402
from nanopore_dna_storage_amd import _lib, synth           # noqa: E402

BYTES_PER_BLOCK = 544          # forward: 160 read + 32 written; backward: 160 + 32 read, 160 written


def spread(xs):
    xs = sorted(xs)
    return dict(median=xs[len(xs) // 2], min=xs[0], max=xs[-1], n=len(xs))


def time_transpost(dec, scores, warmup, repeats):
    dev, off = dec.upload(scores)
    blocks = int(off[-1])
    try:
        for _ in range(warmup):
            dec.posteriors_resident(dev, off)              # in place: the values change, the work does not
        ms = []
        for _ in range(repeats):
            dec.posteriors_resident(dev, off)
            p = dec.profile()
            assert p["read_steps"] == blocks
            ms.append(p["total_ms"])
    finally:
        dec.free(dev)
    s = spread(ms)
    sec = s["median"] / 1e3
    return dict(reads=len(scores), blocks=blocks, kernel_ms=s, reads_per_s=len(scores) / sec, blocks_per_s=blocks / sec,
                algorithmic_bytes_per_block=BYTES_PER_BLOCK, achieved_bytes_per_s=blocks * BYTES_PER_BLOCK / sec)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "transpost.json"))
    a = ap.parse_args(argv)
    res = dict(build=_lib.build_id(), what="lva_transpost_batch_device, in place, HIP events around tp_forward + tp_backward")
    pool = [synth.make_read_scores(11, 5, 180, 1000 + i, rc=bool(i & 1), margin=3.0 if i % 5 == 0 else 6.0)["scores"] for i in range(512)]
    rng = np.random.default_rng(1)
    base = [rng.uniform(-synth.SCORE_CLIP, synth.SCORE_CLIP, (2000, 40)).astype(np.float32) for _ in range(64)]
    with pkg.Decoder(11, 5, 180, list_size=8, max_deviation=20, max_slots=1) as dec:
        res["benchmark_512_reads"] = time_transpost(dec, pool, a.warmup, a.repeats)
        res["uniform_4096x2000"] = time_transpost(dec, [base[i % 64] for i in range(4096)], a.warmup, a.repeats)
    # the fastest decoder shape, same session: host clock around calls that end in a device synchronise
    reads = synth.make_reads(6, 1, 60, 512, seed0=1000, rc_mode="odd")
    posts, rc = [x["post"] for x in reads] * 8, [x["rc"] for x in reads] * 8
    with pkg.Decoder(6, 1, 60, list_size=1, max_deviation=20) as dec:
        dev, off = dec.upload(posts)
        try:
            for _ in range(a.warmup):
                dec.decode_resident(dev, off, rc)
            rates = []
            for _ in range(max(3, a.repeats // 4)):
                t0 = time.perf_counter()
                dec.decode_resident(dev, off, rc)
                rates.append(len(posts) / (time.perf_counter() - t0))
            slots = dec.profile()["slots"]
        finally:
            dec.free(dev)
    res["decoder_m6_r1_L1"] = dict(reads=len(posts), slots=slots, reads_per_s=spread(rates))
    res["posterior_stage_over_fastest_decoder"] = res["benchmark_512_reads"]["reads_per_s"] / res["decoder_m6_r1_L1"]["reads_per_s"]["median"]
    text = json.dumps(res, indent=1)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
