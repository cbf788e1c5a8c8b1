"""Timing of DESIGN.md row S on the GPU: the score kernel of the read simulator (sim_scores) at the m=11 r=5/6 msg_len=180
shape, 4096 reads -- HIP events around the kernel on the decoder's stream (lva_profile.total_ms after lva_simulate_fill_device),
160 bytes written per block -- and beside it the wall time of the host generator (synth.make_read_scores) for 64 such reads.
Two figures side by side: no ratio is asserted and nothing selects a path by them.  Writes profiles/simulate.json and prints it.

    python scripts/simulate_bench.py [--reads 4096] [--warmup 3] [--repeats 20] [--out profiles/simulate.json]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nanopore_dna_storage_amd as pkg                     # noqa: E402
from nanopore_dna_storage_amd import _lib, synth           # noqa: E402

M, R, MSG = 11, 5, 180
CHANNEL = dict(sub=0.002, dele=0.0085, ins=0.0005)          # simulator.py's defaults


def spread(xs):
    xs = sorted(xs)
    return dict(median=xs[len(xs) // 2], min=xs[0], max=xs[-1], n=len(xs))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "simulate.json"))
    a = ap.parse_args(argv)
    res = dict(build=_lib.build_id(), what="lva_simulate_fill_device, HIP events around sim_scores; wall time of the whole simulate call",
               shape=dict(mem_conv=M, rate=R, msg_len=MSG, reads=a.reads, **CHANNEL))
    with pkg.Decoder(M, R, MSG, list_size=8, max_deviation=20, max_slots=1) as dec:
        ms, wall, blocks = [], [], 0
        for k in range(a.warmup + a.repeats):
            t0 = time.perf_counter()
            with dec.simulate(a.reads, seed=1000 + k, **CHANNEL) as (_, off, _truth):
                dt = time.perf_counter() - t0
                p = dec.profile()
                blocks = int(off[-1])
                assert p["read_steps"] == blocks
            if k >= a.warmup:
                ms.append(p["total_ms"])
                wall.append(dt)
    s = spread(ms)
    res["sim_scores"] = dict(blocks=blocks, kernel_ms=s, bytes_written=blocks * 160, bytes_written_per_s=blocks * 160 / (s["median"] / 1e3),
                             reads_per_s=a.reads / (s["median"] / 1e3))
    w = spread(wall)
    res["simulate_call"] = dict(wall_s=w, reads_per_s=a.reads / w["median"],
                                note="plan + fill + truth to the host, two passes of sim_strand and the allocation included")
    t0 = time.perf_counter()
    host = [synth.make_read_scores(M, R, MSG, 1000 + i, **CHANNEL) for i in range(64)]
    dt = time.perf_counter() - t0
    res["host_generator"] = dict(what="synth.make_read_scores, wall time", reads=64, blocks=int(sum(len(x["scores"]) for x in host)),
                                 wall_s=dt, reads_per_s=64 / dt)
    text = json.dumps(res, indent=1)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
