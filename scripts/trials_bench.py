"""Timing of DESIGN.md row N4': reading-cost trials, the per-trial host loop against one trials.run_trials call, on the
experiment-7 shape (10 000 read numbers, 733 indices of which 30 % are parity, 18 bytes per oligo), filter outputs
synthesised (85 % of the reads carry an index, 10 % of those a wrong payload), at
  * 1 sample size x 100 trials,
  * 10 sample sizes x 100 trials.
The per-trial loop is what decode_RS_from_decoded_lists --trials host does per trial from in-memory lists:
rs_code.decode_from_lists (filter, consensus, RS decode) with list_ops "host" and "device", the sample drawn by
random.sample.  Host clock around whole calls, median of 5 (the first call of each kind is not timed).  Writes
profiles/trials.json and prints it.  No threshold: the file records what was measured.

    python scripts/trials_bench.py [--repeats 5] [--trials 100] [--out profiles/trials.json]
"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nanopore_dna_storage_amd import _lib, helper, rs_code, trials  # noqa: E402

BPO, N_READS, N_DATA, RS_REDUNDANCY = 18, 10000, 564, 0.3


def spread(xs):
    xs = sorted(xs)
    return dict(median=xs[len(xs) // 2], min=xs[0], max=xs[-1], n=len(xs))


def timed(fn, repeats):
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return spread(ms)


def make(rng):
    fec = int(N_DATA * RS_REDUNDANCY)
    no = N_DATA + fec
    data = [bytes(rng.integers(0, 256, size=BPO, dtype=np.uint8)) for _ in range(N_DATA)]
    enc = rs_code.MainEncoder(data, fec)
    index = rng.integers(0, no, size=N_READS).astype(np.int32)
    payload = np.frombuffer(b"".join(enc), np.uint8).reshape(no, BPO)[index].copy()
    wrong = rng.random(N_READS) < 0.10
    payload[wrong] = rng.integers(0, 256, size=(int(wrong.sum()), BPO), dtype=np.uint8)
    none = rng.random(N_READS) < 0.15
    index[none] = -1
    payload[none] = 0
    # the lists the host loop reads: the passing entry behind one that fails its CRC; a read without an index has junk only
    junk = "1" * (helper.index_len + helper.crc_len + 8 * BPO)
    lists = [[junk] if index[i] < 0 else [junk, helper.attach_index_crc(int(index[i]), payload[i].tobytes())] for i in range(N_READS)]
    return dict(index=index, payload=payload, lists=lists, original=b"".join(data)[:-5], fec=fec, no=no)


def host_loop(d, points, n_trials, list_ops, seed=1):
    rnd = random.Random(seed)
    wins = []
    for u in points:
        ok = 0
        for _ in range(n_trials):
            lists = [d["lists"][i] for i in rnd.sample(range(N_READS), u)]
            data, passed = rs_code.decode_from_lists(lists, BPO, d["fec"], d["no"], list_ops=list_ops)
            ok += int(passed > 0 and data[:len(d["original"])] == d["original"])
        wins.append(ok)
    return wins


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--trials", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "trials.json"))
    a = ap.parse_args(argv)
    d = make(np.random.default_rng(1))
    res = dict(library=dict(version=_lib.load_library().lva_version().decode(), build_id=_lib.build_id()),
               what="reading-cost trials, host arrays in and out, host clock around whole calls, ms",
               shape=dict(read_numbers=N_READS, num_oligos=d["no"], redundancy=d["fec"], bytes_per_oligo=BPO, trials=a.trials))
    for name, points in (("1_point", [1700]), ("10_points", list(range(1100, 2100, 100)))):
        run = lambda: trials.run_trials(d["index"], d["payload"], d["original"], BPO, d["fec"], d["no"], points, a.trials, 1)
        stats = run()
        entry = dict(reads_to_use=points, trials_per_point=a.trials, device_successes=stats[:, :, 3].sum(axis=1).tolist())
        entry["run_trials_ms"] = timed(run, a.repeats)
        entry["run_trials_ms_per_trial"] = entry["run_trials_ms"]["median"] / (len(points) * a.trials)
        print(name, "run_trials", entry["run_trials_ms"], file=sys.stderr, flush=True)
        for list_ops in ("host", "device"):
            entry["host_loop_successes_list_ops_%s" % list_ops] = host_loop(d, points, a.trials, list_ops)
            ms = timed(lambda: host_loop(d, points, a.trials, list_ops), a.repeats)
            entry["host_loop_list_ops_%s" % list_ops] = dict(ms=ms, ms_per_trial=ms["median"] / (len(points) * a.trials))
            print(name, "host loop, list_ops", list_ops, ms, file=sys.stderr, flush=True)
        res[name] = entry
    text = json.dumps(res, indent=1)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
