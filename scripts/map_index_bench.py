"""Timing of the read-mapping index: for 3 000 and 39 000 random 115-base oligos at k = 10 and k = 12, in one
process on one box,
  1. read_map.MapIndex(...) built on the host (lva_map_index_create: one core sorts the pairs and walks 4^k entries) against
     MapIndex(..., device=0) (lva_map_index_create_device, csrc/mi_kernels.hip: upload, build, wait);
  2. one read_map.map_reads call of 2 000 reads with each kind of index: the host-built one is uploaded by the call (the
     parent commit's only path), the device-built one is resident.
The reads are random pool members through the numpy channel of scripts/read_map_bench.py (deletion 0.02, substitution 0.02, a
geometric run of at most 4 inserted bases with 0.01), every third one reverse-complemented.  Host clock around whole calls,
each of which ends waited for; the two kinds alternate; every call is made once untimed first, then --repeats times (median,
min, max).  The calls of each kind are also timed back to back (two runs of --repeats calls per kind, the first call of a run
excluded), as the chunks of a manifest make them: on the GPU box a call's time turned out to depend on the kind of the call
before it (the two series differ by a factor of two and more; the cause was not looked for).  The tables and the mapping
results of the two kinds are compared (they must be equal).  Writes profiles/map_index.json and prints it.  No threshold: the file records what was measured.

    python scripts/map_index_bench.py [--repeats 5] [--reads 2000] [--pools 3000 39000] [--ks 10 12] [--out profiles/map_index.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nanopore_dna_storage_amd import _lib, read_map as rm  # noqa: E402

OLIGO_LEN = 115
SUB, DELE, INS = 0.02, 0.02, 0.01


def make_reads(oligos, n, rng):
    source = rng.integers(0, len(oligos), n)
    reads = []
    for i in range(n):
        o = oligos[source[i]]
        m = len(o)
        own = np.where(rng.random(m) < SUB, (o + rng.integers(1, 4, m)) & 3, o)
        n_ins = np.minimum(rng.geometric(1 - INS, m) - 1, 4)
        keep = rng.random(m) >= DELE
        r = np.concatenate([np.concatenate([rng.integers(0, 4, n_ins[p]), own[p:p + 1][keep[p:p + 1]]]) for p in range(m)]).astype(np.uint8)
        reads.append((3 - r)[::-1] if i % 3 == 0 else r)
    off = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.int64)
    return np.concatenate(reads).astype(np.uint8), np.stack([off[:-1], np.diff(off)], axis=1)


def spread(secs):
    secs = sorted(secs)
    return dict(median=secs[len(secs) // 2], min=secs[0], max=secs[-1], n=len(secs))


def clock(call):
    t0 = time.perf_counter()
    call()
    return time.perf_counter() - t0


def measure(pool, k, n_reads, repeats, max_occ=64):
    rng = np.random.default_rng(pool + k)
    oligos = rng.integers(0, 4, (pool, OLIGO_LEN)).astype(np.uint8)
    bases, win = make_reads(oligos, n_reads, rng)
    build = lambda device: rm.MapIndex(oligos, k, max_occ, device=device).close()
    build(None), build(0)                                            # (not timed: the first calls)
    build_s = dict(host=[], device=[])
    for _ in range(repeats):
        build_s["host"].append(clock(lambda: build(None)))
        build_s["device"].append(clock(lambda: build(0)))
    with rm.MapIndex(oligos, k, max_occ) as host, rm.MapIndex(oligos, k, max_occ, device=0) as dev:
        equal_tables = all(np.array_equal(a, b) for a, b in zip(host.tables(), dev.tables())) and host.info() == dev.info()
        want, got = rm.map_reads(bases, win, host), rm.map_reads(bases, win, dev)      # (not timed)
        map_s = dict(host=[], device=[])
        for _ in range(repeats):
            map_s["host"].append(clock(lambda: rm.map_reads(bases, win, host)))
            map_s["device"].append(clock(lambda: rm.map_reads(bases, win, dev)))
        # each kind also back to back, as a run of chunks makes the calls
        run_s = dict(host=[], device=[])
        for kind, index in (("host", host), ("device", dev), ("host", host), ("device", dev)):
            rm.map_reads(bases, win, index)                          # (not timed: the first call after the other kind)
            run_s[kind] += [clock(lambda: rm.map_reads(bases, win, index)) for _ in range(repeats)]
        info = host.info()
    return dict(oligos=pool, k=k, max_occ=max_occ, reads=n_reads, bases=int(len(bases)),
                index=dict(kmers=info[0], pairs=info[1], dropped_kmers=info[2], table_bytes=4 * (4 ** k + 1), list_bytes=4 * info[1],
                           mask_bytes=pool * 8 * 8 * ((OLIGO_LEN + 63) // 64)),
                equal_tables=bool(equal_tables), equal_results=bool(np.array_equal(want.out, got.out)), mapped=got.mapped,
                build_s=dict(host=spread(build_s["host"]), device=spread(build_s["device"])),
                map_reads_s=dict(host_index=spread(map_s["host"]), device_index=spread(map_s["device"])),
                map_reads_back_to_back_s=dict(host_index=spread(run_s["host"]), device_index=spread(run_s["device"])))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--reads", type=int, default=2000)
    ap.add_argument("--pools", type=int, nargs="+", default=[3000, 39000])
    ap.add_argument("--ks", type=int, nargs="+", default=[10, 12])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_index.json"))
    a = ap.parse_args(argv)
    rows = [measure(pool, k, a.reads, a.repeats) for pool in a.pools for k in a.ks]
    res = dict(library=dict(version=_lib.load_library().lva_version().decode(), build_id=_lib.build_id()),
               what="the read-mapping index built on the host against built on the device, and one map_reads call with each kind (host "
                    "index: uploaded by the call, the parent commit's path; device index: resident); host clock around whole calls, "
                    "seconds, the first call of each kind excluded; build_s and map_reads_s: the kinds alternating; "
                    "map_reads_back_to_back_s: two runs of consecutive calls per kind, the first call of a run excluded",
               oligo_len=OLIGO_LEN, sub=SUB, dele=DELE, ins=INS, rows=rows)
    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)
    return 0 if all(r["equal_tables"] and r["equal_results"] for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
