"""Timing of DESIGN.md row N6: 2 000 reads of the benchmark oligo set (m = 11, rate 5/6, msg_len 180: 115 bases) mapped to a
pool of 3 000 oligos with read_map's defaults, the definition read_map.reference_map (numpy, a read at a time) against one
read_map.map_reads call.  The reads are random pool members through a channel of this script's own in numpy (the one of
error_profile_bench.py, not simulate.py's: a base is deleted with 0.02, a kept base substituted with 0.02, a geometric run of at
most 4 inserted bases with 0.01 in front of every position), every third one reverse-complemented.  Host clock around whole calls, host arrays in and out; the device call is
made once untimed first, then --repeats times (median, min, max); the definition is timed once.  Both results are compared
(they must be equal).  The split between mp_vote and mp_verify comes from one `rocprofv3 --kernel-trace --stats` run of this
script (--calls-only: the untimed call and the repeats, nothing else).  The cell-equivalent rate (cands x ref_len x window per
read) stands beside align_profile's cells per second of profiles/error_profile.json.  Writes profiles/read_map.json and
prints it.  No threshold: the file records what was measured.

    python scripts/read_map_bench.py [--repeats 5] [--reads 2000] [--pool 3000] [--out profiles/read_map.json]
"""
import argparse
import csv
import glob
import json
import os
import shutil
import signal
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nanopore_dna_storage_amd import _lib, read_map as rm  # noqa: E402
from nanopore_dna_storage_amd.decoder import encode  # noqa: E402

CODE = (11, 5, 180)
SUB, DELE, INS = 0.02, 0.02, 0.01
TRACE_LIMIT_S = 150


def make(n, pool, rng):
    oligos = encode(*CODE, rng.integers(0, 2, size=(pool, CODE[2]), dtype=np.uint8))
    source, rc = rng.integers(0, pool, n).astype(np.int32), (np.arange(n) % 3 == 0).astype(np.int32)
    reads = []
    for i in range(n):
        o = oligos[source[i]]
        m = len(o)
        keep = rng.random(m) >= DELE
        own = np.where(rng.random(m) < SUB, (o + rng.integers(1, 4, m)) & 3, o)
        n_ins = np.minimum(rng.geometric(1 - INS, m + 1) - 1, 4)
        out = []
        for p in range(m + 1):
            out += list(rng.integers(0, 4, n_ins[p]))
            if p < m and keep[p]:
                out.append(own[p])
        r = np.array(out, np.uint8)
        reads.append((3 - r)[::-1] if rc[i] else r)
    off = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.int64)
    return np.concatenate(reads).astype(np.uint8), np.stack([off[:-1], np.diff(off)], axis=1), oligos, source, rc


def kernel_split(argv):
    """total nanoseconds per kernel of one traced run of this script's device calls, or why there is none"""
    tool = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(tool):
        return dict(not_measured="no rocprofv3")
    with tempfile.TemporaryDirectory() as d:
        # a session of its own, so that the time limit ends the profiler and the program under it
        run = subprocess.Popen([tool, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "read_map", "--", sys.executable,
                                os.path.abspath(__file__), "--calls-only"] + argv, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True,
                               start_new_session=True)
        try:                                                 # (the untraced calls take seconds: a traced run that takes minutes hangs)
            err = run.communicate(timeout=TRACE_LIMIT_S)[1]
        except subprocess.TimeoutExpired:
            os.killpg(run.pid, signal.SIGKILL)
            run.communicate()
            return dict(not_measured="the traced run did not end within %d s" % TRACE_LIMIT_S)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if run.returncode != 0 or not files:
            return dict(not_measured="rocprofv3 exit %d, %d stats files" % (run.returncode, len(files)), stderr=err[-400:])
        ns = {}
        with open(files[0]) as f:
            for row in csv.DictReader(f):
                for part in ("mp_vote", "mp_verify"):
                    if part in row["Name"]:
                        ns[part] = ns.get(part, 0) + int(float(row["TotalDurationNs"]))
                        ns[part + "_calls"] = ns.get(part + "_calls", 0) + int(float(row["Calls"]))
    total = ns.get("mp_vote", 0) + ns.get("mp_verify", 0)
    return dict(ns, what="rocprofv3 --kernel-trace --stats, total kernel nanoseconds over the traced calls; mp_verify counts both of its "
                         "passes", mp_vote_share=ns.get("mp_vote", 0) / total if total else None)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--reads", type=int, default=2000)
    ap.add_argument("--pool", type=int, default=3000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "read_map.json"))
    ap.add_argument("--calls-only", action="store_true", help="the device calls alone (what the traced run executes)")
    a = ap.parse_args(argv)
    bases, win, oligos, source, rc = make(a.reads, a.pool, np.random.default_rng(1))
    with rm.MapIndex(oligos) as index:
        got = rm.map_reads(bases, win, index)                            # (not timed: the first call of a process)
        secs = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            rm.map_reads(bases, win, index)
            secs.append(time.perf_counter() - t0)
        info = index.info()
    if a.calls_only:
        return 0
    secs.sort()
    t0 = time.perf_counter()
    want = rm.reference_map(bases, win, oligos)
    ref_s = time.perf_counter() - t0
    cells = int((4 * oligos.shape[1] * win[:, 1]).sum())                  # cands x ref_len x window per read
    parent = {}
    try:
        with open(os.path.join(ROOT, "profiles", "error_profile.json")) as f:
            e = json.load(f)
        parent = dict(build_id=e["library"]["build_id"], align_profile_cells_per_s=e["align_profile_cells_per_s"])
    except (OSError, KeyError, ValueError):
        pass
    res = dict(library=dict(version=_lib.load_library().lva_version().decode(), build_id=_lib.build_id()),
               what="read mapping, host arrays in and out (the index is uploaded by every call), host clock around whole calls, seconds",
               shape=dict(reads=a.reads, pool=a.pool, code=list(CODE), oligo_len=int(oligos.shape[1]), bases=int(len(bases)),
                          k=index.k, max_occ=index.max_occ, cands=4, min_votes=2, max_dist=int(oligos.shape[1]) // 4,
                          index=dict(kmers=info[0], pairs=info[1], dropped_kmers=info[2]), cell_equivalents=cells, sub=SUB, dele=DELE, ins=INS),
               equal=bool(np.array_equal(got.out, want.out)),
               recovered=int(((got.ref == source) & (got.rc == rc)).sum()), mapped=got.mapped,
               reference_map_s=ref_s,
               map_reads_s=dict(median=secs[len(secs) // 2], min=secs[0], max=secs[-1], n=len(secs)),
               map_reads_cell_equivalents_per_s=cells / secs[len(secs) // 2],
               align_profile_of_the_parent_commit=parent,
               kernels=kernel_split(["--repeats", str(a.repeats), "--reads", str(a.reads), "--pool", str(a.pool)]))
    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)
    return 0 if res["equal"] else 1


if __name__ == "__main__":
    sys.exit(main())
