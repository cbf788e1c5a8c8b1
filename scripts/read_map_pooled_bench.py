"""Timing of a pooled run: 3 groups x 1 000 random oligos of 113 / 115 / 117 bases, 2 000 reads of random
members through the channel of read_map_bench.py (deletion 0.02, substitution 0.02, insertion runs 0.01), every third one
reverse-complemented, k 10, cands 4.  Two ways to map them, on the same bytes:

  pooled    one read_map.map_reads call on one index of all 3 000 oligos (lva_map_reads_pooled), with the supplementary
            pass off (min_flank 0) and on (min_flank 56, half the shortest oligo);
  per group what had to be done before the index took oligos of unequal length: one map_reads call per group on that
            group's index (lva_map_reads), every read against every group, and a merge on the host that keeps per read the
            group with the smallest distance.

Host clock around whole calls, host arrays in and out, the indexes built before; every way is run once untimed, then
--repeats times (median, min, max).  Writes profiles/read_map_pooled.json and prints it.  No threshold: the file records
what was measured, and whether the two ways name the same oligo.

    python scripts/read_map_pooled_bench.py [--repeats 5] [--reads 2000] [--per_group 1000] [--out profiles/read_map_pooled.json]
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

LENS = (113, 115, 117)
SUB, DELE, INS = 0.02, 0.02, 0.01


def make(n, per_group, rng):
    oligos = [rng.integers(0, 4, m).astype(np.uint8) for m in LENS for _ in range(per_group)]
    source, rc = rng.integers(0, len(oligos), n).astype(np.int32), (np.arange(n) % 3 == 0).astype(np.int32)
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


def timed(fn, repeats):
    got = fn()                                                           # (not timed: the first call of its kind)
    secs = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        secs.append(time.perf_counter() - t0)
    secs.sort()
    return got, dict(median=secs[len(secs) // 2], min=secs[0], max=secs[-1], n=len(secs))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--reads", type=int, default=2000)
    ap.add_argument("--per_group", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "read_map_pooled.json"))
    a = ap.parse_args(argv)
    bases, win, oligos, source, rc = make(a.reads, a.per_group, np.random.default_rng(1))
    groups = np.repeat(np.arange(len(LENS), dtype=np.int32), a.per_group)
    min_flank = min(LENS) // 2
    with rm.MapIndex(oligos, groups=groups) as index:
        off, off_s = timed(lambda: rm.map_reads(bases, win, index), a.repeats)
        on, on_s = timed(lambda: rm.map_reads(bases, win, index, min_flank=min_flank), a.repeats)
    singles = [rm.MapIndex(np.stack(oligos[g * a.per_group:(g + 1) * a.per_group])) for g in range(len(LENS))]

    def per_group():
        outs = np.stack([rm.map_reads(bases, win, x).out for x in singles])              # [group, read, 8]
        dist = np.where(outs[:, :, 1] >= 0, outs[:, :, 3], 2 ** 30)
        g = dist.argmin(axis=0)                                                           # the smallest distance, the first group on a tie
        row = outs[g, np.arange(outs.shape[1])]
        return np.where(row[:, 0] >= 0, row[:, 0] + g * a.per_group, -1), row[:, 2]

    (m_ref, m_rc), group_s = timed(per_group, a.repeats)
    for x in singles:
        x.close()
    res = dict(library=dict(version=_lib.load_library().lva_version().decode(), build_id=_lib.build_id()),
               what="a pooled run mapped, host arrays in and out (every call uploads its index), host clock around whole calls, seconds",
               shape=dict(reads=a.reads, groups=len(LENS), oligos_per_group=a.per_group, oligo_lens=list(LENS), bases=int(len(bases)), k=10,
                          max_occ=64, cands=4, min_votes=2, min_flank=min_flank, sub=SUB, dele=DELE, ins=INS),
               pooled_call_s=off_s, pooled_call_with_supplementary_pass_s=on_s, one_call_per_group_and_host_merge_s=group_s,
               per_group_over_pooled=group_s["median"] / off_s["median"],
               recovered=dict(pooled=int(((off.ref == source) & (off.rc == rc)).sum()),
                              per_group=int(((m_ref == source) & (m_rc == rc)).sum())),
               same_oligo_both_ways=int((off.ref == m_ref).sum()), chimeric=int(on.chimeric.sum()),
               primary_rows_equal_with_and_without_the_pass=bool(np.array_equal(on.out, off.out)))
    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
