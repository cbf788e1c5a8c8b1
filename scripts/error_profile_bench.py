"""Timing of DESIGN.md row N5: the error profile of 2 000 reads of the benchmark oligo (m = 11, rate 5/6, msg_len 180), the
definition error_profile.reference_profile (numpy, a read at a time) against one error_profile.align_profile call.  The reads
are 2 000 random messages' oligos through simulate.py's channel (host side, sub 0.02, dele 0.02, ins 0.01), every third one
reverse-complemented.  Host clock around whole calls, host arrays in and out; the device call is made once untimed first,
then --repeats times (median, min, max); the definition is timed once.  Both results are compared (they must be equal).
Writes profiles/error_profile.json and prints it.  No threshold: the file records what was measured.

    python scripts/error_profile_bench.py [--repeats 5] [--reads 2000] [--out profiles/error_profile.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nanopore_dna_storage_amd import _lib, error_profile as ep  # noqa: E402
from nanopore_dna_storage_amd.decoder import encode  # noqa: E402

CODE = (11, 5, 180)
SUB, DELE, INS = 0.02, 0.02, 0.01


def make(n, rng):
    msgs = rng.integers(0, 2, size=(n, CODE[2]), dtype=np.uint8)
    oligos = encode(*CODE, msgs)
    reads, rc = [], (np.arange(n) % 3 == 0).astype(np.uint8)
    for i in range(n):
        o = oligos[i]
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
    return np.concatenate(reads).astype(np.uint8), np.stack([off[:-1], np.diff(off)], axis=1), oligos, np.arange(n, dtype=np.int32), rc


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--reads", type=int, default=2000)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "error_profile.json"))
    a = ap.parse_args(argv)
    bases, win, oligos, ref_id, rc = make(a.reads, np.random.default_rng(1))
    cells = int((win[:, 1] * oligos.shape[1]).sum())
    got = ep.align_profile(bases, win, oligos, ref_id, rc)                # (not timed: the first call of a process)
    secs = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        ep.align_profile(bases, win, oligos, ref_id, rc)
        secs.append(time.perf_counter() - t0)
    secs.sort()
    t0 = time.perf_counter()
    want = ep.reference_profile(bases, win, oligos, ref_id, rc)
    ref_s = time.perf_counter() - t0
    res = dict(library=dict(version=_lib.load_library().lva_version().decode(), build_id=_lib.build_id()),
               what="error profile, host arrays in and out, host clock around whole calls, seconds",
               shape=dict(reads=a.reads, code=list(CODE), oligo_len=int(oligos.shape[1]), bases=int(len(bases)), cells=cells,
                          sub=SUB, dele=DELE, ins=INS),
               equal=bool(got == want), rates=got.rates(),
               reference_profile_s=ref_s, reference_profile_cells_per_s=cells / ref_s,
               align_profile_s=dict(median=secs[len(secs) // 2], min=secs[0], max=secs[-1], n=len(secs)),
               align_profile_cells_per_s=cells / secs[len(secs) // 2])
    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)
    return 0 if res["equal"] else 1


if __name__ == "__main__":
    sys.exit(main())
