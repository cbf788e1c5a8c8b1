"""Timing of DESIGN.md row N2: the list consumers on the GPU (list_ops: lva_list_filter / lva_list_consensus /
lva_list_stats, host arrays in, host arrays out -- the upload is inside the call) against the host functions they
stand in for, on
  * 10 000 lists of 8 at msg_len 164 (18 bytes per oligo, 733 oligos): filter, then consensus of what passed,
  * 1 000 lists of 64 at msg_len 164, no entry passing (the host filter's worst case),
  * the statistics of 1 000 trials at msg_len 180 with lists of 4 (the host's Levenshtein is timed on 50 of them).
Host clock around whole calls.  Writes profiles/list_ops.json and prints it.  No threshold: the file records what was measured.

    python scripts/list_ops_bench.py [--warmup 2] [--repeats 10] [--out profiles/list_ops.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nanopore_dna_storage_amd import _lib, helper, list_ops, rs_code  # noqa: E402


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


def make_lists(rng, n, L, bpo, num_oligos, pass_rate):
    """lists of L entries: junk = a valid entry with one bit flipped; with probability pass_rate a valid one at a random rank"""
    bits = 20 + 8 * bpo
    pool = []
    for _ in range(512):
        e = helper.attach_index_crc(int(rng.integers(4096)), bytes(rng.integers(0, 256, size=bpo, dtype=np.uint8)))
        k = int(rng.integers(bits))
        pool.append(e[:k] + ("1" if e[k] == "0" else "0") + e[k + 1:])
    payloads = [bytes(rng.integers(0, 256, size=bpo, dtype=np.uint8)) for _ in range(num_oligos)]
    lists = []
    for _ in range(n):
        lst = [pool[j] for j in rng.integers(512, size=L)]
        if rng.random() < pass_rate:
            k = int(rng.integers(num_oligos))
            p = payloads[k] if rng.random() < 0.9 else bytes(rng.integers(0, 256, size=bpo, dtype=np.uint8))
            lst[int(rng.integers(L))] = helper.attach_index_crc(k, p)
        lists.append(lst)
    return lists


def bench_filter(rng, n, L, pass_rate, warmup, repeats):
    bpo, num_oligos = 18, 733
    lists = make_lists(rng, n, L, bpo, num_oligos, pass_rate)
    msgs, counts = list_ops.lists_to_array(lists)
    host = lambda: [helper.decode_list_CRC_index(lst, bpo, num_oligos, False) for lst in lists]
    want = host()
    index, rank, payload = list_ops.filter_lists(msgs, counts, bpo, num_oligos)
    assert [(-1 if w[0] is None else w[0]) for w in want] == index.tolist()
    res = dict(lists=n, list_size=L, msg_len=msgs.shape[2], passed=int((index >= 0).sum()), upload_bytes=int(msgs.nbytes),
               host_filter_ms=timed(host, 0, max(2, repeats // 3)),
               device_filter_ms=timed(lambda: list_ops.filter_lists(msgs, counts, bpo, num_oligos), warmup, repeats))
    if pass_rate:
        dec = [(w[0], w[1]) for w in want if w[0] is not None]
        assert dict(map(tuple, rs_code.consensus(dec))) == dict(map(tuple, list_ops.consensus(index, payload, num_oligos)))
        res["host_consensus_ms"] = timed(lambda: rs_code.consensus(dec), 0, max(2, repeats // 3))
        res["device_consensus_ms"] = timed(lambda: list_ops.consensus_arrays(index, payload, num_oligos), warmup, repeats)
    return res


def bench_stats(rng, n, msg_len, L, warmup, repeats, host_sample=50):
    truth = rng.integers(0, 2, size=(n, msg_len), dtype=np.uint8)
    msgs = rng.integers(0, 2, size=(n, L, msg_len), dtype=np.uint8)
    msgs[::2, 0] = truth[::2]                               # half of the trials decode correctly
    flip = rng.integers(msg_len, size=n)
    msgs[1::4, 0] = truth[1::4]
    msgs[np.arange(1, n, 4), 0, flip[1::4]] ^= 1            # a quarter with one substitution; the rest random
    counts = np.full(n, L, np.int32)
    lists = list_ops.array_to_lists(msgs, counts)
    tr = ["".join(map(str, row)) for row in truth]

    def host(k):
        for t, lst in zip(tr[:k], lists[:k]):
            _ = (lst[0] == t, t in lst, helper.hamming(t, lst[0]), helper.levenshtein(t, lst[0]))

    got = list_ops.list_stats(msgs, counts, truth)
    assert all(int(got["edit"][i]) == helper.levenshtein(tr[i], lists[i][0]) for i in range(8))
    per_trial = timed(lambda: host(host_sample), 0, 2)
    return dict(trials=n, list_size=L, msg_len=msg_len, host_sample=host_sample,
                host_ms_per_trial={k: (v / host_sample if k != "n" else v) for k, v in per_trial.items()},
                host_ms_extrapolated=per_trial["median"] / host_sample * n,
                device_stats_ms=timed(lambda: list_ops.list_stats(msgs, counts, truth), warmup, repeats))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "list_ops.json"))
    a = ap.parse_args(argv)
    rng = np.random.default_rng(1)
    res = dict(library=dict(version=_lib.load_library().lva_version().decode(), build_id=_lib.build_id()),
               what="list_ops calls, host arrays in and out (upload and download inside), host clock, ms")
    res["filter_10000x8"] = bench_filter(rng, 10000, 8, 0.6, a.warmup, a.repeats)
    res["filter_1000x64_none_passing"] = bench_filter(rng, 1000, 64, 0.0, a.warmup, a.repeats)
    res["stats_1000_trials_180"] = bench_stats(rng, 1000, 180, 4, a.warmup, a.repeats)
    text = json.dumps(res, indent=1)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
