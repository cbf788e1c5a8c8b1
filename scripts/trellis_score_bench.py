"""Timing of DESIGN.md row N7: what every entry of every list scores on its read -- 2 000 simulated reads of the benchmark
code (m = 11, rate 5/6, msg_len 180, list size 8, max_deviation 20) x the entries of each read's list, one
Decoder.score_messages call (host posteriors in, host scores out: the upload is inside) against the definition
trellis_score.reference_score (numpy, a pair at a time).  The reads come from the device simulator with simulator.py's default
error rates and are decoded on the device; posteriors and lists are downloaded once, before anything is timed.  Host clock
around whole calls; the device call is made once untimed first, then --repeats times (median, min, max).  The definition
is timed on the first --ref_pairs pairs only (at its speed all of them would take most of an hour) and compared with the
device there, bit for bit; the rate is per pair-block (blocks of a pair's read, summed over the pairs).  Every list score
is checked to be one of the two values of its pair.  Also timed: score_bases_resident on a buffer that is already on the
device, the same pairs.  Writes profiles/trellis_score.json and prints it.  No threshold: the file records what was measured.

    python scripts/trellis_score_bench.py [--repeats 5] [--reads 2000] [--ref_pairs 24] [--out profiles/trellis_score.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nanopore_dna_storage_amd import Decoder, _lib, simulator, trellis_score as ts  # noqa: E402

CODE, L, MD = (11, 5, 180), 8, 20


def timed(fn, repeats):
    fn()                                                                   # (not timed: the first call)
    secs = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        secs.append(time.perf_counter() - t0)
    secs.sort()
    return out, dict(median=secs[len(secs) // 2], min=secs[0], max=secs[-1], n=len(secs))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--reads", type=int, default=2000)
    ap.add_argument("--ref_pairs", type=int, default=24)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "trellis_score.json"))
    a = ap.parse_args(argv)
    d = simulator.build_parser().parse_args([])
    with Decoder(*CODE, list_size=L, max_deviation=MD) as dec:
        with dec.simulate(a.reads, a.seed, sub=d.syn_sub_prob, dele=d.syn_del_prob, ins=d.syn_ins_prob) as (dev, off, truth):
            dec.posteriors_resident(dev, off)
            lists = dec.decode_resident(dev, off)
            posts = dec.download(dev, off)
            msgs, pairs, scores = [], [], []
            for r, g in enumerate(lists):
                if isinstance(g, int):
                    continue
                pairs += [(r, len(msgs) + i) for i in range(len(g[0]))]
                msgs += list(g[0])
                scores += list(g[1])
            msgs = np.array(msgs, np.uint8)
            blocks = int(sum(len(posts[r]) for r, _ in pairs))
            got, dev_s = timed(lambda: dec.score_messages(posts, msgs, pairs), a.repeats)
            seqs = list(ts.message_bases(*CODE, msgs))
            res_got, res_s = timed(lambda: dec.score_bases_resident(dev, off[:-1], np.diff(off), seqs, pairs), a.repeats)
    listed = all(np.float32(s).tobytes() in (g[0].tobytes(), g[1].tobytes()) for s, g in zip(scores, got))
    k = min(a.ref_pairs, len(pairs))
    t0 = time.perf_counter()
    want = np.array([ts.reference_score(posts[r], seqs[m], MD) for r, m in pairs[:k]], np.float32).reshape(k, 2)
    ref_s = time.perf_counter() - t0
    ref_blocks = int(sum(len(posts[r]) for r, _ in pairs[:k]))
    res = dict(library=dict(version=_lib.load_library().lva_version().decode(), build_id=_lib.build_id()),
               what="trellis score of every list entry, host clock around whole calls, seconds",
               shape=dict(reads=a.reads, code=list(CODE), list_size=L, max_deviation=MD, pairs=len(pairs), pair_blocks=blocks,
                          positions=int(len(seqs[0]) + 1) if seqs else 0, seed=a.seed),
               equal_to_definition=bool(want.tobytes() == got[:k].tobytes()), definition_pairs=k,
               resident_equals_host_call=bool(res_got.tobytes() == got.tobytes()),
               every_list_score_is_one_of_its_pair=bool(listed),
               reference_score_s=ref_s, reference_score_pair_blocks_per_s=ref_blocks / ref_s if k else 0.0,
               score_messages_s=dev_s, score_messages_pair_blocks_per_s=blocks / dev_s["median"],
               score_bases_resident_s=res_s, score_bases_resident_pair_blocks_per_s=blocks / res_s["median"])
    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)
    return 0 if res["equal_to_definition"] and res["resident_equals_host_call"] and listed else 1


if __name__ == "__main__":
    sys.exit(main())
