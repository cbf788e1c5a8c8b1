"""Timing of the traceback of DESIGN.md row N7: where the truth's best path runs on its read -- 2 000 simulated reads of the
benchmark code (m = 11, rate 5/6, msg_len 180, max_deviation 20; the reads of scripts/trellis_score_bench.py) x their true
message, under the decoder's band and with the band off.  One Decoder.trace_bases_resident call beside one
Decoder.score_bases_resident call on the same pairs of the same resident buffer: the score kernel is the yardstick, not the
code under test.  A trace does the score's forward pass, writes and reads blocks x W back-pointer bytes once and walks the
path serially.  Host clock around whole calls; each call is made once untimed first, then --repeats times (median, min,
max).  The definition trellis_score.reference_trace is timed on the first --ref_pairs pairs and compared with the device
there, byte for byte.  Reported too: the back-pointer bytes of the call and the chunks they go in.  Writes
profiles/trellis_trace.json and prints it.  No threshold: the file records what was measured.

    python scripts/trellis_trace_bench.py [--repeats 5] [--reads 2000] [--ref_pairs 6] [--out profiles/trellis_trace.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nanopore_dna_storage_amd import Decoder, _lib, code_info, simulator, trellis_score as ts  # noqa: E402

CODE, L, MD = (11, 5, 180), 8, 20
LIMIT = 1 << 30                                              # the default scratch_limit of lva_trace_bases*


def timed(fn, repeats):
    fn()                                                                   # (not timed: the first call)
    secs = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        secs.append(time.perf_counter() - t0)
    secs.sort()
    return out, dict(median=secs[len(secs) // 2], min=secs[0], max=secs[-1], n=len(secs))


def scratch(blocks, n_bases, md):
    """(bytes of back-pointers of the call, chunks) as the host stage cuts them"""
    need = [(int(b) * min(2 * md, n_bases + 1) + 15) // 16 * 16 for b in blocks]
    chunks, used = 1, 0
    for n in need:
        if used + n > LIMIT:
            chunks, used = chunks + 1, 0
        used += n
    return int(sum(need)), chunks


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--reads", type=int, default=2000)
    ap.add_argument("--ref_pairs", type=int, default=6)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "trellis_trace.json"))
    a = ap.parse_args(argv)
    d = simulator.build_parser().parse_args([])
    npos = code_info(*CODE).nstate_pos
    off_band = CODE[2] + CODE[0] + 1
    res = dict(library=dict(version=_lib.load_library().lva_version().decode(), build_id=_lib.build_id()),
               what="trace of the truth of every read beside its score, resident posteriors, host clock around whole calls, seconds")
    ok = True
    with Decoder(*CODE, list_size=L, max_deviation=MD) as dec:
        with dec.simulate(a.reads, a.seed, sub=d.syn_sub_prob, dele=d.syn_del_prob, ins=d.syn_ins_prob) as (dev, off, truth):
            dec.posteriors_resident(dev, off)
            first, count = off[:-1], np.diff(off)
            keep = [i for i in range(a.reads) if count[i] >= npos + 1]
            seqs = list(ts.message_bases(*CODE, truth["msgs"]))
            pairs = [(i, i) for i in keep]
            blocks = int(sum(count[i] for i in keep))
            posts = dec.download(dev, off)
            res["shape"] = dict(reads=a.reads, code=list(CODE), pairs=len(pairs), pair_blocks=blocks, positions=int(npos), seed=a.seed)
            for name, md in (("banded", MD), ("unbanded", off_band)):
                sc, sc_s = timed(lambda: dec.score_bases_resident(dev, first, count, seqs, pairs, max_deviation=md), a.repeats)
                tr, tr_s = timed(lambda: dec.trace_bases_resident(dev, first, count, seqs, pairs, max_deviation=md), a.repeats)
                k = min(a.ref_pairs, len(pairs))
                t0 = time.perf_counter()
                want = [ts.reference_trace(posts[r], seqs[s], md) for r, s in pairs[:k]]
                ref_s = time.perf_counter() - t0
                same = all(np.array_equal(tr["enter"][j, :len(w["enter"])], w["enter"]) and np.array_equal(tr["kind"][j, :len(w["kind"])], w["kind"])
                           and int(tr["start_state"][j]) == w["start_state"] and int(tr["end_state"][j]) == w["end_state"]
                           and int(tr["n_stale"][j]) == w["n_stale"] for j, w in enumerate(want))
                nbytes, chunks = scratch([count[i] for i in keep], npos - 1, md)
                res[name] = dict(max_deviation=md, score_bases_resident_s=sc_s, trace_bases_resident_s=tr_s,
                                 trace_over_score=tr_s["median"] / sc_s["median"],
                                 trace_pair_blocks_per_s=blocks / tr_s["median"], scratch_bytes=nbytes, chunks=chunks,
                                 paths=int((tr["end_state"] >= 0).sum()), pairs_with_stale_hops=int((tr["n_stale"] > 0).sum()),
                                 scores_equal_score_bases=bool(tr["score"].tobytes() == sc.tobytes()),
                                 equal_to_definition=bool(same), definition_pairs=k, reference_trace_s=ref_s,
                                 reference_trace_pair_blocks_per_s=int(sum(count[r] for r, _ in pairs[:k])) / ref_s if k else 0.0)
                ok = ok and same and res[name]["scores_equal_score_bases"]
    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
