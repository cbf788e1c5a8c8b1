"""Timing of the forward score of DESIGN.md row N7: what all alignments of every list entry weigh on its read -- 2 000
simulated reads of the benchmark code (m = 11, rate 5/6, msg_len 180, list size 8, max_deviation 20; the reads of
scripts/trellis_score_bench.py) x the entries of their decoded lists.  One Decoder.forward_bases_resident call beside one
Decoder.score_bases_resident call on the same pairs of the same resident buffer: the score kernel is the yardstick, the same
trellis without the transcendentals (a flip cell: two expf and one logf more, a flop cell: one of each).  Host clock around
whole calls; each call is made once untimed first, then --repeats times (median, min, max).  The error of the device against
trellis_score.reference_forward in float64 is recorded on --ref_pairs of the pairs, beside the error of the definition's
float32 restatement there (the yardstick of tests/test_gpu_trellis_forward.py).  Writes profiles/trellis_forward.json and
prints it.  No threshold: the file records what was measured.

    python scripts/trellis_forward_bench.py [--repeats 5] [--reads 2000] [--ref_pairs 24] [--out profiles/trellis_forward.json]
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


def timed(fn, repeats):
    fn()                                                                   # (not timed: the first call)
    secs = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        secs.append(time.perf_counter() - t0)
    secs.sort()
    return out, dict(median=secs[len(secs) // 2], min=secs[0], max=secs[-1], n=len(secs))


def error(x, want):
    """max |x - want|; both -inf counts as 0, one of them as inf"""
    x, want = np.asarray(x, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    with np.errstate(invalid="ignore"):
        d = np.where(np.isneginf(x) & np.isneginf(want), 0.0, np.abs(x - want))
    d[np.isnan(d)] = np.inf
    return float(d.max()) if len(d) else 0.0


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--reads", type=int, default=2000)
    ap.add_argument("--ref_pairs", type=int, default=24)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "trellis_forward.json"))
    a = ap.parse_args(argv)
    d = simulator.build_parser().parse_args([])
    npos = code_info(*CODE).nstate_pos
    res = dict(library=dict(version=_lib.load_library().lva_version().decode(), build_id=_lib.build_id()),
               what="forward score of every list entry beside its score, resident posteriors, host clock around whole calls, seconds")
    with Decoder(*CODE, list_size=L, max_deviation=MD) as dec:
        with dec.simulate(a.reads, a.seed, sub=d.syn_sub_prob, dele=d.syn_del_prob, ins=d.syn_ins_prob) as (dev, off, truth):
            dec.posteriors_resident(dev, off)
            first, count = off[:-1], np.diff(off)
            lists = dec.decode_resident(dev, off)
            msgs, pairs = [], []
            for i, g in enumerate(lists):
                if not isinstance(g, int) and count[i] >= npos + 1:
                    pairs += [(i, len(msgs) + j) for j in range(len(g[0]))]
                    msgs += list(g[0])
            seqs = list(ts.message_bases(*CODE, np.array(msgs, np.uint8)))
            blocks = int(sum(count[r] for r, _ in pairs))
            res["shape"] = dict(reads=a.reads, code=list(CODE), list_size=L, max_deviation=MD, pairs=len(pairs), pair_blocks=blocks,
                                positions=int(npos), bases=len(seqs[0]), seed=a.seed)
            sc, sc_s = timed(lambda: dec.score_bases_resident(dev, first, count, seqs, pairs), a.repeats)
            fw, fw_s = timed(lambda: dec.forward_bases_resident(dev, first, count, seqs, pairs), a.repeats)
            posts = dec.download(dev, off)
    pick = np.linspace(0, len(pairs) - 1, min(a.ref_pairs, len(pairs))).astype(int).tolist() if pairs else []
    t0 = time.perf_counter()
    f64 = np.array([ts.reference_forward(posts[pairs[k][0]], seqs[pairs[k][1]], MD) for k in pick], np.float64).reshape(-1, 2)
    ref_s = time.perf_counter() - t0
    f32 = np.array([ts.reference_forward(posts[pairs[k][0]], seqs[pairs[k][1]], MD, dtype=np.float32) for k in pick], np.float32).reshape(-1, 2)
    tot_fw, tot_sc = ts.forward_total(fw), sc.max(axis=1).astype(np.float64)
    res["timing"] = dict(score_bases_resident_s=sc_s, forward_bases_resident_s=fw_s, forward_over_score=fw_s["median"] / sc_s["median"],
                         forward_pair_blocks_per_s=blocks / fw_s["median"], score_pair_blocks_per_s=blocks / sc_s["median"])
    res["error"] = dict(definition_pairs=len(pick), device_vs_float64=error(fw[pick], f64), float32_restatement_vs_float64=error(f32, f64),
                        largest_value=float(np.abs(f64[np.isfinite(f64)]).max()) if np.isfinite(f64).any() else 0.0,
                        reference_forward_s=ref_s)
    live = np.isfinite(tot_fw) & np.isfinite(tot_sc)
    res["lists"] = dict(pairs_with_a_path=int(live.sum()),
                        forward_minus_best_path_median=float(np.median(tot_fw[live] - tot_sc[live])) if live.any() else 0.0,
                        forward_minus_best_path_max=float((tot_fw[live] - tot_sc[live]).max()) if live.any() else 0.0)
    ok = res["error"]["device_vs_float64"] <= 2 * res["error"]["float32_restatement_vs_float64"]
    res["error"]["within_twice_the_restatement"] = bool(ok)
    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
