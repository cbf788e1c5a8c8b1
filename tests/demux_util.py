"""Shared by the demultiplexing tests: seeded experiment tables and a restatement of the selection rule that is independent of
helper.demux_barcodes (a sort instead of its two minima)."""
import numpy as np

INF = float("inf")
FIELDS = ("ok", "start_pos", "end_pos", "rc", "dist_start", "dist_end")


def random_experiments(seed, k, length=25, mem_conv=6, rate_conv=1, msg_len=60, list_size=4):
    """k experiments with barcodes drawn from the seed (the reference's table is not copied)"""
    rng = np.random.default_rng([seed, k, length])
    word = lambda: "".join("ACGT"[int(x)] for x in rng.integers(0, 4, length))
    return [dict(name="exp%02d" % e, start_barcode=word(), end_barcode=word(), mem_conv=mem_conv, rate_conv=rate_conv,
                 msg_len=msg_len, list_size=list_size) for e in range(k)]


def select(cands, max_dist=None, min_margin=0):
    """the selection rule of the issue on a list of per-experiment candidates (locate_payload dicts)"""
    loc = sorted((c["dist_start"] + c["dist_end"], e) for e, c in enumerate(cands) if c["start_pos"] != -1)
    if not loc:
        return dict(ok=False, start_pos=-1, end_pos=-1, rc=False, dist_start=INF, dist_end=INF, experiment=-1, reason=1,
                    runner_up=-1, runner_up_dist=INF)
    (t, w), (t2, ru) = loc[0], (loc[1] if len(loc) > 1 else (INF, -1))
    reason = 2 if (max_dist is not None and t > max_dist) else 3 if t2 - t < min_margin else 4 if not cands[w]["ok"] else 0
    return dict({f: cands[w][f] for f in FIELDS}, ok=reason == 0, experiment=w, reason=reason, runner_up=ru, runner_up_dist=t2)


def rand_bases(rng, n):
    return "".join("ACGT"[int(x)] for x in rng.integers(0, 4, n))


def trans_for(rng, n):
    """a made-up list of transition positions: increasing, a few blocks per base"""
    return np.cumsum(rng.integers(1, 6, max(n, 1))) + 1
