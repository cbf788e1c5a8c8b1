"""What the one-message trellis tests share (tests/test_trellis_score_host.py, tests/test_gpu_trellis_score.py): the golden
fixtures they run on, a fixture's decode settings, and the invariant run's parameters.  No NaN, +inf or tie fixture: they
are outside trellis_score.reference_score's definition."""
import numpy as np

from golden_util import load_case, sync_kw

FIXTURES = ("m8_r3_L8_edge0", "m8_r3_L8_edge1", "m8_r3_L8_edge3",              # stale band: garbage lists, top_correct false
            "m6_r1_L8_unbanded", "m6_r1_L8_wide", "m6_r1_L4_indel", "m6_r1_L4_sync", "m6_r1_L4_sync_rc",
            "m6_r5_L8_rc", "m8_r2_L2_rc", "m8_r5_L8_rc", "m6_r3_L8")

_cases = {}


def case(name):
    """-> dict(name, m = the manifest entry, post, code = (mem_conv, rate, msg_len), rc, sync = keywords, md = max_deviation as a
    number, md_arg = as the manifest has it, None: the unbanded default); loaded once, and without the library: the GPU tests
    group the fixtures when they are collected"""
    if name not in _cases:
        m, post, _ = load_case(name)
        code = (m["mem_conv"], m["rate"], m["msg_len"])
        md = m["max_deviation"] if m["max_deviation"] is not None else m["msg_len"] + m["mem_conv"] + 1
        _cases[name] = dict(name=name, m=m, post=post, code=code, rc=bool(m["rc"]), sync=sync_kw(m), md=md,
                            md_arg=m["max_deviation"])
    return _cases[name]


def one_of_both(score, pair):
    """is the float32 `score` one of the two float32 values of `pair`, bit for bit?"""
    return np.float32(score).tobytes() in (np.float32(pair[0]).tobytes(), np.float32(pair[1]).tobytes())


# The invariant run (test_gpu_trellis_score.py): 64 reads of the device simulator at m = 8, rate 3, list size 8.  The seeds
# were chosen on the CPU -- simulate.reference_reads, float64 posteriors, the oracle's lists, reference_score -- so that the
# run with the simulator's default error rates has reads whose list holds the truth, and the run with the substitution
# rate raised has, besides those, reads whose full list misses it (on the CPU: 63 reads in the list and 1 missed by a full
# list in the first run, 6 and 58 in the second, no read in neither class).
INVARIANT = dict(mem_conv=8, rate=3, msg_len=64, list_size=8, max_deviation=10, n=64)
INVARIANT_RUNS = (dict(seed=1, sub=0.002, dele=0.0085, ins=0.0005), dict(seed=1, sub=0.1, dele=0.0085, ins=0.0005))
