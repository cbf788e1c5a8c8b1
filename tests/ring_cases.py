"""The shapes of the ring-wrap tests, in one place: test_ring_cases_host.py asserts what this list covers,
test_gpu_ring_wrap.py decodes it.  The step kernels keep two parity buffers of R trellis positions, addressed modulo R,
R = min(nstate_pos, 2 max_deviation + ring_extra) (plan_config, csrc/lva_api.cpp; ring_extra: csrc/lva_plan.h).  The bands
below put 2 max_deviation + ring_extra on nstate_pos - 2, - 1, on nstate_pos itself and one above it (where the min clamps),
and on one value between half the trellis and nstate_pos - 2, where positions p and p + R that share a ring slot are both
well inside the trellis.

2 max_deviation + ring_extra has one parity per kernel, so the four crossover values take two trellis lengths of opposite
parity: msg_len 24 and 25, at rate 1 and at the punctured rate 3.  On the compact layout (cmp: acs, big, lazy) a slot holds
half as many lists at a one-bit position as at a two-bit one (compact_pos, csrc/lva_kernels.hip).  At rate 3 the two kinds
alternate, so a slot changes kind when R is odd -- and the lazy kernel's R is even unless it is clamped.  The lazy kernels
therefore also run a rate 5 code (kinds of period 3, nstate_pos 22, R = 20 = nstate_pos - 2: the one-bit position 1 and
the two-bit position 21 share a slot).  The record layout (big_rec)
exists at three message planes only: one shape of 129 bits, R = nstate_pos - 1, for its copy of the arithmetic.

The reads of a code are the same for every kernel and band, so that kernels of one list size share the oracle's decodes.
Block counts are exact (the dwell of every base is drawn to a given total): nstate_pos + 1 (the shortest the reference
accepts: the band advances on every step and its lower clip is active throughout) and + 2, 1.8 blocks per position (what
flappie emits), the 4.4 of the other tests, and 10, where the band's lower edge stands still for ten steps at a time."""
import functools

import numpy as np

import boundary_cases as bc
import nanopore_dna_storage_amd as pkg
from nanopore_dna_storage_amd import synth

M = bc.M
KERNELS = bc.KERNELS
CROSSOVER = (-2, -1, 0, 1)             # 2 max_deviation + ring_extra - nstate_pos
RATE1 = [(M, 1, 24), (M, 1, 25)]       # nstate_pos 31 and 32
RATE3 = [(M, 3, 24), (M, 3, 25)]       # nstate_pos 21 and 22: one-bit and two-bit positions in turn
RATE5 = (M, 5, 29)                     # nstate_pos 22, kinds of period 3: the lazy kernels, whose R is even
REC = (M, 1, 123)                      # 129 bits, three planes: lva_step_big_rec at 32 entries
GROUPS = {"rate1": RATE1, "rate3": RATE3}
COMPACT = ("acs1", "lazy2", "lazy8", "big12", "big32")          # cmp = 1: a slot's kind matters
REC_KINDS = ("tie", "plus2", "shortest", "too_short")           # the 129-bit shape: 11 ms of the oracle's per block
SLOTS = 2


def npos(code):
    return pkg.code_info(*code).nstate_pos


def plan(kernel, code, md):
    request, L, _ = KERNELS[kernel]
    return pkg.kernel_plan(*code, list_size=L, max_deviation=md, kernel=request)


def ring_extra(kernel, code):
    """from the plan, at a band far narrower than the trellis"""
    return plan(kernel, code, 1)["ring_positions"] - 2


def dominant(kernel, code):
    return bc.dominant(kernel, code)


def crossover_md(kernel, code, delta):
    """max_deviation with 2 md + ring_extra = nstate_pos + delta, or None where the parity does not allow it"""
    v = npos(code) + delta - ring_extra(kernel, code)
    return v // 2 if v >= 0 and v % 2 == 0 else None


def mid_md(kernel, code):
    """the ring nearest three quarters of the trellis, nstate_pos / 2 < R < nstate_pos - 2"""
    n, e = npos(code), ring_extra(kernel, code)
    ok = [md for md in range(n) if n / 2 < 2 * md + e < n - 2]
    return min(ok, key=lambda md: (abs(4 * (2 * md + e) - 3 * n), md))


def bands(kernel, code):
    """[(label, max_deviation, the ring length meant)]: the crossover values this code's parity reaches, then the mid value"""
    n, e = npos(code), ring_extra(kernel, code)
    out = [(d, crossover_md(kernel, code, d), min(n, n + d)) for d in CROSSOVER if crossover_md(kernel, code, d) is not None]
    md = mid_md(kernel, code)
    return out + [("mid", md, 2 * md + e)]


def _accepted(code):
    return bc.accepted(*code)


# ---- the matrix: per kernel and code group every crossover value on some code of the group, and a mid value on every code ----
# wide65 aside (its oracle is the slow one: two crossover shapes, below).  INTENDED lists what is meant, DROPPED what of it
# cannot be had (a refused length, a parity no code of the group reaches); test_ring_cases_host.py caps the share.
ALL_BUT_WIDE = bc.ALL_BUT_WIDE
INTENDED = [(k, g, d) for k in ALL_BUT_WIDE for g in GROUPS for d in CROSSOVER]
INTENDED += [(k, g, "mid-%d" % c[2]) for k in ALL_BUT_WIDE for g, codes in GROUPS.items() for c in codes]
DROPPED = []
RUNS = []                              # (kernel name, code): what the GPU test is parametrised by; the bands are bands(kernel, code)
for _k in ALL_BUT_WIDE:
    for _g, _codes in GROUPS.items():
        _live = [c for c in _codes if _accepted(c)]
        DROPPED += [(_k, _g, "mid-%d" % c[2]) for c in _codes if c not in _live]
        DROPPED += [(_k, _g, d) for d in CROSSOVER if not any(crossover_md(_k, c, d) is not None for c in _live)]
        RUNS += [(_k, c) for c in _live]
RUNS += [(k, RATE5) for k in ("lazy2", "lazy8")]


def _code_at(kernel, codes, delta):
    """the code of the group whose parity puts this kernel's ring on nstate_pos + delta"""
    return next(c for c in codes if crossover_md(kernel, c, delta) is not None)


# (kernel, code, label): the runs that are no full (kernel, code) case
WIDE_RUNS = [("wide65", _code_at("wide65", RATE1, d), d) for d in (-2, -1)]
REC_RUNS = [("big32", REC, -1)]
OVERFLOW_RUNS = [(k, _code_at(k, RATE1, -1), -1) for k in ("lazy8", "big12", "big32")]      # R = nstate_pos - 1, LVA_WORK_CAP = 4
OVERFLOW_KINDS = ("tie", "shortest")


def band_of(kernel, code, label):
    return next(b for b in bands(kernel, code) if b[0] == label)


# ---- reads ---------------------------------------------------------------------------------------------------------------

def lengths(n):
    """block counts by class.  The tie read's length is what makes the schedule below come out: through two slots, longest
    first, the reads after the longest fill the other slot, and the last but one still runs there when the longest ends."""
    return {"long": 10 * n, "default": round(4.4 * n), "tie": round(3.3 * n), "real": round(1.8 * n), "plus2": n + 2, "shortest": n + 1}


def read_with_dwell(code, seed, nblk, rc=False, margin=3.0, sigma=1.5, quantum=None):
    """synth.make_read with a given block count: one leading stay block, one block per base, and nblk - nstate_pos stays
    dealt to the bases at random (synth.true_transitions draws a Poisson number per base: the total is then not in hand)"""
    m, r, msg_len = code
    rng = np.random.default_rng(seed)
    msg = rng.integers(0, 2, size=msg_len, dtype=np.uint8)
    oligo = synth.encode(m, r, msg_len, msg)
    seq = synth.reverse_complement_bases(oligo) if rc else oligo
    extra = nblk - (len(seq) + 1)
    assert extra >= 0
    stays = rng.multinomial(extra, np.full(len(seq), 1.0 / len(seq)))
    states = synth.state_path(seq)
    lead = (int(states[0]) % 4 + 1 + int(rng.integers(0, 3))) % 4
    true_idx, cur = [synth.transition_index(lead, lead)], lead
    for st, k in zip(states, stays):
        st = int(st)
        true_idx += [synth.transition_index(cur, st)] + [synth.transition_index(st, st)] * int(k)
        cur = st
    assert len(true_idx) == nblk
    logits = rng.normal(0.0, sigma, size=(nblk, 40))
    logits[np.arange(nblk), np.asarray(true_idx)] += margin
    if quantum:
        post = (np.round((logits - logits.max(axis=1, keepdims=True)) / quantum) * quantum).astype(np.float32)
    else:
        mx = logits.max(axis=1, keepdims=True)
        post = (logits - (mx + np.log(np.exp(logits - mx).sum(axis=1, keepdims=True)))).astype(np.float32)
    return dict(msg=msg, oligo=oligo, read_bases=seq, post=post, rc=bool(rc), seed=seed)


# class -> (orientation, margin, quantum); "default" is the clean read whose message the oracle must return
READ_KINDS = {"long": (True, 3.0, None), "default": (False, 6.0, None), "tie": (True, 2.5, 0.5), "real": (False, 3.0, None),
              "plus2": (True, 3.5, None), "shortest": (False, 3.5, None)}
BATCH_ORDER = ("real", "shortest", "too_short", "long", "plus2", "tie", "default")      # as handed to decode()


@functools.lru_cache(maxsize=None)
def reads_for(code):
    """{class: read}; "too_short" is one block short of what the reference accepts (LVA_ERR_POST_TOO_SHORT, -6)"""
    m, r, msg_len = code
    n = npos(code)
    seed = 70000 + 1000 * r + 10 * (m + msg_len)
    out = {}
    for kind, nblk in lengths(n).items():
        rc, margin, quantum = READ_KINDS[kind]
        out[kind] = read_with_dwell(code, seed + list(READ_KINDS).index(kind), nblk, rc=rc, margin=margin, quantum=quantum)
    short = dict(out["shortest"])
    short["post"] = short["post"][:-1].copy()
    out["too_short"] = short
    return out


def batch(code, kinds=BATCH_ORDER):
    """[(class, read)] in the order the decoder is given them"""
    reads = reads_for(code)
    return [(kind, reads[kind]) for kind in BATCH_ORDER if kind in reads and kind in kinds]


def slot_history(nblks, nslots=SLOTS, lazy=False, min_blocks=0):
    """The batch schedule of lva_decode_batch, restated (decode_impl, csrc/lva_api.cpp): reads shorter than min_blocks take no
    slot, the others enter longest first (stable), an idle slot takes the next read, lowest slot first; a lazy decoder
    starts a read on an even launch.  -> per slot the indices of the reads it held, in order"""
    order = sorted((i for i, nb in enumerate(nblks) if nb >= min_blocks), key=lambda i: -nblks[i])
    held, end, hist = [None] * nslots, [0] * nslots, [[] for _ in range(nslots)]
    launch, nxt = 0, 0
    while True:
        for s in range(nslots):
            if held[s] is None and nxt < len(order):
                held[s] = order[nxt]
                nxt += 1
                end[s] = launch + (launch & 1 if lazy else 0) + nblks[held[s]]
                hist[s].append(held[s])
        if all(h is None for h in held):
            return hist
        launch += 1
        for s in range(nslots):
            if held[s] is not None and end[s] == launch:
                held[s] = None
