"""Messages with one fingerprint, and reads that favour all of them: the inputs of test_fingerprint_host.py (CPU) and
test_gpu_collisions.py (GPU).

The fingerprint the step kernels de-duplicate on is linear over GF(2): fp(M) = fp(0) ^ XOR over the set bits j of M of a
fixed word w_j.  The words are taken from the library itself (pkg.code_fingerprint of the one-bit messages), never
restated here, so the order in which a code consumes its message bits -- rate, reverse complement -- cannot be got wrong.
Any 33 words of 32 bits are linearly dependent: Gaussian elimination finds a non-empty set d of message positions inside a
window of 33 whose words XOR to zero, and then M and M ^ d are different messages with the same fingerprint.

A read is built for ALL the messages of a case at once: one dwell sequence, synth's N(0, 1.5^2) logits, +margin on the
transition of every message's path at every block.  Once the trellis has consumed the last bit of d and mem_conv more,
the paths share their conv state and their future, so they are candidates for the same targets at every later step: a true
collision per step, and the final list must hold every message.
"""
import functools

import numpy as np

import nanopore_dna_storage_amd as pkg
from nanopore_dna_storage_amd import synth

FULL = 0xFFFFFFFF
UPPER29 = 0xFFFFFFF8       # what the small-list merge compares (csrc/lva_kernels.hip fast_merge_core)
WINDOW = 33


def bit_words(m, r, msg_len, rc=False):
    """w_j of every message position j (encode()'s order): fp(one-bit message j) ^ fp(all-zero message), from the library"""
    zero = np.zeros(msg_len, np.uint8)
    f0 = pkg.code_fingerprint(m, r, msg_len, zero, rc=rc)
    out = []
    for j in range(msg_len):
        e = zero.copy()
        e[j] = 1
        out.append(pkg.code_fingerprint(m, r, msg_len, e, rc=rc) ^ f0)
    return out


def kernel_vectors(words, mask=FULL):
    """Gaussian elimination over GF(2): -> index sets (bit i of an int = words[i] takes part) whose words XOR to zero under
    `mask`.  Each set holds an index that no earlier set holds, so they are linearly independent."""
    basis, out = {}, []
    for i, w in enumerate(words):
        v, combo = w & mask, 1 << i
        while v:
            p = v.bit_length() - 1
            if p not in basis:
                basis[p] = (v, combo)
                break
            v, combo = v ^ basis[p][0], combo ^ basis[p][1]
        else:
            out.append(combo)
    return out


def _as_bits(combo, lo, msg_len):
    d = np.zeros(msg_len, np.uint8)
    for i in range(combo.bit_length()):
        if (combo >> i) & 1:
            d[lo + i] = 1
    return d


def xor_words(words, d):
    x = 0
    for j in np.flatnonzero(d):
        x ^= words[int(j)]
    return x


def find_differences(m, r, msg_len, lo, rc=False, count=1, width=None):
    """`count` linearly independent differences d (uint8 [msg_len]) inside message positions [lo, lo + width) with
    fp(M ^ d) == fp(M) for every M; width defaults to the smallest that guarantees them, 32 + count."""
    width = WINDOW + count - 1 if width is None else width
    assert 0 <= lo and lo + width <= msg_len
    words = bit_words(m, r, msg_len, rc)
    found = kernel_vectors(words[lo:lo + width])
    assert len(found) >= count
    return [_as_bits(c, lo, msg_len) for c in found[:count]]


def find_upper29_difference(m, r, msg_len, lo, rc=False):
    """a difference inside [lo, lo + 33) under which the fingerprint keeps its upper 29 bits and changes its low three"""
    words = bit_words(m, r, msg_len, rc)
    found = kernel_vectors(words[lo:lo + WINDOW], UPPER29)
    cands = found + [a ^ b for k, a in enumerate(found) for b in found[k + 1:]]
    for c in cands:
        d = _as_bits(c, lo, msg_len)
        if xor_words(words, d) & 7:
            return d
    raise AssertionError("every upper-29 match in the window is a full match")


def further_bit(d, lo, width=WINDOW):
    """d plus one further bit of the window: the control of a colliding pair (fingerprints differ: no word is zero)"""
    out = d.copy()
    free = [j for j in range(lo, lo + width) if not d[j]]
    out[free[len(free) // 2]] = 1
    return out


def shared_read(m, r, msg_len, msgs, rng, rc=False, margin=6.0, sigma=1.5, mean_extra_dwell=3.4):
    """synth's recipe (synth.true_transitions, synth.posteriors_from_bases) for several messages at once: one leading stay
    block, one dwell sequence for all, +margin on the true transition of EVERY message's path -> float32 [nblk, 40]"""
    oligos = [pkg.encode(m, r, msg_len, x) for x in msgs]
    seqs = [synth.reverse_complement_bases(o) if rc else o for o in oligos]
    n = len(seqs[0])
    dwell = rng.poisson(mean_extra_dwell, size=n)
    lead = (int(seqs[0][0]) + 1 + int(rng.integers(0, 3))) % 4
    assert all(int(s[0]) == int(seqs[0][0]) for s in seqs)          # the paths part after their first base
    paths = []
    for s in seqs:
        idx, cur = [synth.transition_index(lead, lead)], lead
        for st, extra in zip(synth.state_path(s), dwell):
            st = int(st)
            idx.append(synth.transition_index(cur, st))
            idx.extend([synth.transition_index(st, st)] * int(extra))
            cur = st
        paths.append(np.asarray(idx))
    nblk = len(paths[0])
    logits = rng.normal(0.0, sigma, size=(nblk, 40))
    true = np.zeros((nblk, 40), bool)
    for p in paths:
        true[np.arange(nblk), p] = True
    logits[true] += margin
    mx = logits.max(axis=1, keepdims=True)
    lse = mx + np.log(np.exp(logits - mx).sum(axis=1, keepdims=True))
    return (logits - lse).astype(np.float32)


MAX_DEV = 20

# The constructed reads.  kind: "pair" = M, M ^ d;  "low3" = a pair that agrees in the upper 29 bits only;  "triple" = M, M ^ d1,
# M ^ d2 with d1, d2 inside 34 positions.  lo: first message position of the window (a reverse complement consumes the
# message from its far end, so its window sits there).  seed: chosen on the CPU so that the oracle's list holds every message at
# every list size of RUNS below (test_fingerprint_host.py asserts it); the message, the dwells and the noise all come from it.
# The stored message is a shift register (newest bit = bit 0): a difference at positions [lo, lo + 33) lies wholly in the
# SECOND 64-bit plane once lo + 33 + 64 bits are consumed, in the THIRD after lo + 33 + 128 -- "plane2" / "plane3" put the
# window at the start of the message so that the last steps of the read see it there.  (A window behind message position 64
# of a 100-bit message would stay in the first plane to the end, and merge only two positions before the last one.)
CASES = {
    "pair60": dict(m=6, r=1, msg_len=60, kind="pair", lo=10, rc=False, seed=7),
    "wide60": dict(m=6, r=1, msg_len=60, kind="pair", lo=10, rc=False, seed=7),
    "pair124": dict(m=6, r=1, msg_len=124, kind="pair", lo=20, rc=False, seed=1),
    "low3": dict(m=6, r=1, msg_len=60, kind="low3", lo=10, rc=False, seed=7),
    "plane2": dict(m=8, r=1, msg_len=100, kind="pair", lo=2, rc=False, seed=7),
    "plane3": dict(m=6, r=5, msg_len=180, kind="pair", lo=4, rc=False, seed=7),
    "triple": dict(m=6, r=1, msg_len=60, kind="triple", lo=10, rc=False, seed=7),
    "rc60": dict(m=6, r=1, msg_len=60, kind="pair", lo=17, rc=True, seed=7),
}


@functools.lru_cache(maxsize=None)
def build(name, seed=None, drop_last=False):
    """-> dict(msgs = the colliding messages, post, control_msgs, control_post, rc, and the case's fields).  The control is
    the same recipe from the same seed with every difference replaced by itself plus one further bit: nothing collides.
    drop_last: both reads without their last block (the other parity of the last time step)."""
    c = dict(CASES[name])
    m, r, msg_len, lo, rc = c["m"], c["r"], c["msg_len"], c["lo"], c["rc"]
    seed = c["seed"] if seed is None else seed
    if c["kind"] == "pair":
        ds = find_differences(m, r, msg_len, lo, rc)
    elif c["kind"] == "low3":
        ds = [find_upper29_difference(m, r, msg_len, lo, rc)]
    else:
        ds = find_differences(m, r, msg_len, lo, rc, count=2)
    width = WINDOW + len(ds) - 1
    controls = [further_bit(d, lo, width) for d in ds]
    if len(controls) == 2 and np.array_equal(controls[0] ^ ds[0], controls[1] ^ ds[1]):      # two different further bits
        free = [j for j in range(lo, lo + width) if not ds[1][j] and not (controls[0] ^ ds[0])[j]]
        controls[1] = ds[1].copy()
        controls[1][free[0]] = 1
    out = dict(c, name=name, seed=seed, differences=ds)
    for key, diffs in (("", ds), ("control_", controls)):
        rng = np.random.default_rng(seed)
        M = rng.integers(0, 2, size=msg_len, dtype=np.uint8)
        msgs = [M] + [M ^ d for d in diffs]
        post = shared_read(m, r, msg_len, msgs, rng, rc=rc)
        out[key + "msgs"] = msgs
        out[key + "post"] = post[:-1].copy() if drop_last else post
    return out


def holds(msg_list, msgs):
    """does a decoded list (uint8 [count, msg_len]) hold every one of msgs?"""
    return all(any(np.array_equal(row, x) for row in msg_list) for x in msgs)


# What the GPU test runs: (case, kernel mode asked for, list size, the step kernel that must serve it, read without its last block).
# The smallest shapes that reach each kernel; lva_step_big_rec takes three message planes (lva_plan.h), hence pair124.
RUNS = []
for _L in (2, 4, 8):
    RUNS.append(("pair60", 2, _L, "fast", False))
    RUNS += [("pair60", _k, _L, "lazy", _drop) for _k in (4, 0) for _drop in (False, True)]     # both parities of the last step
    RUNS += [("low3", 2, _L, "fast", False), ("low3", 4, _L, "lazy", False)]
RUNS += [("pair60", 2, 12, "big", False), ("pair60", 2, 16, "big", False),                      # compact lists at every position
         ("pair124", 2, 32, "big_rec", False), ("pair124", 2, 64, "big_rec", False),
         ("pair60", 3, 8, "wave", False), ("wide60", 3, 100, "wave_wide", False), ("pair60", 1, 4, "exact", False),
         ("plane2", 2, 4, "fast", False), ("plane2", 4, 4, "lazy", False), ("plane2", 2, 12, "big", False),
         ("plane3", 2, 8, "fast", False), ("plane3", 4, 8, "lazy", False), ("plane3", 2, 12, "big", False),   # plain and compact lists
         ("triple", 2, 4, "fast", False), ("triple", 4, 4, "lazy", False), ("triple", 2, 8, "fast", False),
         ("triple", 4, 8, "lazy", False), ("triple", 2, 12, "big", False),
         ("rc60", 2, 4, "fast", False), ("rc60", 4, 4, "lazy", False)]
MIXED = [("pair60", 2, 4, "fast"), ("pair60", 4, 4, "lazy")]      # one colliding read among ordinary ones, two slots


def oracle_decodes():
    """every (case, drop_last, list size) the GPU test compares with the oracle, once"""
    seen = []
    for name, _, L, _, drop in RUNS + [x + (False,) for x in MIXED]:
        if (name, drop, L) not in seen:
            seen.append((name, drop, L))
    return seen
