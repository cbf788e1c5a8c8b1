"""The message fingerprint of the step kernels, without a GPU: lva_code_fingerprint against a plain restatement, its
linearity, the finder of colliding messages (collide_util), and the CPU half of test_gpu_collisions.py's guard -- the
oracle's list of every constructed read holds every colliding message."""
import numpy as np
import pytest

import collide_util as cu
import nanopore_dna_storage_amd as pkg

MASK64 = (1 << 64) - 1
# (m, rate, msg_len): every block pattern with two-bit positions (rates 2, 3, 5, 7) and the one without
CODES = [(6, 1, 60), (8, 2, 100), (6, 3, 60), (6, 5, 180), (8, 5, 100), (6, 7, 92), (11, 7, 101)]


def splitmix_word(i):
    """the fixed word of the i-th bit a path consumes (csrc/lva_code.cpp fp_word), restated"""
    z = ((i + 1) * 0x9E3779B97F4A7C15) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    z ^= z >> 31
    return ((z >> 16) & 0xFFFFFFFF) | 1


def plain_fingerprint(m, r, msg_len, msg, n_bits, rc):
    """XOR of the words of the set bits among the first n_bits consumed: the message forwards (backwards for a reverse
    complement), then -- for a whole message -- the terminating bits that lead to the final state"""
    consumed = [int(b) for b in (msg[::-1] if rc else msg)][:n_bits]
    if n_bits == msg_len:
        fin = pkg.code_info(m, r, msg_len, rc=rc).final_state
        consumed += [(fin >> k) & 1 for k in range(m)]
    fp = 0
    for i, b in enumerate(consumed):
        if b:
            fp ^= splitmix_word(i)
    return fp


@pytest.mark.parametrize("rc", [False, True])
@pytest.mark.parametrize("sync", ["", "101"])
@pytest.mark.parametrize("m,r,msg_len", CODES)
def test_library_fingerprint_equals_the_plain_restatement(m, r, msg_len, rc, sync):
    rng = np.random.default_rng(1000 * m + 10 * r + rc)
    period = 11 if sync else 0
    bounds = {int(x) for x in pkg.code_tables(m, r, msg_len, rc, sync, period)["pos2msg"]}     # bits consumed on arrival at a position
    partial = sorted(x for x in bounds if x <= msg_len)
    assert len(partial) > msg_len // 2
    for _ in range(6):
        msg = rng.integers(0, 2, size=msg_len, dtype=np.uint8)
        for n in [msg_len] + [int(x) for x in rng.choice(partial, size=8)]:
            got = pkg.code_fingerprint(m, r, msg_len, msg, n_bits=n, rc=rc, sync_marker=sync, sync_period=period)
            assert got == plain_fingerprint(m, r, msg_len, msg, n, rc), (n, rc)
    assert pkg.code_fingerprint(m, r, msg_len, msg, n_bits=0, rc=rc) == 0


def test_prefixes_no_path_holds_are_refused():
    msg = np.ones(180, np.uint8)
    inside = [n for n in range(181) if n not in {int(x) for x in pkg.code_tables(6, 5, 180)["pos2msg"]}]
    assert inside                                                          # rate 5 has two-bit positions
    for n in inside[:3] + [181]:
        with pytest.raises(pkg.LvaError):
            pkg.code_fingerprint(6, 5, 180, msg, n_bits=n)
    with pytest.raises(pkg.LvaError):
        pkg.code_fingerprint(6, 5, 180, msg[:-1])


@pytest.mark.parametrize("rc", [False, True])
@pytest.mark.parametrize("m,r,msg_len", CODES)
def test_fingerprint_is_linear(m, r, msg_len, rc):
    rng = np.random.default_rng(7 + m + r)
    f0 = pkg.code_fingerprint(m, r, msg_len, np.zeros(msg_len, np.uint8), rc=rc)
    for _ in range(8):
        a, b = rng.integers(0, 2, size=(2, msg_len), dtype=np.uint8)
        fa, fb, fab = (pkg.code_fingerprint(m, r, msg_len, x, rc=rc) for x in (a, b, a ^ b))
        assert fab == fa ^ fb ^ f0


@pytest.mark.parametrize("m,r,msg_len,rc,los", [(6, 1, 60, False, (0, 4, 10, 20, 27)), (6, 1, 60, True, (0, 17, 27)),
                                                 (8, 1, 100, False, (2, 30, 66)), (6, 5, 180, False, (4, 40, 130, 147)),
                                                 (6, 5, 180, True, (3, 146))])
def test_finder(m, r, msg_len, rc, los):
    rng = np.random.default_rng(99)
    fp = lambda x: pkg.code_fingerprint(m, r, msg_len, x, rc=rc)           # noqa: E731
    for lo in los:
        M = rng.integers(0, 2, size=msg_len, dtype=np.uint8)
        (d,) = cu.find_differences(m, r, msg_len, lo, rc)
        assert d.any() and not d[:lo].any() and not d[lo + 33:].any()
        assert fp(M ^ d) == fp(M) and not np.array_equal(M ^ d, M)
        assert fp(M ^ cu.further_bit(d, lo)) != fp(M)                      # the control does not collide
        # the small-list merge's view: upper 29 bits equal, low three different
        d = cu.find_upper29_difference(m, r, msg_len, lo, rc)
        assert d.any() and not d[:lo].any() and not d[lo + 33:].any()
        x = fp(M ^ d) ^ fp(M)
        assert x & cu.UPPER29 == 0 and x & 7 != 0
        assert (fp(M ^ cu.further_bit(d, lo)) ^ fp(M)) & cu.UPPER29 != 0
        # three messages under one fingerprint: two independent differences inside 34 positions
        if lo + 34 <= msg_len:
            d1, d2 = cu.find_differences(m, r, msg_len, lo, rc, count=2)
            assert not d1[:lo].any() and not d1[lo + 34:].any() and not d2[:lo].any() and not d2[lo + 34:].any()
            assert d1.any() and d2.any() and (d1 ^ d2).any()
            assert fp(M ^ d1) == fp(M) == fp(M ^ d2)


@pytest.mark.parametrize("name", sorted(cu.CASES))
def test_cases_are_what_they_claim(name):
    """the messages of a case share their fingerprint (their upper 29 bits for "low3"), the control's do not; the difference
    sits where the case says: by the end of the read in the second / third 64-bit plane of the stored message"""
    b = cu.build(name)
    m, r, msg_len, rc = b["m"], b["r"], b["msg_len"], b["rc"]
    fps = [pkg.code_fingerprint(m, r, msg_len, x, rc=rc) for x in b["msgs"]]
    ctl = [pkg.code_fingerprint(m, r, msg_len, x, rc=rc) for x in b["control_msgs"]]
    assert len({x.tobytes() for x in b["msgs"]}) == len(b["msgs"]) == (3 if b["kind"] == "triple" else 2)
    if b["kind"] == "low3":
        assert (fps[0] ^ fps[1]) & cu.UPPER29 == 0 and fps[0] != fps[1]
    else:
        assert len(set(fps)) == 1
    assert len({x & cu.UPPER29 for x in ctl}) == len(ctl)
    for d in b["differences"]:
        newest = (msg_len + m - 1) - int(np.flatnonzero(d).max())          # stored bit index of d's last bit after the final step
        if name in ("plane2", "plane3"):
            assert newest >= (64 if name == "plane2" else 128)


@pytest.mark.parametrize("name,drop,L", cu.oracle_decodes())
def test_oracle_list_holds_every_colliding_message(oracle, name, drop, L):
    """the CPU half of test_gpu_collisions.py's guard: what the GPU is compared with holds all the colliding messages, so the
    collision reaches the final list and a kernel that dropped one of them could not pass"""
    b = cu.build(name, None, drop)
    code = oracle.OracleCode(b["m"], b["r"], b["msg_len"], rc=b["rc"])
    msgs, _ = code.decode(b["post"], L, cu.MAX_DEV, num_threads=16)
    assert cu.holds(msgs, b["msgs"])
