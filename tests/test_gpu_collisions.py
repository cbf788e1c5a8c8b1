"""Fingerprint collisions on every step kernel: reads built for two or three DIFFERENT messages with the SAME 32-bit
fingerprint (collide_util: the fingerprint is linear over GF(2)), so that every time step after the paths merge presents a
fingerprint match that must fail its verification on the full message.  Each kernel verifies in code of its own --
wave_target's filter, the small-list confirmation, the lazy output phase (anchor and odd steps), the output phases of
lva_step_big and lva_step_big_rec, lva_step_exact's filter -- and a copy that took a match for a duplicate would drop a
genuine list entry.  Every case is held bit for bit (messages and score bits) to the CPU oracle, whose list holds all the
colliding messages (test_fingerprint_host.py asserts that half on the CPU).

On modes 2 and 4 each colliding read is decoded once more as a control -- the same seed, the difference plus one further bit,
so nothing collides -- and lva_profile.fixup_reason[3] (fingerprint collision) must be larger for the colliding read: the
collision path ran.  (Reason 3 also counts a message that sits in three lists, so the control's count is not zero.)"""
import numpy as np
import pytest

import collide_util as cu
import nanopore_dna_storage_amd as pkg
from nanopore_dna_storage_amd import synth

pytestmark = pytest.mark.gpu


def _same(g, want, what):
    want_msgs, want_scores = want
    assert not isinstance(g, int), "%s: error %r" % (what, g)
    assert g[0].shape == want_msgs.shape, "%s: %d entries, oracle %d" % (what, len(g[0]), len(want_msgs))
    assert np.array_equal(g[0], want_msgs), "%s: list differs" % what
    assert np.array_equal(g[1].view(np.uint32), want_scores.view(np.uint32)), "%s: scores differ" % what


def _plan(b, kernel, L, dominant):
    """the configuration runs the kernel the case names, on the layout it names"""
    plan = pkg.kernel_plan(b["m"], b["r"], b["msg_len"], L, cu.MAX_DEV, kernel=kernel)
    assert plan["dominant"] == dominant, plan
    assert plan["mode"] == {"fast": 2, "big": 2, "big_rec": 2, "lazy": 4, "wave": 3, "wave_wide": 3, "exact": 1}[dominant]
    assert plan["fixup"] == {2: "wave", 4: "lazy", 3: "none", 1: "none"}[plan["mode"]]
    assert (plan["rec"], plan["cmp"]) == {"big": (0, 1), "big_rec": (1, 0), "lazy": (0, 1)}.get(dominant, (0, 0))
    return plan


@pytest.mark.parametrize("name,kernel,L,dominant,drop", cu.RUNS,
                         ids=["%s-k%d-L%d-%s%s" % (n, k, L, d, "-short" if s else "") for n, k, L, d, s in cu.RUNS])
def test_colliding_messages_on_every_kernel(oracle, name, kernel, L, dominant, drop):
    b = cu.build(name, None, drop)
    m, r, msg_len, rc = b["m"], b["r"], b["msg_len"], b["rc"]
    plan = _plan(b, kernel, L, dominant)
    want = oracle.OracleCode(m, r, msg_len, rc=rc).decode(b["post"], L, cu.MAX_DEV, num_threads=16)
    assert cu.holds(want[0], b["msgs"])                        # the collision reaches the final list
    hit = ctl = None
    with pkg.Decoder(m, r, msg_len, list_size=L, max_deviation=cu.MAX_DEV, kernel=kernel, max_slots=1) as dec:
        assert dec.profile()["kernel"] == plan["mode"]
        got = dec.decode([b["post"]], rc=[rc])[0]
        if plan["mode"] in (2, 4):
            hit = dec.profile()["fixup_reason"][3]
            ctl_got = dec.decode([b["control_post"]], rc=[rc])[0]
            ctl = dec.profile()["fixup_reason"][3]
            assert not isinstance(ctl_got, int)
            print("fixup_reason[3] %s k%d L%d%s: colliding %d, control %d" % (name, kernel, L, " short" if drop else "", hit, ctl))
    _same(got, want, name)
    if hit is not None:
        assert hit > ctl, (hit, ctl)


@pytest.mark.parametrize("name,kernel,L,dominant", cu.MIXED)
def test_colliding_read_among_ordinary_reads_through_two_slots(oracle, name, kernel, L, dominant):
    """the collision's fix-up must not disturb its neighbours: five reads of both orientations through two slots"""
    b = cu.build(name)
    m, r, msg_len = b["m"], b["r"], b["msg_len"]
    _plan(b, kernel, L, dominant)
    reads = synth.make_reads(m, r, msg_len, 4, seed0=50, rc_mode="odd", margin=4.0)
    reads.insert(2, dict(post=b["post"], rc=b["rc"]))
    with pkg.Decoder(m, r, msg_len, list_size=L, max_deviation=cu.MAX_DEV, kernel=kernel, max_slots=2) as dec:
        assert dec.profile()["slots"] == 2
        got = dec.decode([x["post"] for x in reads], rc=[x["rc"] for x in reads])
    for i, (x, g) in enumerate(zip(reads, got)):
        want = oracle.OracleCode(m, r, msg_len, rc=x["rc"]).decode(x["post"], L, cu.MAX_DEV, num_threads=16)
        _same(g, want, "read %d" % i)
    assert cu.holds(got[2][0], b["msgs"])
