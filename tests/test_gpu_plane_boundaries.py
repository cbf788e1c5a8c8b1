"""Every step kernel at the message widths where the plane arithmetic can be off by one (tests/boundary_cases.py): totals
msg_len + mem_conv that end on a 64-bit plane (64, 128, 192, 256: the oldest message bit in bit 63 of the last plane, no
plane beyond), one bit short of it and one bit past it (a top plane that one position ever wrote, npair rising on the very
last step, the template instance and -- at 128/129 and 192/193 -- the record layout switching), codes whose two-bit
positions step over a boundary instead of landing on it, and the 32-bit word boundaries of the output path.  Lists and the
uint32 view of the scores against the CPU oracle, bit for bit; the plan of every run is asserted, so that no case runs on
another kernel than the one it names.

Per case three reads through two slots (the third reuses a slot whose planes hold an earlier read's bits): forward, reverse
complement, and one on a 0.5 grid whose score ties send targets through the fix-up and exact paths; odd and even block
counts (the lazy gather follows one hop after an odd last step).  Where the oracle is slow (65 entries on 192 bits, m = 11)
two reads: the forward one and the tie read, reverse complemented, through one slot.
test_plane_boundaries_host.py asserts what the shape list covers."""
import numpy as np
import pytest

import boundary_cases as bc
import nanopore_dna_storage_amd as pkg

pytestmark = pytest.mark.gpu


def _id(v):
    return v if isinstance(v, str) else "m%d-r%d-T%d" % (v[0], v[1], bc.total(v))


def _plan(kernel, code):
    """the configuration runs the kernel the case names, on the layout it names"""
    request, L, _ = bc.KERNELS[kernel]
    dominant = bc.dominant(kernel, code)
    plan = pkg.kernel_plan(*code, list_size=L, max_deviation=bc.MAX_DEV, kernel=request)
    assert plan["dominant"] == dominant, plan
    assert plan["mode"] == {"acs": 2, "fast": 2, "big": 2, "big_rec": 2, "lazy": 4, "wave": 3, "wave_wide": 3, "exact": 1}[dominant]
    assert (plan["rec"], plan["cmp"]) == {"acs": (0, 1), "big": (0, 1), "big_rec": (1, 0), "lazy": (0, 1)}.get(dominant, (0, 0))
    if kernel == "big32":
        assert plan["rec"] == (1 if bc.total(code) in (129, 191, 192) else 0) and plan["instance"] == 32
    return plan


def _run(oracle, kernel, code, reads, slots):
    request, L, _ = bc.KERNELS[kernel]
    plan = _plan(kernel, code)
    with pkg.Decoder(*code, list_size=L, max_deviation=bc.MAX_DEV, kernel=request, max_slots=slots) as dec:
        assert dec.profile()["kernel"] == plan["mode"] and dec.profile()["slots"] == slots
        got = dec.decode([x["post"] for x in reads], rc=[x["rc"] for x in reads])
        prof = dec.profile()
    for i, (x, g) in enumerate(zip(reads, got)):
        want_msgs, want_scores = oracle.OracleCode(*code, rc=x["rc"]).decode(x["post"], L, bc.MAX_DEV, num_threads=16)
        assert not isinstance(g, (int, np.integer)), "read %d: error %r" % (i, g)
        assert len(want_msgs) == L                                 # a full list of the oracle's: every entry is compared
        assert g[0].shape == want_msgs.shape, "read %d: %d entries, oracle %d" % (i, len(g[0]), len(want_msgs))
        assert np.array_equal(g[0], want_msgs), "read %d (nblk %d, rc %d): list differs" % (i, x["post"].shape[0], x["rc"])
        assert np.array_equal(g[1].view(np.uint32), want_scores.view(np.uint32)), "read %d: scores differ" % i
    return prof


def _reads(code, n):
    reads = bc.reads_for(code, n)
    assert len(reads) == n and len({x["post"].shape[0] & 1 for x in reads}) == 2       # odd and even block counts
    assert {x["rc"] for x in reads} == {False, True}
    return reads


@pytest.mark.parametrize("kernel,code", bc.RUNS, ids=_id)
def test_kernel_at_the_boundary_equals_the_oracle(oracle, kernel, code):
    slow = kernel == "wide65" and bc.total(code) > 128
    _run(oracle, kernel, code, _reads(code, 2 if slow else 3), 1 if slow else 2)


@pytest.mark.parametrize("kernel,code", bc.PRODUCTION_RUNS, ids=_id)
def test_full_last_plane_on_the_production_trellis(oracle, kernel, code):
    """m = 11: the 32-tile geometry with a last plane that is exactly full, one plane and three"""
    assert bc.total(code) in (64, 192)
    _run(oracle, kernel, code, _reads(code, 2), 1)


@pytest.mark.parametrize("kernel,code", bc.OVERFLOW_RUNS, ids=_id)
def test_whole_step_redo_at_a_full_last_plane(oracle, monkeypatch, kernel, code):
    """a 4-entry work list overflows on the tie read: the fix-up kernels redo whole steps on their exact paths"""
    monkeypatch.setenv("LVA_WORK_CAP", "4")
    tie = bc.reads_for(code)[2:]
    prof = _run(oracle, kernel, code, tie, 1)
    assert prof["overflow_steps"] > 0
