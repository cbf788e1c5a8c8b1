"""Every step kernel where its ring of R = min(nstate_pos, 2 max_deviation + ring_extra) trellis positions wraps inside the
trellis or just stops doing so (tests/ring_cases.py): 2 max_deviation + ring_extra on nstate_pos - 2, - 1, nstate_pos and
nstate_pos + 1 (clamped), and on a value about three quarters of the trellis, at rate 1 and at punctured rates whose
one-bit and two-bit positions share ring slots.  Lists and the uint32 view of the scores against the CPU oracle, bit for
bit; counts and error codes too; the plan of every run is asserted, so that no case runs on another kernel or ring than
the one it names.

Per band one batch through two slots: reads of exactly nstate_pos + 1 blocks (the shortest the reference accepts: the
band advances on every step, its lower clip is active throughout) and nstate_pos + 2, of 1.8, 3.3 (on a 0.5 grid: score
ties, the fix-up and heap-replay paths), 4.4 and 10 blocks per position (the band's lower edge stands still, the lazy
anchor and odd steps alternate on the same slots), odd and even block counts, both orientations, and one read a block too
short in the middle (-6, takes no slot).  The shortest read follows the longest one in slot 0: stale ring contents, and
ring slot 0 rewritten by the initial state.  test_ring_cases_host.py asserts all of that of the shape list.

Cost, measured once (16 oracle threads on 8 cores; decodes of one list size and band are shared between kernels): the
oracle's decodes of the whole file take 41 s -- acs1 1.5 s, lazy2 1.4 s, lazy8 4.3 s, fast4 / wave4 / exact4 1.8 s between
them, big12 5.0 s, big32 15.5 s, wide65 (two shapes) 7 s, the 129-bit record-layout shape 4.1 s (it goes without the three
longest reads: 11 ms of the oracle's per block), the overflow runs nothing of their own.  Nothing of the matrix is dropped."""
import numpy as np
import pytest

import nanopore_dna_storage_amd as pkg
import ring_cases as rc

pytestmark = pytest.mark.gpu

TOO_SHORT = -6
MODES = {"acs": 2, "fast": 2, "big": 2, "big_rec": 2, "lazy": 4, "wave": 3, "wave_wide": 3, "exact": 1}


def _id(v):
    return v if isinstance(v, str) else "m%d-r%d-n%d" % v if isinstance(v, tuple) else "R%+d" % v


def _run(oracle, kernel, code, band, reads):
    """one decoder, one batch of [(class, read)] through two slots -> its profile"""
    label, md, R = band
    request, L, _ = rc.KERNELS[kernel]
    plan = rc.plan(kernel, code, md)
    assert plan["dominant"] == rc.dominant(kernel, code) and plan["ring_positions"] == R, (plan, band)
    with pkg.Decoder(*code, list_size=L, max_deviation=md, kernel=request, max_slots=rc.SLOTS) as dec:
        assert dec.profile()["kernel"] == MODES[plan["dominant"]] and dec.profile()["slots"] == rc.SLOTS
        got = dec.decode([x["post"] for _, x in reads], rc=[x["rc"] for _, x in reads])
        prof = dec.profile()
    assert len(got) == len(reads)
    for (kind, x), g in zip(reads, got):
        what = "%s %s, band %r, %s read (nblk %d, rc %d)" % (kernel, _id(code), band, kind, x["post"].shape[0], x["rc"])
        oc = oracle.OracleCode(*code, rc=x["rc"])
        if kind == "too_short":
            with pytest.raises(oracle.OracleError) as e:
                oc.decode(x["post"], L, md, num_threads=16)
            assert e.value.status == TOO_SHORT and isinstance(g, (int, np.integer)) and g == TOO_SHORT, what
            continue
        want_msgs, want_scores = oc.decode(x["post"], L, md, num_threads=16)
        assert not isinstance(g, (int, np.integer)), "%s: error %r" % (what, g)
        assert len(want_msgs) == L, what                           # a full list of the oracle's: every entry is compared
        if kind == "default":
            assert np.array_equal(want_msgs[0], x["msg"]), what    # the clean read is decoded, not just agreed upon
        assert g[0].shape == want_msgs.shape, "%s: %d entries, oracle %d" % (what, len(g[0]), len(want_msgs))
        assert np.array_equal(g[0], want_msgs), "%s: list differs" % what
        assert np.array_equal(g[1].view(np.uint32), want_scores.view(np.uint32)), "%s: scores differ" % what
    if plan["fixup"] != "none" and any(kind == "tie" for kind, _ in reads):
        assert prof["fixup_states"] > 0, (kernel, code, band)      # the ties did reach the fix-up
    return prof


@pytest.mark.parametrize("kernel,code", rc.RUNS, ids=_id)
def test_kernel_at_the_ring_crossover_equals_the_oracle(oracle, kernel, code):
    bands = rc.bands(kernel, code)
    assert len(bands) == 3 and bands[-1][0] == "mid"
    for band in bands:
        _run(oracle, kernel, code, band, rc.batch(code))


@pytest.mark.parametrize("kernel,code,label", rc.WIDE_RUNS, ids=_id)
def test_wide_kernel_with_a_ring_just_shorter_than_the_trellis(oracle, kernel, code, label):
    _run(oracle, kernel, code, rc.band_of(kernel, code, label), rc.batch(code))


@pytest.mark.parametrize("kernel,code,label", rc.REC_RUNS, ids=_id)
def test_record_layout_with_a_ring_one_shorter_than_the_trellis(oracle, kernel, code, label):
    """lva_step_big_rec has its own copy of the ring arithmetic and exists at three message planes only"""
    assert rc.dominant(kernel, code) == "big_rec"
    _run(oracle, kernel, code, rc.band_of(kernel, code, label), rc.batch(code, rc.REC_KINDS))


@pytest.mark.parametrize("kernel,code,label", rc.OVERFLOW_RUNS, ids=_id)
def test_whole_step_redo_with_a_ring_one_shorter_than_the_trellis(oracle, monkeypatch, kernel, code, label):
    """a 4-entry work list overflows on the tie read: the fix-up kernels redo whole steps on their exact paths"""
    monkeypatch.setenv("LVA_WORK_CAP", "4")
    prof = _run(oracle, kernel, code, rc.band_of(kernel, code, label), rc.batch(code, rc.OVERFLOW_KINDS))
    assert prof["overflow_steps"] > 0
