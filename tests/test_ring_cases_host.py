"""The ring wrap and the read-length extremes, the half that needs no GPU: what tests/ring_cases.py (the shapes
test_gpu_ring_wrap.py decodes) covers.  The ring length of every run is the one meant and the kernel the one named; the
band tables of the reads do what their length class is there for (lva_band_table: the reference's band and the band the
kernels work on); positions that share a ring slot are both in band, and at the punctured rates of both kinds; the batch
schedule puts the shortest read into the slot the longest one left."""
import numpy as np
import pytest

import nanopore_dna_storage_amd as pkg
import ring_cases as rc

# ring positions beyond the band's 2 max_deviation: the position below the band that a step reads, and for the lazy kernel the
# one below that (its two-hop chains reach lo - 2: csrc/lva_plan.h).  The shape list takes the number from the plan; this is
# what the plan has to say.
RING_EXTRA = {"lazy": 2}
ALL_RUNS = ([(k, c, b) for k, c in rc.RUNS for b in rc.bands(k, c)]
            + [(k, c, rc.band_of(k, c, lab)) for k, c, lab in rc.WIDE_RUNS + rc.REC_RUNS + rc.OVERFLOW_RUNS])
CODES = sorted({c for _, c, _ in ALL_RUNS})


def _id(v):
    return v if isinstance(v, str) else "m%d-r%d-n%d" % v


def _bands_of(code):
    """every max_deviation some kernel decodes this code at"""
    return sorted({b[1] for _, c, b in ALL_RUNS if c == code})


def _work(code, x, md):
    ref, work = pkg.band_table(*code, x["post"].shape[0], md, rc=x["rc"])
    return ref, work


# ---- ring positions ----------------------------------------------------------------------------------------------------

def test_ring_positions_and_kernel_of_every_run():
    for k, code, (label, md, R) in ALL_RUNS:
        n = rc.npos(code)
        plan = rc.plan(k, code, md)
        want = rc.dominant(k, code)
        assert plan["dominant"] == want, (k, code, plan)
        extra = RING_EXTRA.get(want, 1)
        assert rc.ring_extra(k, code) == extra, (k, code)
        assert plan["ring_positions"] == R == min(n, 2 * md + extra), (k, code, label, md, plan)
        if label == "mid":
            assert n / 2 < R < n - 2 and R == 2 * md + extra
        else:
            assert label in rc.CROSSOVER and 2 * md + extra == n + label
    assert rc.dominant("big32", rc.REC) == "big_rec" and {rc.dominant(k, c) for k, c in rc.RUNS} == {
        "acs", "lazy", "fast", "big", "wave", "exact"}


def test_every_crossover_value_on_every_kernel():
    """nstate_pos - 2, - 1, nstate_pos and the clamped nstate_pos + 1, per kernel at rate 1 and at rate 3, and a mid value
    on every code; the wide kernel at exactly two crossover shapes below the trellis length"""
    for k in rc.ALL_BUT_WIDE:
        for g, codes in rc.GROUPS.items():
            seen = {b[0] for kk, c in rc.RUNS if kk == k and c in codes for b in rc.bands(k, c)}
            assert seen == set(rc.CROSSOVER) | {"mid"}, (k, g, seen)
        assert {c for kk, c in rc.RUNS if kk == k} >= set(rc.RATE1 + rc.RATE3)
    assert {k for k, _ in rc.RUNS} == set(rc.ALL_BUT_WIDE) and set(rc.KERNELS) == set(rc.ALL_BUT_WIDE) | {"wide65"}
    assert rc.WIDE_RUNS == [("wide65", rc.RATE1[0], -2), ("wide65", rc.RATE1[1], -1)]
    assert rc.OVERFLOW_RUNS == [("lazy8", rc.RATE1[0], -1), ("big12", rc.RATE1[1], -1), ("big32", rc.RATE1[1], -1)]
    assert sorted({k for k, _, _ in rc.OVERFLOW_RUNS}) == ["big12", "big32", "lazy8"]
    for k, code, lab in rc.WIDE_RUNS + rc.REC_RUNS + rc.OVERFLOW_RUNS:
        assert rc.band_of(k, code, lab)[2] == rc.npos(code) + lab < rc.npos(code)
    assert all(lab == -1 for _, _, lab in rc.REC_RUNS + rc.OVERFLOW_RUNS)


def test_omissions_are_capped():
    """what the list means to hold and cannot (a refused length, a parity no code of the group reaches) is counted"""
    assert len(rc.INTENDED) == len(rc.ALL_BUT_WIDE) * len(rc.GROUPS) * (len(rc.CROSSOVER) + 2)
    assert set(rc.DROPPED) <= set(rc.INTENDED)
    assert 10 * len(rc.DROPPED) <= len(rc.INTENDED), "dropped: %r" % (rc.DROPPED,)
    for code in rc.RATE1 + rc.RATE3 + [rc.RATE5, rc.REC]:
        pkg.code_info(*code)                                    # every code is accepted
    assert {rc.npos(c) & 1 for c in rc.RATE1} == {rc.npos(c) & 1 for c in rc.RATE3} == {0, 1}


# ---- the reads -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("code", CODES, ids=_id)
def test_reads_of_every_length_class(code):
    n = rc.npos(code)
    reads = rc.reads_for(code)
    nblk = {kind: x["post"].shape[0] for kind, x in reads.items()}
    assert nblk == dict(rc.lengths(n), too_short=n)
    assert nblk["shortest"] == n + 1 and nblk["plus2"] == n + 2 and nblk["long"] >= 10 * n
    assert abs(nblk["real"] - 1.8 * n) <= 0.5 and abs(nblk["default"] - 4.4 * n) <= 0.5
    for kinds in (rc.BATCH_ORDER, rc.REC_KINDS) if code == rc.REC else (rc.BATCH_ORDER,):
        live = [reads[kind] for kind in kinds if kind != "too_short"]
        assert {x["post"].shape[0] & 1 for x in live} == {0, 1} and {x["rc"] for x in live} == {False, True}
    tie = reads["tie"]["post"]
    assert np.array_equal(tie, np.round(tie * 2) / 2) and not np.array_equal(reads["default"]["post"], np.round(reads["default"]["post"] * 2) / 2)
    assert [kind for kind, _ in rc.batch(code)] == list(rc.BATCH_ORDER) and rc.BATCH_ORDER.index("too_short") not in (0, len(rc.BATCH_ORDER) - 1)
    for x in reads.values():
        assert np.all(np.isfinite(x["post"])) and x["post"].dtype == np.float32
        assert len(x["read_bases"]) == n - 1


@pytest.mark.parametrize("lazy", [False, True])
@pytest.mark.parametrize("code", CODES, ids=_id)
def test_the_shortest_read_follows_the_longest_in_its_slot(code, lazy):
    """through two slots, longest first: the shortest read is decoded on the ring the longest one left behind, slot 0 of
    it rewritten by the initial state"""
    kinds = [kind for kind, _ in rc.batch(code)]
    nblk = [x["post"].shape[0] for _, x in rc.batch(code)]
    hist = rc.slot_history(nblk, rc.SLOTS, lazy, min_blocks=rc.npos(code) + 1)
    named = [[kinds[i] for i in h] for h in hist]
    assert sorted(sum(named, [])) == sorted(set(kinds) - {"too_short"})
    assert named[0] == ["long", "shortest"], named
    if code == rc.REC:                                          # its shorter batch: the shortest read after the one of n + 2 blocks
        sub = [i for i, kind in enumerate(kinds) if kind in rc.REC_KINDS]
        hist = rc.slot_history([nblk[i] for i in sub], rc.SLOTS, lazy, min_blocks=rc.npos(code) + 1)
        assert [[kinds[sub[i]] for i in h] for h in hist] == [["tie"], ["plus2", "shortest"]]


# ---- the band tables -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("code", CODES, ids=_id)
def test_band_of_the_shortest_and_of_the_longest_read(code):
    reads = rc.reads_for(code)
    for md in _bands_of(code):
        for kind in ("shortest", "plus2"):
            ref, work = _work(code, reads[kind], md)
            assert np.all(work[:, 0] >= ref[:, 0]) and np.all(work[:, 1] <= ref[:, 1])
            assert np.any(work[:, 0] > ref[:, 0]), (code, md, kind)                       # the lower clip is active
        ref, work = _work(code, reads["shortest"], md)
        lo = work[:, 0]
        assert np.count_nonzero(np.diff(lo) > 0) > (len(lo) - 1) * 0.9                       # ... and the edge advances on most steps
        assert np.count_nonzero(work[:, 0] > ref[:, 0]) > len(lo) / 2
        ref, work = _work(code, reads["long"], md)
        lo = work[:, 0]
        runs = np.diff(np.flatnonzero(np.concatenate([[True], np.diff(lo) != 0, [True]])))
        # the edge stands still eight steps and more at a time, also once it has left position 0 (the clip moves it at the very end)
        assert lo[0] == 0 and np.count_nonzero(runs[1:] >= 8) >= 3, (code, md, runs)


def test_wrapped_positions_are_in_band():
    """R < nstate_pos: every read's band reaches positions p >= R, and on some step holds R - 1 and R -- the last slot of the
    ring and slot 0 again -- together"""
    checked = 0
    for k, code, (label, md, R) in ALL_RUNS:
        if R >= rc.npos(code):
            continue
        for kind, x in rc.batch(code):
            if kind == "too_short":
                continue
            _, work = _work(code, x, md)
            assert work[:, 1].max() == rc.npos(code) > R
            assert np.any((work[:, 0] < R) & (R < work[:, 1])), (k, code, label, kind)
            assert np.all(work[:, 1] - work[:, 0] <= R - rc.ring_extra(k, code))          # no two positions of a step share a slot
            checked += 1
    assert checked > 200


def _kinds(code, orient):
    """per position: does the compact layout halve its lists (compact_pos, csrc/lva_kernels.hip)"""
    ptype = pkg.code_tables(*code, rc=orient)["ptype"]
    return [p >= 1 and int(ptype[p]) == 0 for p in range(len(ptype))], [int(t) == 0 for t in ptype]


def test_ring_slots_change_kind_at_the_punctured_rates():
    """some positions p and p + R are a one-bit and a two-bit position, on every kernel at every punctured code, and in both
    orientations (at R = nstate_pos - 1 the one pair is 0 and R: not in every run); on the kernels with compact lists, whose
    slot layout depends on it, with p >= 1 (position 0 is never compact), at a crossover value as well as at the mid value"""
    seen, mixed = {}, set()
    for k, code, (label, md, R) in ALL_RUNS:
        n = rc.npos(code)
        if code[1] == 1 or R >= n:
            continue
        for orient in (False, True):
            compact, one_bit = _kinds(code, orient)
            assert any(one_bit[2:]) and not all(one_bit[2:])
            if any(one_bit[p] != one_bit[p + R] for p in range(n - R)):
                mixed.add((k, code, orient))
            if any(compact[p] != compact[p + R] for p in range(1, n - R)):
                seen.setdefault(k, set()).add("mid" if label == "mid" else "crossover")
    # (the lazy kernels' even R pairs like with like at rate 3, position 0 of the forward strand aside: hence their rate 5 code)
    assert {(k, c) for k, c, o in mixed if not o} == {(k, c) for k, c in rc.RUNS if c[1] != 1}
    assert {(k, o) for k, _, o in mixed} == {(k, o) for k in rc.ALL_BUT_WIDE for o in (False, True)}
    for k in rc.COMPACT:
        assert rc.plan(k, rc.RATE3[0], 5)["cmp"] == 1
        assert seen.get(k) == {"mid", "crossover"}, (k, seen.get(k))
    assert {k for k in rc.ALL_BUT_WIDE if rc.plan(k, rc.RATE3[0], 5)["cmp"]} == set(rc.COMPACT)
