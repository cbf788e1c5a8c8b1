"""Message widths at the 64-bit plane boundaries, the half that needs no GPU: what tests/boundary_cases.py (the shapes
test_gpu_plane_boundaries.py decodes) covers, the code tables and the encoder at those widths, the kernel plan on both
sides of every plane count, and the refusals at the documented maximum.

nbits[pos] -- the bits a path has consumed on arrival at a trellis position, of which max(1, ceil(nbits / 64)) planes are
moved -- is restated from the block type of every position as the oracle gives it (set_conv_params,
viterbi_convolutional_code.cpp:296-357, the source test_code_tables.py holds the product's tables to)."""
import numpy as np
import pytest

import boundary_cases as bc
import nanopore_dna_storage_amd as pkg
from test_fingerprint_host import plain_fingerprint

MSG_LEN, MSG_TOO_LONG = -3, -7


def _id(code):
    return "m%d-r%d-T%d" % (code[0], code[1], bc.total(code))


def _oracle_nbits(oracle, code, rc):
    oc = oracle.OracleCode(*code, rc=rc)
    nbits = bc.nbits_of([oc.pattern_at(p) for p in range(oc.nstate_pos)])
    assert nbits[-1] == bc.total(code)
    return oc, nbits


# ---- the alignment of every rate, and what the shape list covers -------------------------------------------------

@pytest.mark.parametrize("m", bc.MEMS)
def test_alignment_of_every_rate(oracle, m):
    """forwards the alignment belongs to the rate alone -- rate 1 and the rates 2 and 4 land on every boundary, rate 3 and
    rate 7 step over 128, rate 5 over 64 and 192 -- whatever the memory; the product's tables say the same"""
    want = {1: ("hits", "hits", "hits"), 2: ("hits", "hits", "hits"), 3: ("hits", "over", "hits"), 4: ("hits", "hits", "hits"),
            5: ("over", "hits", "over"), 7: ("hits", "over", "hits")}
    for r in bc.RATES:
        msg_len = max(n for n in range(200 - m, 256 - m) if bc.accepted(m, r, n))       # past the last boundary
        oc, nbits = _oracle_nbits(oracle, (m, r, msg_len), False)
        assert [int(x) for x in oc.pos2msg()] == nbits                                  # forwards nbits is the reference's table
        tab = pkg.code_tables(m, r, msg_len)
        assert bc.nbits_of(tab["ptype"]) == nbits
        assert tuple(bc.alignment(nbits, B) for B in bc.BOUNDARIES) == want[r], r
    for r in set(range(10)) - set(bc.RATES):                                            # RATES is every rate there is
        with pytest.raises(pkg.LvaError):
            pkg.code_info(m, r, 60)


def _alignments(oracle, codes, orientations=(False,)):
    """{boundary: {"hits": [code ids], "over": [...]}} of the codes that pass the boundary or end on it"""
    out = {B: {"hits": [], "over": []} for B in bc.BOUNDARIES}
    for code in codes:
        for rc in orientations:
            _, nbits = _oracle_nbits(oracle, code, rc)
            for B in bc.BOUNDARIES:
                a = bc.alignment(nbits, B)
                if a:
                    out[B][a].append(_id(code) + ("-rc" if rc else ""))
    return out


def test_gpu_shapes_hit_and_step_over_every_boundary_on_every_kernel(oracle):
    """per step kernel (the wide wavefront kernel aside, which runs rate 1 only) the decoded shapes hold, for each of 64, 128
    and 192, a code whose nbits lands on it and a code that carries two bits across it -- in the forward orientation already,
    and every case decodes a reverse complement too"""
    for k in bc.ALL_BUT_WIDE:
        codes = [c for kk, c in bc.RUNS if kk == k]
        al = _alignments(oracle, codes)
        for B in bc.BOUNDARIES:
            assert al[B]["hits"] and al[B]["over"], (k, B, al[B])
        # and each kind both as the very last step of a read and in mid-read: a total that ends on the boundary / one past it
        ends = {bc.total(c) for c in codes}
        assert {64, 128, 192, 256} <= ends and {65, 129, 193} <= ends
        assert {bc.total(c) for c in codes if c[1] != 1 and bc.total(c) in (65, 129, 193)} == {65, 129, 193}   # 63 -> 65 and the like
    wide = [c for kk, c in bc.RUNS if kk == "wide65"]
    assert sorted(bc.total(c) for c in wide) == list(bc.WIDE_TOTALS) and all(c[1] == 1 for c in wide)
    both = _alignments(oracle, bc.STEP_OVER, (False, True))
    assert all(both[B]["hits"] and both[B]["over"] for B in bc.BOUNDARIES)


def test_shape_list_after_filtering():
    """a punctured-rate length that ends inside a two-bit position is refused (LVA_ERR_MSG_LEN) and left out of the list;
    nothing else is: rate 1 keeps every total, the step-over set is not empty, the maximum is reached at m = 6 and m = 8"""
    assert [bc.total(c) for c in bc.RATE1] == list(bc.PLANE_TOTALS) and all(c[:2] == (bc.M, 1) for c in bc.RATE1)
    assert [bc.total(c) for c in bc.WORDS] == list(bc.WORD_TOTALS)
    for code in bc.RATE1 + bc.WORDS + bc.PRODUCTION:
        pkg.code_info(*code)
    assert {c[1] for c in bc.STEP_OVER} == set(bc.STEP_OVER_RATES)
    for r in bc.STEP_OVER_RATES:
        for T in bc.PLANE_TOTALS:
            if (bc.M, r, T - bc.M) not in bc.STEP_OVER:
                with pytest.raises(pkg.LvaError) as e:
                    pkg.code_info(bc.M, r, T - bc.M)
                assert e.value.code == MSG_LEN
    assert {c[0] for c in bc.FULL_ALL} >= {6, 8}
    # as it turns out the maximum is reached at every memory, at the rates 2, 3, 4 and 5 (rate 7 ends on 255 and 257)
    assert sorted(bc.FULL_ALL) == sorted((m, r, 256 - m) for m in bc.MEMS for r in (2, 3, 4, 5))
    assert sorted(bc.FULL_GPU) == [(6, r, 250) for r in (2, 3, 4, 5)]
    assert all(bc.total(c) == 256 and bc.planes(c) == 4 for c in bc.FULL_ALL)
    # every run names a kernel of the table, and every kernel but the wide one sees every plane total, 256 included
    for k in bc.ALL_BUT_WIDE:
        assert {bc.total(c) for kk, c in bc.RUNS if kk == k} >= set(bc.PLANE_TOTALS) | {256}
    assert {k for k, _ in bc.RUNS} == set(bc.KERNELS)
    assert {bc.total(c) for k, c in bc.OVERFLOW_RUNS} == {64, 192}


def test_the_maximum_is_256_bits_and_255_message_bits():
    """msg_len + mem_conv <= 256 and msg_len <= 255 (viterbi_convolutional_code.cpp:604-605, :831): at rate 1 a total of 256
    is one trellis position too many for the code tables; a message of 256 bits is refused by the plan and by
    lva_decoder_create before it looks for a device, at a rate whose tables would hold it"""
    for m in bc.MEMS:
        with pytest.raises(pkg.LvaError) as e:
            pkg.code_info(m, 1, 256 - m)
        assert e.value.code == MSG_TOO_LONG and "256 bits" in str(e.value)
        pkg.code_info(m, 1, 255 - m)
        assert bc.accepted(m, 3, 256)                          # the tables hold it: 256 + m bits in fewer than 256 positions
        for call in (pkg.kernel_plan, pkg.Decoder):
            for r, msg_len in ((1, 256), (3, 256), (3, 256 - m + 3)):      # the last: msg_len <= 255 but more than 256 bits in all
                with pytest.raises(pkg.LvaError) as e:
                    call(m, r, msg_len, list_size=4, max_deviation=bc.MAX_DEV)
                assert e.value.code == MSG_TOO_LONG and "256 bits" in str(e.value), (m, r, msg_len)
        pkg.kernel_plan(m, 3, 256 - m, list_size=4, max_deviation=bc.MAX_DEV)


# ---- the tables at the edge --------------------------------------------------------------------------------------

@pytest.mark.parametrize("code", bc.HOST_CODES, ids=_id)
def test_encoder_and_fingerprint_at_the_boundary_widths(oracle, code):
    m, r, msg_len = code
    rng = np.random.default_rng(1000 * bc.total(code) + 10 * m + r)
    msgs = rng.integers(0, 2, size=(4, msg_len), dtype=np.uint8)
    msgs[2], msgs[3] = 1, 0                                    # every bit set: the oldest bit of the top plane among them
    info = pkg.code_info(*code)
    assert info.msg_words == -(-bc.total(code) // 32) and (info.msg_words + 1) // 2 == bc.planes(code)
    fwd = oracle.OracleCode(*code)
    got = pkg.encode(m, r, msg_len, msgs)
    assert got.shape == (4, info.oligo_len) and info.oligo_len == fwd.nstate_pos - 1
    for msg, oligo in zip(msgs, got):
        assert np.array_equal(oligo, fwd.encode(msg))
    for rc in (False, True):
        oc, nbits = _oracle_nbits(oracle, code, rc)
        tab = pkg.code_tables(m, r, msg_len, rc=rc)
        assert pkg.code_info(m, r, msg_len, rc=rc).nstate_pos == oc.nstate_pos
        assert np.array_equal(tab["pos2msg"], oc.pos2msg())
        assert bc.nbits_of(tab["ptype"]) == nbits
        for msg in msgs:
            assert pkg.code_fingerprint(m, r, msg_len, msg, rc=rc) == plain_fingerprint(m, r, msg_len, msg, msg_len, rc)


# ---- the plan flips where it should --------------------------------------------------------------------------------

PLANES = {63: 1, 64: 1, 65: 2, 127: 2, 128: 2, 129: 3, 191: 3, 192: 3, 193: 4, 255: 4, 256: 4}
WORDS = {96: 3, 97: 4, 160: 5, 161: 6, 224: 7, 225: 8}


def test_planes_and_output_words_at_the_chosen_totals():
    """lva_kernel_plan_info does not carry the plane count; msg_words (32-bit words, code_info) does: P = ceil(msg_words / 2)"""
    for code in bc.RATE1 + bc.STEP_OVER + bc.FULL_ALL:
        assert (pkg.code_info(*code).msg_words + 1) // 2 == PLANES[bc.total(code)] == bc.planes(code)
    assert {bc.total(c) for c in bc.RATE1 + bc.FULL_GPU} == set(PLANES)
    for code in bc.WORDS:
        assert pkg.code_info(*code).msg_words == WORDS[bc.total(code)]
    assert [bc.planes(c) for c in bc.PRODUCTION] == [1, 3]


@pytest.mark.parametrize("request_", [0, 2])
def test_record_layout_exactly_at_three_planes(request_):
    """rec = 1, lva_step_big_rec, no compact lists for 129 <= T <= 192 with L in {32, 36, 64}; the plane layout, lva_step_big and
    compact lists at 128 and 193 and beyond, and for L = 12 and L = 34 everywhere -- at rate 1 for every total from 60 to 255,
    and at every punctured code of the shape list"""
    codes = [(bc.M, 1, T - bc.M) for T in range(60, 256)] + bc.STEP_OVER + bc.FULL_ALL + bc.PRODUCTION
    seen = set()
    for code in codes:
        T = bc.total(code)
        for L in (12, 32, 34, 36, 64):
            plan = pkg.kernel_plan(*code, list_size=L, max_deviation=bc.MAX_DEV, kernel=request_)
            rec = 129 <= T <= 192 and L in (32, 36, 64)
            inst = 16 if L <= 16 else 32 if L <= 32 else 64
            assert plan == dict(mode=2, dominant="big_rec" if rec else "big", fixup="wave", lazy=0, rec=int(rec), cmp=int(not rec),
                                ring_positions=2 * bc.MAX_DEV + 1, instance=inst), (code, L)
            seen.add((T, L, plan["rec"]))
    for T in (128, 193, 255, 256):
        assert (T, 32, 0) in seen and (T, 64, 0) in seen
    for T in (129, 191, 192):
        assert (T, 32, 1) in seen and (T, 36, 1) in seen and (T, 64, 1) in seen and (T, 34, 0) in seen and (T, 12, 0) in seen


@pytest.mark.parametrize("kernel,code", bc.RUNS + bc.PRODUCTION_RUNS, ids=lambda v: v if isinstance(v, str) else _id(v))
def test_every_gpu_run_is_planned_on_the_kernel_it_names(kernel, code):
    request_, L, _ = bc.KERNELS[kernel]
    plan = pkg.kernel_plan(*code, list_size=L, max_deviation=bc.MAX_DEV, kernel=request_)
    assert plan["dominant"] == bc.dominant(kernel, code)
    if kernel == "big32":
        assert (plan["dominant"] == "big_rec") == (bc.total(code) in (129, 191, 192)) == bool(plan["rec"])
