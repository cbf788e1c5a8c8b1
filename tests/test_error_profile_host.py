"""The error profile (error_profile.py, lva_align_profile, csrc/ep_kernels.hip) without a GPU: the definition on hand-made
cases with the expected arrays written out, its identities on random pairs, the CSV against a literal file, the payload
window against the barcode search it reads backwards, and every refusal of the entry point before a device is looked for."""
import os
import re

import numpy as np
import pytest

import nanopore_dna_storage_amd as pkg
from nanopore_dna_storage_amd import _lib, error_profile as ep, helper

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "ACGTAC"
# rows of pos: a match, a substitution, a deletion, nothing, an inserted base in front, a match with one in front
M, S, D, Z, I, MI = [1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 0], [0, 0, 0, 1], [1, 0, 0, 1]
SAME = [[2, 0, 0, 0, 0, 0], [0, 2, 0, 0, 0, 0], [0, 0, 1, 0, 0, 0], [0, 0, 0, 1, 0, 0]]       # conf of REF read as itself


def one(ref, read, rc=False):
    return ep.reference_profile(read, [[0, len(read)]], [ref], [0], rc=[rc])


def expect(p, read, pos, conf, ins):
    assert p.read.dtype == np.int32 and p.pos.dtype == p.conf.dtype == p.ins.dtype == np.int64
    assert p.read.tolist() == [read] and p.pos.tolist() == pos and p.conf.tolist() == conf and p.ins.tolist() == ins


CASES = {
    "identical": ("ACGTAC", [0, 0, 0, 0], [M, M, M, M, M, M, Z], SAME, [0, 0, 0, 0, 0]),
    "substitution first": ("CCGTAC", [1, 1, 0, 0], [S, M, M, M, M, M, Z],
                           [[1, 1, 0, 0, 0, 0], [0, 2, 0, 0, 0, 0], [0, 0, 1, 0, 0, 0], [0, 0, 0, 1, 0, 0]], [0, 0, 0, 0, 0]),
    "substitution middle": ("ACGAAC", [1, 1, 0, 0], [M, M, M, S, M, M, Z],
                            [[2, 0, 0, 0, 0, 0], [0, 2, 0, 0, 0, 0], [0, 0, 1, 0, 0, 0], [1, 0, 0, 0, 0, 0]], [0, 0, 0, 0, 0]),
    "substitution last": ("ACGTAA", [1, 1, 0, 0], [M, M, M, M, M, S, Z],
                          [[2, 0, 0, 0, 0, 0], [1, 1, 0, 0, 0, 0], [0, 0, 1, 0, 0, 0], [0, 0, 0, 1, 0, 0]], [0, 0, 0, 0, 0]),
    "deletion first": ("CGTAC", [1, 0, 1, 0], [D, M, M, M, M, M, Z],
                       [[1, 0, 0, 0, 0, 1], [0, 2, 0, 0, 0, 0], [0, 0, 1, 0, 0, 0], [0, 0, 0, 1, 0, 0]], [0, 0, 0, 0, 0]),
    "deletion middle": ("ACGAC", [1, 0, 1, 0], [M, M, M, D, M, M, Z],
                        [[2, 0, 0, 0, 0, 0], [0, 2, 0, 0, 0, 0], [0, 0, 1, 0, 0, 0], [0, 0, 0, 0, 0, 1]], [0, 0, 0, 0, 0]),
    "deletion last": ("ACGTA", [1, 0, 1, 0], [M, M, M, M, M, D, Z],
                      [[2, 0, 0, 0, 0, 0], [0, 1, 0, 0, 0, 1], [0, 0, 1, 0, 0, 0], [0, 0, 0, 1, 0, 0]], [0, 0, 0, 0, 0]),
    "insertion first": ("TACGTAC", [1, 0, 0, 1], [MI, M, M, M, M, M, Z], SAME, [0, 0, 0, 1, 0]),
    "insertion middle": ("ACGATAC", [1, 0, 0, 1], [M, M, M, MI, M, M, Z], SAME, [1, 0, 0, 0, 0]),
    "insertion last": ("ACGTACG", [1, 0, 0, 1], [M, M, M, M, M, M, I], SAME, [0, 0, 1, 0, 0]),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_made_case(name):
    read, row, pos, conf, ins = CASES[name]
    expect(one(REF, read), row, pos, conf, ins)
    codes = np.array(["ACGT".index(c) for c in read], np.uint8)                     # lva_encode's codes are the same bases
    assert ep.reference_profile(codes, [[0, len(codes)]], [REF], [0]) == one(REF, read)


def test_the_move_order_places_the_edit_in_a_homopolymer():
    """every placement costs 1; diagonal first from the far end leaves the edit at the near end"""
    expect(one("AAAA", "AAA"), [1, 0, 1, 0], [D, M, M, M, Z], [[3, 0, 0, 0, 0, 1], [0] * 6, [0] * 6, [0] * 6], [0, 0, 0, 0, 0])
    expect(one("AAA", "AAAA"), [1, 0, 0, 1], [MI, M, M, Z], [[3, 0, 0, 0, 0, 0], [0] * 6, [0] * 6, [0] * 6], [1, 0, 0, 0, 0])


def test_an_empty_window_is_all_deletions():
    expect(one("ACGT", ""), [4, 0, 4, 0], [D, D, D, D, Z], [[0, 0, 0, 0, 0, 1], [0, 0, 0, 0, 0, 1], [0, 0, 0, 0, 0, 1], [0, 0, 0, 0, 0, 1]],
           [0, 0, 0, 0, 0])


def test_n_equals_nothing():
    read_n = [[1, 0, 0, 0, 0, 0], [0, 0, 0, 0, 1, 0], [0, 0, 1, 0, 0, 0], [0, 0, 0, 1, 0, 0]]          # C read as N
    expect(one("ACGT", "ANGT"), [1, 1, 0, 0], [M, S, M, M, Z], read_n, [0, 0, 0, 0, 0])
    expect(one("ACGT", "A-GT"), [1, 1, 0, 0], [M, S, M, M, Z], read_n, [0, 0, 0, 0, 0])                 # any other byte is N
    ref_n = [[1, 0, 0, 0, 0, 0], [0] * 6, [0, 0, 1, 0, 0, 0], [0, 0, 0, 1, 0, 0]]                       # no row for the reference N
    expect(one("ANGT", "ACGT"), [1, 1, 0, 0], [M, S, M, M, Z], ref_n, [0, 0, 0, 0, 0])
    expect(one("ANGT", "ANGT"), [1, 1, 0, 0], [M, S, M, M, Z], ref_n, [0, 0, 0, 0, 0])                  # itself included
    expect(one("ANGT", "AGT"), [1, 0, 1, 0], [M, D, M, M, Z], ref_n, [0, 0, 0, 0, 0])
    expect(one("ACGT", "ACNGT"), [1, 0, 0, 1], [M, M, MI, M, Z], [[1, 0, 0, 0, 0, 0], [0, 1, 0, 0, 0, 0], [0, 0, 1, 0, 0, 0], [0, 0, 0, 1, 0, 0]],
           [0, 0, 0, 0, 1])


def test_an_rc_read_against_its_forward_twin():
    for read in ("ACGAAC", "CGTAC", "ACGATAC", "ACNTAC", ""):
        twin = helper.reverse_complement(read)
        assert one(REF, twin, rc=True) == one(REF, read)
    assert one(REF, "GTACGT", rc=True).read.tolist() == [[0, 0, 0, 0]] and one(REF, "GTACGT").read[0, 0] > 0


def test_a_skipped_read_adds_nothing_and_windows_may_overlap():
    buf = "TTACGTACGG"
    p = ep.reference_profile(buf, [[2, 6], [0, 10], [3, 6], [2, 6]], [REF, "CGTACG"], [0, -1, 1, 0])
    assert p.read.tolist() == [[0, 0, 0, 0], [-1, -1, -1, -1], [0, 0, 0, 0], [0, 0, 0, 0]] and p.reads == 3
    with pytest.raises(ValueError):
        ep.reference_profile(buf, [[2, 6]], [REF, "CGTAC"], [0])                      # references of one length
    p = ep.reference_profile(buf, [[2, 6], [0, 10], [2, 6]], [REF], [0, -1, 0])
    assert p.pos.tolist() == [[2, 0, 0, 0]] * 6 + [Z] and p.conf.tolist() == [[2 * v for v in row] for row in SAME]


def random_pair(rng):
    """a reference of 1 .. 80 bases and what a channel with error rates up to 0.2 makes of it"""
    ref = rng.integers(0, 4, rng.integers(1, 81)).astype(np.uint8)
    sub, dele, ins = rng.uniform(0, 0.2, 3)
    read = []
    for b in ref:
        while rng.random() < ins:
            read.append(rng.integers(0, 4))
        if rng.random() < dele:
            continue
        read.append((b + rng.integers(1, 4)) % 4 if rng.random() < sub else b)
    return ref, np.array(read, np.uint8)


def test_identities_on_random_pairs():
    rng = np.random.default_rng(20261020)
    for _ in range(200):
        ref, read = random_pair(rng)
        p = ep.reference_profile(read, [[0, len(read)]], ref[None, :], [0])
        dist, sub, dele, ins = p.read[0].tolist()
        matches = int(p.pos[:, 0].sum())
        assert dist == helper.levenshtein(ref.tolist(), read.tolist())
        assert sub + dele + ins == dist
        assert matches + sub + dele == len(ref)
        assert matches + sub + ins == len(read)
        assert p.pos[:, 1:].sum(axis=0).tolist() == [sub, dele, ins]
        assert p.pos[len(ref), :3].tolist() == [0, 0, 0]
        assert int(p.conf[:, :5].sum()) == matches + sub and int(p.conf[:, 5].sum()) == dele and int(p.ins.sum()) == ins


def test_rates_channel_and_sum():
    rng = np.random.default_rng(3)
    ref = rng.integers(0, 4, 40).astype(np.uint8)
    reads = [random_pair(rng)[1] for _ in range(6)]
    buf = np.concatenate(reads)
    off = np.concatenate([[0], np.cumsum([len(r) for r in reads])])
    win = np.stack([off[:-1], np.diff(off)], axis=1)
    whole = ep.reference_profile(buf, win, ref[None, :], [0] * 6)
    assert ep.reference_profile(buf, win[:2], ref[None, :], [0] * 2) + ep.reference_profile(buf, win[2:], ref[None, :], [0] * 4) == whole
    assert whole.aligned() == 6 * 40
    s, d, i = (int(whole.pos[:, k].sum()) for k in (1, 2, 3))
    assert whole.rates() == dict(sub=s / 240, dele=d / 240, ins=i / 240)
    g = i / (6 * 41)
    assert whole.channel() == dict(sub=s / (240 - d), dele=d / 240, ins=g / (1 + g))


def test_write_csv_against_a_literal_file(tmp_path):
    read = np.array([[1, 1, 0, 0], [-1, -1, -1, -1], [2, 0, 1, 1], [1, 0, 0, 1], [0, 0, 0, 0]], np.int32)       # four reads and a skipped one
    pos = np.array([[3, 1, 0, 0], [3, 0, 1, 1], [0, 0, 0, 1]], np.int64)
    p = ep.ErrorProfile(read, pos, np.zeros((4, 6), np.int64), np.zeros(5, np.int64))
    p.write_csv(str(tmp_path / "run"))
    with open(str(tmp_path / "run.error_stats.csv")) as f:
        text = f.read()
    assert text == ("subs_pos,subs_rate\n0,0.25\n1,0.0\n"
                    "ins_pos,ins_rate\n0,0.0\n1,0.25\n2,0.25\n"
                    "del_pos,del_rate\n0,0.0\n1,0.25\n")


def test_payload_windows_on_a_hand_made_trans_list():
    trans = [2, 5, 9, 12, 15, 20, 26, 30]
    loc = [dict(ok=True, start_pos=8, end_pos=19), dict(ok=False, start_pos=-1, end_pos=-1), dict(ok=True, start_pos=0, end_pos=40),
           dict(ok=True, start_pos=5, end_pos=7), dict(ok=True, start_pos=9, end_pos=11)]
    assert ep.payload_windows([trans] * 5, loc).tolist() == [[2, 4], [0, 0], [0, 8], [0, 0], [3, 1]]


def test_payload_windows_undo_the_barcode_search():
    """helper.find_barcode_pos turns base positions into block positions; payload_windows gives back the payload's bases"""
    rng = np.random.default_rng(5)
    sb, eb = "CACCTGTGCT", "GCATTGACAC"
    for flank5, flank3, n_pay in ((5, 5, 40), (0, 1, 30), (12, 3, 64)):
        draw = lambda k: "".join("ACGT"[x] for x in rng.integers(0, 4, k))
        payload = draw(n_pay)
        call = draw(flank5) + sb + payload + eb + draw(flank3)
        trans = np.cumsum(rng.integers(1, 6, len(call)))
        start, end, ds, de = helper.find_barcode_pos(call, trans, sb, eb)
        assert (ds, de) == (0, 0)
        first, count = ep.payload_windows([trans], [dict(ok=True, start_pos=start, end_pos=end)])[0]
        assert call[first:first + count] == payload


# ---------------------------------------------------------------- lva_align_profile's refusals (no device is touched)

def test_header_library_binding_and_build_carry_the_entry_point():
    with open(os.path.join(ROOT, "include", "lva_decoder.h")) as f:
        header = f.read()
    assert re.search(r"\bint lva_align_profile\(", header) and "#define LVA_ABI_VERSION 5" in header
    assert "lva_align_profile" in _lib.EXPORTS and _lib.load_library().lva_align_profile.argtypes
    with open(os.path.join(ROOT, "nanopore_dna_storage_amd", "csrc", "Makefile")) as f:
        mk = f.read()
    assert re.search(r"^SRC\s*=.*\bep_kernels\.hip\b", mk, re.M) and re.search(r"^HDR\s*=.*\bep_kernels\.h\b", mk, re.M)


NR = 3


def call(**kw):
    a = dict(device=0, bases=np.zeros(8192, np.uint8), first_base=np.zeros(NR, np.int64), n_bases=np.full(NR, 5, np.int32), n_reads=NR,
             refs=np.zeros((2, 6), np.uint8), n_refs=2, ref_len=6, ref_id=np.array([0, 1, -1], np.int32), rc=None, chunk_reads=0,
             out_read=np.zeros((NR, 4), np.int32), out_pos=np.zeros((7, 4), np.int64), out_conf=np.zeros((4, 6), np.int64),
             out_ins=np.zeros(5, np.int64))
    a.update(kw)
    ptr = lambda v: None if v is None else v.ctypes.data
    return _lib.load_library().lva_align_profile(a["device"], ptr(a["bases"]), ptr(a["first_base"]), ptr(a["n_bases"]), a["n_reads"],
                                                 ptr(a["refs"]), a["n_refs"], a["ref_len"], ptr(a["ref_id"]), ptr(a["rc"]),
                                                 a["chunk_reads"], ptr(a["out_read"]), ptr(a["out_pos"]), ptr(a["out_conf"]),
                                                 ptr(a["out_ins"]))


MANY = 1 << 19           # reads of 4096 bases whose lengths sum to 2^31

REFUSED = {
    "ref_len 0": dict(ref_len=0),
    "ref_len above 1024": dict(ref_len=1025, refs=np.zeros((2, 1025), np.uint8)),
    "n_bases negative": dict(n_bases=np.array([5, -1, 5], np.int32)),
    "n_bases above 4096": dict(n_bases=np.array([5, 4097, 5], np.int32)),
    "n_bases above 4096 in a skipped read": dict(n_bases=np.array([5, 5, 4097], np.int32)),
    "n_refs 0": dict(n_refs=0),
    "n_refs * ref_len = 2^31": dict(n_refs=1 << 21, ref_len=1024),
    "ref_id = n_refs": dict(ref_id=np.array([0, 2, -1], np.int32)),
    "first_base negative": dict(first_base=np.array([0, -1, 0], np.int64)),
    "n_bases sum to 2^31": dict(n_reads=MANY, first_base=np.zeros(MANY, np.int64), n_bases=np.full(MANY, 4096, np.int32),
                                ref_id=np.full(MANY, -1, np.int32), out_read=None),
    "n_reads negative": dict(n_reads=-1),
    "chunk_reads negative": dict(chunk_reads=-1),
    "refs NULL": dict(refs=None),
    "refs NULL and no read": dict(refs=None, n_reads=0),
    "bases NULL": dict(bases=None),
    "first_base NULL": dict(first_base=None),
    "n_bases NULL": dict(n_bases=None),
    "ref_id NULL": dict(ref_id=None),
}


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_refusal(what):
    # an ordinal no machine has: a call that passed the checks would answer -11, never run
    assert call(device=1 << 20, **REFUSED[what]) == -10, what


def test_the_limits_themselves_are_accepted_and_then_the_device_is_asked_for():
    """-11 for an ordinal no machine has: the arguments passed; no read succeeds before the device is looked at"""
    nowhere = 1 << 20
    assert call(device=nowhere) == -11
    assert call(device=nowhere, ref_len=1024, refs=np.zeros((2, 1024), np.uint8), out_pos=None) == -11
    assert call(device=nowhere, n_bases=np.array([0, 4096, 4096], np.int32), out_read=None, out_conf=None, out_ins=None) == -11
    assert call(device=nowhere, ref_id=np.array([1, 1, 1], np.int32), rc=np.ones(NR, np.uint8), chunk_reads=1) == -11
    assert call(device=nowhere, n_reads=0) == 0 and call(device=-1, n_reads=0, bases=None, first_base=None, n_bases=None, ref_id=None) == 0
    assert call(device=-1) == -11
    try:                                         # the library's own word on whether device 0 exists
        pkg.Decoder(6, 1, 60).close()
        have_device = True
    except pkg.LvaError as e:
        assert e.code == -11
        have_device = False
    assert call() == (0 if have_device else -11)         # a good small call: without a GPU, LVA_ERR_NO_DEVICE


def test_python_layer_refuses_before_the_library():
    with pytest.raises(ValueError):
        ep.align_profile("ACGT", [[2, 3]], [REF], [0])                # a window past the buffer
    with pytest.raises(ValueError):
        ep.align_profile("ACGT", [[0, 4]], [REF], [1])                # no such reference
    with pytest.raises(ValueError):
        ep.align_profile("ACGT", [[0, 4]], ["A" * 1025], [0])
    with pytest.raises(ValueError):
        ep.align_profile("ACGT", [[0, 4]], [REF], [0, 0])
