"""The read simulator on the device (csrc/sim_kernels.hip, Decoder.simulate) against its definition (simulate.reference_reads):
messages, emitted bases, both offset arrays, the true transition of every block and the scores as uint32 words, with ZERO
differing words -- no tolerance: no draw and no decision involves a floating-point comparison, and a score is three separately
rounded float32 operations on both sides.  Then the chain it feeds: simulate -> posteriors -> decode.

A reference is computed once per argument set and shared; batches smaller than the largest are cut out of it (a read depends
on its number alone: tests/test_simulate_host.py holds the reference to that)."""
import io

import numpy as np
import pytest

import nanopore_dna_storage_amd as pkg
from nanopore_dna_storage_amd import simulate as S, simulator

pytestmark = pytest.mark.gpu

SB, EB = "CACCTGTGCTGCGTCAGGCTGTGTC", "GCTGTCCGTTCCGCATTGACACGGC"
CODES = [(6, 1, 60), (8, 3, 164), (11, 5, 180)]
CHANNELS = {"none": {}, "default": dict(sub=0.002, dele=0.0085, ins=0.0005), "heavy": dict(sub=0.1, dele=0.1, ins=0.1)}
ARG, UNSUPPORTED, BUSY = -10, -12, -13
_REF, _DEC = {}, {}


def _decoder(code, **kw):
    key = (code, tuple(sorted(kw.items())))
    if key not in _DEC:
        _DEC[key] = pkg.Decoder(*code, list_size=kw.pop("list_size", 1), max_deviation=20, **kw)
    return _DEC[key]


def teardown_module(module):
    for d in _DEC.values():
        d.close()
    _DEC.clear()
    _REF.clear()


def _freeze(kw):
    return tuple(sorted((k, v.tobytes() if isinstance(v, np.ndarray) else v) for k, v in kw.items()))


def _reference(code, n, seed, first_read=0, **kw):
    """reference_reads, remembered; a batch inside a remembered larger one of the same arguments is cut out of it"""
    key = (code, seed, _freeze(kw))
    have = _REF.get(key)
    if have is None or not (have[0] <= first_read and first_read + n <= have[0] + have[1]):
        have = (first_read, n, S.reference_reads(*code, n, seed, first_read=first_read, **kw))
        _REF[key] = have
    f0, _, ref = have
    a = first_read - f0
    r0, r1, b0, b1 = ref["row_offsets"][a], ref["row_offsets"][a + n], ref["base_offsets"][a], ref["base_offsets"][a + n]
    return dict(msgs=ref["msgs"][a:a + n], bases=ref["bases"][b0:b1], true_idx=ref["true_idx"][r0:r1], scores=ref["scores"][r0:r1],
                row_offsets=ref["row_offsets"][a:a + n + 1] - r0, base_offsets=ref["base_offsets"][a:a + n + 1] - b0)


def _device(dec, n, seed, first_read=0, **kw):
    with dec.simulate(n, seed, first_read, **kw) as (dev, row, truth):
        scores = np.concatenate(dec.download(dev, row) + [np.zeros((0, 40), np.float32)], axis=0)
    return dict(truth, row_offsets=row, scores=scores)


def _same(got, want):
    for key in ("row_offsets", "base_offsets", "msgs", "bases", "true_idx"):
        assert got[key].shape == want[key].shape and np.array_equal(got[key], want[key]), key
    a, b = np.ascontiguousarray(got["scores"]).view(np.uint32), np.ascontiguousarray(want["scores"]).view(np.uint32)
    assert a.shape == b.shape
    differing = int((a != b).sum())
    if differing:
        t, e = np.argwhere(a != b)[0]
        print("first differing word: block %d entry %d, device %r, reference %r (true transition %d)"
              % (t, e, got["scores"][t, e], want["scores"][t, e], want["true_idx"][t]))
    assert differing == 0, "%d of %d score words differ" % (differing, a.size)


def _check(code, n, seed, first_read=0, **kw):
    got = _device(_decoder(code), n, seed, first_read, **kw)
    _same(got, _reference(code, n, seed, first_read, **kw))
    return got


@pytest.mark.parametrize("n", [130, 1, 63, 64, 65])
@pytest.mark.parametrize("code", CODES)
def test_codes_and_batches(code, n):
    _check(code, n, 21, **CHANNELS["default"])


@pytest.mark.parametrize("channel", ["none", "heavy"])
@pytest.mark.parametrize("code", CODES)
def test_channels(code, channel):
    got = _check(code, 65, 22, **CHANNELS[channel])
    lengths, oligo = np.diff(got["base_offsets"]), pkg.code_info(*code).oligo_len
    if channel == "none":
        assert (lengths == oligo).all()
    else:                                           # insertion runs, reads shorter and longer than the oligo
        assert lengths.min() < oligo < lengths.max()


DWELL = {"no_extra_dwell": np.array([0xFFFFFFFF], np.uint32),            # d = 0 (the one word that is not below: d = 1)
         "one_entry": np.array([1 << 31], np.uint32),                     # d = 0 or 1
         "reaches_K": np.array([1 << 29, 1 << 30, 3 << 29], np.uint32)}   # d = 3 = K for 5 words in 8


@pytest.mark.parametrize("table", sorted(DWELL))
def test_dwell_tables(table):
    got = _check(CODES[0], 65, 23, dwell_cdf=DWELL[table], **CHANNELS["default"])
    blocks, bases = np.diff(got["row_offsets"]), np.diff(got["base_offsets"])
    if table == "no_extra_dwell":
        assert (blocks == bases + 1).all()
    if table == "reaches_K":
        assert blocks.sum() > 65 + 2.5 * bases.sum()


@pytest.mark.parametrize("rc_mode", [0, 1, 2])
def test_barcoded_strands(rc_mode):
    """flanks of 0..120 bases: strands of two to six lane passes beside each other, channel errors in flanks and barcodes too"""
    got = _check(CODES[0], 65, 24 + rc_mode, first_read=3, start_barcode=SB, end_barcode=EB, flank=(0, 120), rc_mode=rc_mode,
                 **CHANNELS["heavy"])
    lengths = np.diff(got["base_offsets"])
    assert lengths.min() < 160 and lengths.max() > 260


def test_long_strand_beside_the_shortest():
    """the longest strand the call accepts (flanks of 256) beside strands without flanks: 1 to 10 lane passes per read"""
    got = _check(CODES[2], 64, 27, start_barcode="ACGT", end_barcode="T", flank=(0, 256), **CHANNELS["default"])
    lengths = np.diff(got["base_offsets"])
    assert lengths.min() < 200 and lengths.max() > 560


def test_a_window_of_a_larger_batch_and_the_same_seed_twice():
    kw = dict(rc_mode=2, **CHANNELS["heavy"])
    big = _device(_decoder(CODES[1]), 20, 31, **kw)
    part = _check(CODES[1], 10, 31, first_read=5, **kw)
    r, b = big["row_offsets"], big["base_offsets"]
    assert np.array_equal(part["msgs"], big["msgs"][5:15]) and np.array_equal(part["bases"], big["bases"][b[5]:b[15]])
    assert np.array_equal(part["true_idx"], big["true_idx"][r[5]:r[15]])
    assert np.array_equal(part["scores"].view(np.uint32), big["scores"][r[5]:r[15]].view(np.uint32))
    again = _device(_decoder(CODES[1]), 10, 31, first_read=5, **kw)
    for key in part:
        assert np.array_equal(np.ascontiguousarray(part[key]).view(np.uint8), np.ascontiguousarray(again[key]).view(np.uint8)), key
    other = _device(_decoder(CODES[1]), 10, 32, first_read=5, **kw)
    assert not np.array_equal(other["msgs"], part["msgs"])


def test_margin_zero_and_a_clip_that_bites():
    got = _check(CODES[0], 33, 33, margin=0.0, clip=2.0, sigma=1.5)
    assert (np.abs(got["scores"]) == 2.0).mean() > 0.05 and float(np.abs(got["scores"]).max()) == 2.0
    _check(CODES[0], 33, 33, margin=2.7, clip=3.1, sigma=0.9)            # margin and scale that a fused multiply-add would round once
    _check(CODES[0], 2, (1 << 63) + 12345, first_read=(1 << 32) - 2)      # the key's high word, the last read numbers


# ---- the chain it feeds -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("list_size", [1, 8])
def test_every_clean_read_decodes_to_its_message(list_size):
    """64 reads of m = 6 r = 1 msg_len 60, seed 7, no channel errors, margin 6.0.  That margin was confirmed without a GPU:
    reference_reads -> tests/transpost_ref.py float64 posteriors -> the CPU oracle returns the true message on top for all
    64 reads at list sizes 1 and 8, so a miss here is the device chain's."""
    dec = _decoder(CODES[0], list_size=list_size)
    truth, results = dec.simulate_and_decode(64, 7, margin=6.0)
    assert np.array_equal(truth["msgs"], _reference(CODES[0], 64, 7, margin=6.0)["msgs"])
    for i, res in enumerate(results):
        assert not isinstance(res, int) and np.array_equal(res[0][0], truth["msgs"][i]), i


def test_barcoded_reads_are_found_and_decoded():
    """16 reads of seed 9 with flanks of 10..40 bases, odd read numbers reverse-complemented, margin 6.0 (confirmed without a
    GPU as above: the oracle's locate_payload finds every window in the right orientation and its decode returns the message)"""
    dec = _decoder(CODES[0])
    truth, results = dec.simulate_and_decode(16, 9, margin=6.0, start_barcode=SB, end_barcode=EB, rc_mode=2)
    for i, (loc, res) in enumerate(results):
        assert loc["ok"] and loc["rc"] == bool(i & 1), (i, loc)
        assert res is not None and not isinstance(res, int) and np.array_equal(res[0][0], truth["msgs"][i]), i


@pytest.mark.parametrize("stats", ["host", "device"])
def test_simulator_synth_device_prints_what_the_reference_reads_give(stats):
    code = CODES[0]
    argv = ["--num_trials", "24", "--mem_conv", "6", "--rate", "1", "--msg_len", "60", "--list_size", "4", "--seed", "5",
            "--margin", "3.0"]
    dec = _decoder(code, list_size=4)
    got = io.StringIO()
    args = simulator.build_parser().parse_args(argv + ["--synth", "device", "--stats", stats])
    got_stats = simulator.run(args, out=got, decoder=dec)
    ref = _reference(code, 24, 5, margin=3.0, **CHANNELS["default"])
    off = ref["row_offsets"]
    results = dec.decode_from_scores([ref["scores"][off[i]:off[i + 1]] for i in range(24)])
    oligos = pkg.encode(*code, ref["msgs"])
    want = io.StringIO()
    want_stats = simulator.report(simulator.build_parser().parse_args(argv), [dict(msg=m, oligo=o) for m, o in zip(ref["msgs"], oligos)],
                                  results, out=want)
    assert got_stats == want_stats and got.getvalue() == want.getvalue()
    assert got_stats["Number total"] == 24 and "Summary statistics:" in got.getvalue()


# ---- refusals -----------------------------------------------------------------------------------------------------------

def _call(dec, fill, n=2, seed=1, first_read=0, thr=(0, 0, 0), cdf="ok", k=None, sb=None, eb=None, flank=(10, 40), rc_mode=0,
          clip=5.0, row="ok", base="ok", scores="ok", msgs="ok", handle="ok"):
    """one call through the C ABI with every output primed -> (status, outputs untouched)"""
    L = dec._L
    table = S.poisson_dwell_cdf()
    primed = np.full(max(n, 0) + 1, 77, np.int64)                            # plan: outputs; fill: some offsets of two reads
    keep = dict(row=np.array([0, 7, 11], np.int64) if fill else primed, base=np.array([0, 3, 5], np.int64) if fill else primed.copy(),
                msgs=np.full((max(n, 1), dec.msg_len), 9, np.uint8))
    before = {key: v.copy() for key, v in keep.items()}
    shared = (dec._h if handle == "ok" else None, seed, first_read, n, *thr, table.ctypes.data if cdf == "ok" else None,
              len(table) if k is None else k, sb, eb, flank[0], flank[1], rc_mode)
    ptr = lambda which, a: a.ctypes.data if which == "ok" else None
    if not fill:
        st = L.lva_simulate_plan(*shared, ptr(row, keep["row"]), ptr(base, keep["base"]))
    else:
        with dec.resident(11 * 160) as (dev, _):
            st = L.lva_simulate_fill_device(*shared, 1.0, 6.0, clip, ptr(row, keep["row"]), ptr(base, keep["base"]),
                                            dev if scores == "ok" else None, ptr(msgs, keep["msgs"]), None, None)
    return st, all(np.array_equal(keep[key], before[key]) for key in keep)


BAD = [("no decoder", dict(handle=None), ARG), ("negative count", dict(n=-1), ARG), ("no dwell table", dict(cdf=None), ARG),
       ("empty dwell table", dict(k=0), ARG), ("dwell table of 65", dict(k=65), ARG), ("rc_mode 3", dict(rc_mode=3), ARG),
       ("substitution above 0.25", dict(thr=((1 << 30) + 1, 0, 0)), ARG), ("deletion above 0.25", dict(thr=(0, 1 << 31, 0)), ARG),
       ("insertion above 0.25", dict(thr=(0, 0, (1 << 30) + 1)), ARG), ("read numbers past 2^32", dict(first_read=(1 << 32) - 1), ARG),
       ("no row offsets", dict(row=None), ARG), ("no base offsets", dict(base=None), ARG),
       ("one barcode", dict(sb=SB.encode()), ARG), ("a barcode with N", dict(sb=b"ACNT", eb=EB.encode()), ARG),
       ("an empty barcode", dict(sb=b"", eb=EB.encode()), ARG), ("a barcode of 65", dict(sb=b"A" * 65, eb=EB.encode()), ARG),
       ("flank range reversed", dict(sb=SB.encode(), eb=EB.encode(), flank=(9, 8)), ARG),
       ("flank above 256", dict(sb=SB.encode(), eb=EB.encode(), flank=(0, 257)), ARG)]
BAD_FILL = [("no score buffer", dict(scores=None), ARG), ("no message buffer", dict(msgs=None), ARG), ("clip 0", dict(clip=0.0), ARG),
            ("clip NaN", dict(clip=float("nan")), ARG)]


@pytest.mark.parametrize("fill", [False, True], ids=["plan", "fill"])
def test_refusals(fill):
    dec = _decoder(CODES[0])
    for what, kw, code in BAD + (BAD_FILL if fill else []):
        st, untouched = _call(dec, fill, **kw)
        assert st == code and untouched, (what, st, untouched)
    # a decoder with a sync marker: lva_encode takes none
    with pkg.Decoder(6, 1, 60, list_size=1, max_deviation=20, sync_marker="110", sync_period=9) as marked:
        st, untouched = _call(marked, fill)
        assert st == UNSUPPORTED and untouched
        assert _call(marked, fill, rc_mode=3)[0] == ARG                     # an argument error wins
    # a busy decoder: own arguments and barcodes are judged first, then the stream
    with dec.stream():
        st, untouched = _call(dec, fill)
        assert st == BUSY and untouched
        assert _call(dec, fill, sb=SB.encode())[0] == ARG and _call(dec, fill, k=0)[0] == ARG
        assert _call(dec, fill, n=0)[0] == BUSY                             # busy before nothing-to-do
    assert _call(dec, fill, n=0)[0] == 0
    assert _call(dec, False)[0] == 0                                        # and the decoder still works


def test_fill_refuses_offsets_that_are_not_the_plan():
    dec = _decoder(CODES[0])
    q = S.parameters()
    cdf = q["cdf"]
    shared = (dec._h, 4, 0, 3, 0, 0, 0, cdf.ctypes.data, len(cdf), None, None, 0, 0, 0)
    row, base = np.zeros(4, np.int64), np.zeros(4, np.int64)
    assert dec._L.lva_simulate_plan(*shared, row.ctypes.data, base.ctypes.data) == 0
    msgs = np.zeros((3, 60), np.uint8)
    wrong = row.copy()
    wrong[2:] -= 1                                                           # read 1 one block short
    with dec.resident(int(row[-1]) * 160) as (dev, _):
        fill = lambda r: dec._L.lva_simulate_fill_device(*shared, float(q["scale"]), 6.0, 5.0, r.ctypes.data, base.ctypes.data, dev,
                                                         msgs.ctypes.data, None, None)
        assert fill(wrong) == ARG
        assert fill(np.array([1, 2, 3, 4], np.int64)) == ARG                 # not offsets at all
        assert fill(row) == 0
        got = np.concatenate(dec.download(dev, row), axis=0)
    assert np.array_equal(got.view(np.uint32), _reference(CODES[0], 3, 4)["scores"].view(np.uint32))
    assert dec.profile()["read_steps"] == int(row[-1])
