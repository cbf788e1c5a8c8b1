"""The pool source of the read simulator on the device (csrc/sim_pool_kernels.hip, Decoder.simulate(pool=...)) against its
definition (simulate.reference_reads(pool=...)): messages, pool entries, orientations, emitted bases, both offset arrays, the true
transition of every block and the scores as uint32 words, with ZERO differing words.  Then what it is for: a file's oligos as
the pool -> reads -> posteriors -> lists -> filter -> consensus / trials -> RS -> the file (helper.simulate_and_decode with
posterior_source="device", roundtrip).

A reference is computed once per argument set and shared; batches smaller than the largest are cut out of it."""
import io

import numpy as np
import pytest

import nanopore_dna_storage_amd as pkg
from nanopore_dna_storage_amd import helper, roundtrip, rs_code, simulate as S, trials
from nanopore_dna_storage_amd.decode_RS_from_decoded_lists import print_curve

pytestmark = pytest.mark.gpu

SB, EB = "CACCTGTGCTGCGTCAGGCTGTGTC", "GCTGTCCGTTCCGCATTGACACGGC"
CODES = [(6, 1, 60), (8, 3, 164), (11, 5, 180)]
DEFAULT, HEAVY = dict(sub=0.002, dele=0.0085, ins=0.0005), dict(sub=0.1, dele=0.1, ins=0.1)
ARG, UNSUPPORTED, BUSY = -10, -12, -13
KEYS = ("row_offsets", "base_offsets", "msgs", "source", "rc", "bases", "true_idx")
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


def _pool(n_pool, msg_len=60):
    """random messages between an all-zero first and an all-one last entry (one entry: random; two: those two)"""
    pool = np.random.default_rng(100 + n_pool).integers(0, 2, size=(n_pool, msg_len), dtype=np.uint8)
    if n_pool > 1:
        pool[0], pool[-1] = 0, 1
    return pool


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
    return dict(msgs=ref["msgs"][a:a + n], source=ref["source"][a:a + n], rc=ref["rc"][a:a + n], bases=ref["bases"][b0:b1],
                true_idx=ref["true_idx"][r0:r1], scores=ref["scores"][r0:r1], row_offsets=ref["row_offsets"][a:a + n + 1] - r0,
                base_offsets=ref["base_offsets"][a:a + n + 1] - b0)


def _device(dec, n, seed, first_read=0, **kw):
    with dec.simulate(n, seed, first_read, **kw) as (dev, row, truth):
        scores = np.concatenate(dec.download(dev, row) + [np.zeros((0, 40), np.float32)], axis=0)
    return dict(truth, row_offsets=row, scores=scores)


def _same(got, want):
    for key in KEYS:
        assert got[key].shape == want[key].shape and got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), key
    a, b = np.ascontiguousarray(got["scores"]).view(np.uint32), np.ascontiguousarray(want["scores"]).view(np.uint32)
    assert a.shape == b.shape
    differing = int((a != b).sum())
    assert differing == 0, "%d of %d score words differ" % (differing, a.size)


def _check(code, n, seed, first_read=0, **kw):
    got = _device(_decoder(code), n, seed, first_read, **kw)
    _same(got, _reference(code, n, seed, first_read, **kw))
    return got


@pytest.mark.parametrize("n", [130, 1, 63, 64, 65])
@pytest.mark.parametrize("n_pool", [1, 2, 3, 65])
def test_pools_and_batches(n_pool, n):
    got = _check(CODES[0], n, 41, pool=_pool(n_pool), rc_mode=3, **DEFAULT)
    if n == 130:
        assert got["rc"].min() == 0 and got["rc"].max() == 1 and len(set(got["source"].tolist())) >= min(n_pool, 3)
    if n_pool == 2:                                   # the all-zero and the all-one message
        assert set(got["msgs"].sum(axis=1).tolist()) <= {0, 60}


def test_first_read_3():
    got = _check(CODES[0], 65, 42, first_read=3, pool=_pool(3), rc_mode=3, **DEFAULT)
    again = _device(_decoder(CODES[0]), 68, 42, pool=_pool(3), rc_mode=3, **DEFAULT)
    assert np.array_equal(got["source"], again["source"][3:]) and np.array_equal(got["rc"], again["rc"][3:])


def test_weighted_with_an_entry_of_weight_zero():
    cdf = S.weights_to_cdf([3, 0, 1, 2, 0])
    got = _check(CODES[0], 130, 43, pool=_pool(5), pool_cdf=cdf, rc_mode=3, **DEFAULT)
    assert set(got["source"].tolist()) == {0, 2, 3}
    wide = S.weights_to_cdf(np.arange(65) % 3)        # a search of seven steps, every third entry never drawn
    got = _check(CODES[0], 130, 43, pool=_pool(65), pool_cdf=wide, **DEFAULT)
    assert (got["source"] % 3 != 0).all() and len(set(got["source"].tolist())) > 30


@pytest.mark.parametrize("rc_mode", [0, 1, 2, 3])
def test_orientation_modes(rc_mode):
    got = _check(CODES[0], 65, 44, first_read=1, pool=_pool(3), rc_mode=rc_mode, **DEFAULT)
    want = [np.zeros(65), np.ones(65), (1 + np.arange(65)) & 1, got["rc"]][rc_mode]
    assert np.array_equal(got["rc"], want.astype(np.uint8))


@pytest.mark.parametrize("rc_mode", [2, 3])
def test_barcoded_with_flanks(rc_mode):
    got = _check(CODES[0], 65, 45, first_read=3, pool=_pool(3), start_barcode=SB, end_barcode=EB, flank=(0, 120), rc_mode=rc_mode,
                 **HEAVY)
    lengths = np.diff(got["base_offsets"])
    assert lengths.min() < 160 and lengths.max() > 260


def test_the_heavy_channel():
    got = _check(CODES[0], 130, 46, pool=_pool(65), rc_mode=3, **HEAVY)
    lengths, oligo = np.diff(got["base_offsets"]), pkg.code_info(*CODES[0]).oligo_len
    assert lengths.min() < oligo < lengths.max()


@pytest.mark.parametrize("code", CODES[1:])
def test_longer_messages(code):
    """msg_len 164 and 180: no multiple of 64, more than two lane passes over the pool entry"""
    pool = _pool(7, code[2])
    got = _check(code, 65, 47, pool=pool, pool_cdf=S.weights_to_cdf([1, 2, 0, 3, 1, 1, 2]), rc_mode=3, **DEFAULT)
    assert np.array_equal(got["msgs"], pool[got["source"]]) and 2 not in got["source"]


def test_a_window_of_a_larger_batch():
    kw = dict(pool=_pool(65), rc_mode=3, **HEAVY)
    big = _device(_decoder(CODES[0]), 130, 46, **kw)
    part = _device(_decoder(CODES[0]), 10, 46, first_read=40, **kw)
    r, b = big["row_offsets"], big["base_offsets"]
    for key in ("msgs", "source", "rc"):
        assert np.array_equal(part[key], big[key][40:50]), key
    assert np.array_equal(part["bases"], big["bases"][b[40]:b[50]]) and np.array_equal(part["true_idx"], big["true_idx"][r[40]:r[50]])
    assert np.array_equal(part["row_offsets"], r[40:51] - r[40]) and np.array_equal(part["base_offsets"], b[40:51] - b[40])
    assert np.array_equal(part["scores"].view(np.uint32), big["scores"][r[40]:r[50]].view(np.uint32))


# ---- refusals through the raw ABI ----------------------------------------------------------------------------------------

def _call(dec, fill, n=2, seed=1, first_read=0, thr=(0, 0, 0), cdf="ok", k=None, sb=None, eb=None, flank=(10, 40), rc_mode=0,
          clip=5.0, row="ok", base="ok", scores="ok", msgs="ok", handle="ok", pool="ok", n_pool=3, pool_cdf=None, pair="pool"):
    """one call through the C ABI with every output primed -> (status, outputs untouched)"""
    L = dec._L
    table = S.poisson_dwell_cdf()
    primed = np.full(max(n, 0) + 1, 77, np.int64)                            # plan: outputs; fill: some offsets of two reads
    keep = dict(row=np.array([0, 7, 11], np.int64) if fill else primed, base=np.array([0, 3, 5], np.int64) if fill else primed.copy(),
                msgs=np.full((max(n, 1), dec.msg_len), 9, np.uint8), source=np.full(max(n, 1), -5, np.int32),
                rc=np.full(max(n, 1), 9, np.uint8))
    before = {key: v.copy() for key, v in keep.items()}
    entries = np.zeros((3, dec.msg_len), np.uint8) if isinstance(pool, str) else pool
    shared = (dec._h if handle == "ok" else None, seed, first_read, n, *thr, table.ctypes.data if cdf == "ok" else None,
              len(table) if k is None else k, sb, eb, flank[0], flank[1], rc_mode)
    if pair == "pool":
        shared += (None if entries is None else entries.ctypes.data, n_pool, None if pool_cdf is None else pool_cdf.ctypes.data)
    ptr = lambda which, a: a.ctypes.data if which == "ok" else None
    if not fill:
        fn = L.lva_simulate_pool_plan if pair == "pool" else L.lva_simulate_plan
        st = fn(*shared, ptr(row, keep["row"]), ptr(base, keep["base"]))
    else:
        fn = L.lva_simulate_pool_fill_device if pair == "pool" else L.lva_simulate_fill_device
        drawn = (keep["source"].ctypes.data, keep["rc"].ctypes.data) if pair == "pool" else ()
        with dec.resident(11 * 160) as (dev, _):
            st = fn(*shared, 1.0, 6.0, clip, ptr(row, keep["row"]), ptr(base, keep["base"]), dev if scores == "ok" else None,
                    ptr(msgs, keep["msgs"]), None, None, *drawn)
    return st, all(np.array_equal(keep[key], before[key]) for key in keep)


def _u32(*v):
    return np.array(v, np.uint32)


TWO = np.array([[0] * 60, [1] * 59 + [2]], np.uint8)
BAD = [("no pool", dict(pool=None), ARG), ("an empty pool", dict(n_pool=0), ARG), ("a negative pool", dict(n_pool=-1), ARG),
       ("a pool above 2^24", dict(n_pool=(1 << 24) + 1), ARG), ("a pool byte above 1", dict(pool=TWO, n_pool=2), ARG),
       ("a table that decreases", dict(pool_cdf=_u32(5, 4, 0xFFFFFFFF)), ARG),
       ("a table that does not end in 0xFFFFFFFF", dict(pool_cdf=_u32(1, 2, 0xFFFFFFFE)), ARG),
       ("rc_mode 4", dict(rc_mode=4), ARG), ("rc_mode -1", dict(rc_mode=-1), ARG),
       ("no decoder", dict(handle=None), ARG), ("negative count", dict(n=-1), ARG), ("no dwell table", dict(cdf=None), ARG),
       ("insertion above 0.25", dict(thr=(0, 0, (1 << 30) + 1)), ARG), ("read numbers past 2^32", dict(first_read=(1 << 32) - 1), ARG),
       ("no row offsets", dict(row=None), ARG), ("no base offsets", dict(base=None), ARG),
       ("one barcode", dict(sb=SB.encode()), ARG), ("flank above 256", dict(sb=SB.encode(), eb=EB.encode(), flank=(0, 257)), ARG)]
BAD_FILL = [("no score buffer", dict(scores=None), ARG), ("no message buffer", dict(msgs=None), ARG), ("clip 0", dict(clip=0.0), ARG)]


@pytest.mark.parametrize("fill", [False, True], ids=["plan", "fill"])
def test_refusals(fill):
    dec = _decoder(CODES[0])
    for what, kw, code in BAD + (BAD_FILL if fill else []):
        st, untouched = _call(dec, fill, **kw)
        assert st == code and untouched, (what, st, untouched)
    # n_pool * msg_len >= 2^31 with n_pool in range needs msg_len >= 128; the pool is refused before a byte of it is read
    st, untouched = _call(_decoder(CODES[2]), fill, n_pool=12_000_000)
    assert 12_000_000 <= 1 << 24 and 12_000_000 * 180 >= 1 << 31 and st == ARG and untouched
    # the pair accepts what it should: rc_mode 3, a table, and a table of equal entries
    assert _call(dec, False, rc_mode=3, pool_cdf=_u32(7, 7, 0xFFFFFFFF))[0] == 0
    # a decoder with a sync marker: lva_encode takes none
    with pkg.Decoder(6, 1, 60, list_size=1, max_deviation=20, sync_marker="110", sync_period=9) as marked:
        st, untouched = _call(marked, fill)
        assert st == UNSUPPORTED and untouched
        assert _call(marked, fill, rc_mode=4)[0] == ARG and _call(marked, fill, pool=None)[0] == ARG     # an argument error wins
        assert _call(marked, fill, pool_cdf=_u32(5, 4, 0xFFFFFFFF))[0] == ARG
    # a busy decoder: own arguments and barcodes are judged first, then the stream
    with dec.stream():
        st, untouched = _call(dec, fill)
        assert st == BUSY and untouched
        assert _call(dec, fill, sb=SB.encode())[0] == ARG and _call(dec, fill, n_pool=0)[0] == ARG
        assert _call(dec, fill, n=0)[0] == BUSY                             # busy before nothing-to-do
    assert _call(dec, fill, n=0)[0] == 0
    # the pair without a pool keeps refusing the coin
    st, untouched = _call(dec, fill, rc_mode=3, pair="plain")
    assert st == ARG and untouched
    assert _call(dec, False)[0] == 0 and _call(dec, False, pair="plain")[0] == 0       # and the decoder still works


def test_fill_reports_what_was_drawn_or_not():
    """source_out and rc_out may each be NULL"""
    dec = _decoder(CODES[0])
    pool, cdf = _pool(3), S.parameters()["cdf"]
    shared = (dec._h, 4, 0, 5, 0, 0, 0, cdf.ctypes.data, len(cdf), None, None, 0, 0, 3, pool.ctypes.data, 3, None)
    row, base = np.zeros(6, np.int64), np.zeros(6, np.int64)
    assert dec._L.lva_simulate_pool_plan(*shared, row.ctypes.data, base.ctypes.data) == 0
    want = _reference(CODES[0], 5, 4, pool=pool, rc_mode=3)
    assert np.array_equal(row, want["row_offsets"])
    msgs, source, rc = np.zeros((5, 60), np.uint8), np.full(5, -1, np.int32), np.full(5, 9, np.uint8)
    with dec.resident(int(row[-1]) * 160) as (dev, _):
        fill = lambda s, r: dec._L.lva_simulate_pool_fill_device(*shared, float(S.score_scale(1.5)), 6.0, 5.0, row.ctypes.data,
                                                                 base.ctypes.data, dev, msgs.ctypes.data, None, None, s, r)
        assert fill(None, None) == 0 and fill(source.ctypes.data, None) == 0 and (rc == 9).all()
        assert fill(None, rc.ctypes.data) == 0
        got = np.concatenate(dec.download(dev, row), axis=0)
    assert np.array_equal(source, want["source"]) and np.array_equal(rc, want["rc"]) and np.array_equal(msgs, want["msgs"])
    assert np.array_equal(got.view(np.uint32), want["scores"].view(np.uint32))


# ---- the chain it feeds -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("list_size", [1, 8])
def test_every_clean_read_decodes_to_its_pool_entry(list_size):
    dec = _decoder(CODES[0], list_size=list_size)
    pool = _pool(65)
    truth, results = dec.simulate_and_decode(64, 7, pool=pool, rc_mode=3, margin=6.0)
    assert truth["rc"].min() == 0 and truth["rc"].max() == 1
    for i, res in enumerate(results):
        assert not isinstance(res, int) and np.array_equal(res[0][0], pool[truth["source"][i]]), i


# A 1 000-byte file in oligos of 18 bytes: 56 data oligos + 16 of the outer code = 72.  NUM_READS and SEED were chosen on the CPU:
# simulate.pool_draws (what reference_reads(pool=..., scores=False) reports as `source`) leaves 2 of the 72 oligos undrawn in
# reads 0..159 under seed 1 -- at most num_oligos_RS = 16 may be missing for the outer code to fill them in.  The test checks it.
FILE_CODE, BYTES_PER_OLIGO, REDUNDANCY, NUM_READS, SEED = CODES[1], 18, 0.3, 160, 1


@pytest.fixture(scope="module")
def stored(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("file")
    data = bytes(np.random.default_rng(5).integers(0, 256, size=1000, dtype=np.uint8))
    path = str(tmp / "data.bin")
    with open(path, "wb") as f:
        f.write(data)
    helper.encode(path, str(tmp / "oligos"), BYTES_PER_OLIGO, REDUNDANCY, FILE_CODE[0], FILE_CODE[1], out=io.StringIO())
    pool = helper.read_conv_input(str(tmp / "oligos.conv_input"))
    assert pool.shape == (72, FILE_CODE[2])
    source = S.reference_reads(*FILE_CODE, NUM_READS, SEED, scores=False, pool=pool, rc_mode=3)["source"]
    assert 72 - len(set(source.tolist())) <= 16                  # the condition on the input, see above
    return dict(tmp=tmp, data=data, path=path, oligos=str(tmp / "oligos"), pool=pool)


def _run(stored, list_size, **channel):
    out = io.StringIO()
    return helper.simulate_and_decode(stored["oligos"], str(stored["tmp"] / "decoded.bin"), NUM_READS, 1000, BYTES_PER_OLIGO, REDUNDANCY,
                                      FILE_CODE[0], FILE_CODE[1], list_size=list_size, seed=SEED, out=out, posterior_source="device",
                                      list_ops="device", decoder=_decoder(FILE_CODE, list_size=list_size), chunk=64, **channel)


def test_a_file_comes_back_from_clean_reads(stored):
    res = _run(stored, 1, syn_sub_prob=0.0, syn_del_prob=0.0, syn_ins_prob=0.0)
    assert res["num_success"] == res["num_attempted"] == NUM_READS and res["data"] == stored["data"]
    with open(str(stored["tmp"] / "decoded.bin"), "rb") as f:
        assert f.read() == stored["data"]


def test_the_default_channel_gives_what_the_host_gives_from_the_definition(stored):
    got = _run(stored, 8)
    ref = S.reference_reads(*FILE_CODE, NUM_READS, SEED, pool=stored["pool"], rc_mode=3, sub=0.005, dele=0.005, ins=0.0005, margin=6.0)
    off = ref["row_offsets"]
    results = _decoder(FILE_CODE, list_size=8).decode_from_scores([ref["scores"][off[i]:off[i + 1]] for i in range(NUM_READS)],
                                                                  rc=ref["rc"].astype(bool))
    seen, num_success = {}, 0                                     # helper.simulate_and_decode's host filter, first payload stands
    for res in results:
        if isinstance(res, (int, np.integer)):
            continue
        index, payload, _ = helper.decode_list_CRC_index(["".join("1" if b else "0" for b in row) for row in res[0]], BYTES_PER_OLIGO,
                                                         72, False)
        if index is not None:
            num_success += 1
            seen.setdefault(index, payload)
    data = b"".join(rs_code.MainDecoder([[k, v] for k, v in seen.items()], 16, 72))[:1000]
    print("num_success %d (device %d), num_unique %d (device %d)" % (num_success, got["num_success"], len(seen), got["num_unique"]))
    assert (got["num_success"], got["num_unique"], got["data"]) == (num_success, len(seen), data)
    assert 0 < num_success <= NUM_READS


def _roundtrip(stored, chunk, extra, out_name):
    argv = ["--data_file", stored["path"], "--bytes_per_oligo", "18", "--RS_redundancy", "0.3", "--mem_conv", "8", "--rate_conv", "3",
            "--list_size", "8", "--num_reads", str(NUM_READS), "--seed", str(SEED), "--chunk", str(chunk),
            "--out", str(stored["tmp"] / out_name)] + extra
    res = roundtrip.main(argv, out=io.StringIO(), decoder=_decoder(FILE_CODE, list_size=8))
    with open(str(stored["tmp"] / out_name), "rb") as f:
        return res, f.read()


def test_roundtrip_recovers_the_file_whatever_the_chunk(stored):
    clean = ["--sub", "0", "--dele", "0", "--ins", "0"]
    a, file_a = _roundtrip(stored, 7, clean, "a.bin")
    b, file_b = _roundtrip(stored, 1000, clean, "b.bin")
    assert file_a == file_b == stored["data"]
    assert np.array_equal(a["index"], b["index"]) and np.array_equal(a["payload"], b["payload"]) and (a["index"] >= 0).all()


def test_roundtrip_trial_table_whatever_the_chunk_and_as_the_definition(stored):
    curve = ["--sub", "0.005", "--dele", "0.005", "--ins", "0.0005", "--num_reads_to_use", "60,110,160", "--num_trials", "5"]
    a, table_a = _roundtrip(stored, 7, curve, "a.txt")
    b, table_b = _roundtrip(stored, 1000, curve, "b.txt")
    assert table_a == table_b and table_a.decode() == a["table"] and np.array_equal(a["stats"], b["stats"])
    assert np.array_equal(a["index"], b["index"]) and np.array_equal(a["payload"], b["payload"])
    want = trials.reference_trials(a["index"], a["payload"], stored["data"], 18, 16, 72, [60, 110, 160], 5, SEED)
    text = io.StringIO()
    print_curve([60, 110, 160], 8, 5, lambda k, t: bool(want[k, t, 3]), text)
    assert np.array_equal(a["stats"], want) and a["table"] == text.getvalue()
    assert a["table"].count("NUM_READS_TO_USE:") == 3
