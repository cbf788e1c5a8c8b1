"""List sizes 65..256 on the wavefront-per-target kernel (kernel mode 3 above 64 entries: lva_step_wave_wide<R>, R = ceil(L / 64)
register rows per candidate list and for the accepted entries) -- bit for bit the CPU oracle's, the reference's own list
(golden m6_r1_L100) and kernel mode 1's: messages equal, scores equal as uint32.  Every case must really use its last row: at
least one read comes back from the ORACLE with more than 64 (R - 1) entries.
Reference: viterbi/viterbi_convolutional_code.cpp:743-800."""
import numpy as np
import pytest

import nanopore_dna_storage_amd as pkg
from nanopore_dna_storage_amd import synth
from nanopore_dna_storage_amd._lib import LvaError
from golden_util import as_strings, load_case, sync_kw

pytestmark = pytest.mark.gpu

LISTS = (65, 100, 128, 129, 192, 256)


def _rows(L):
    return (L + 63) // 64


def _same(g, wm, ws, what):
    assert not isinstance(g, (int, np.integer)), (what, g)
    assert g[0].shape == wm.shape and np.array_equal(g[0], wm), "%s: list differs" % what
    assert np.array_equal(g[1].view(np.uint32), ws.view(np.uint32)), "%s: scores differ" % what


def _against_oracle(oracle, m, r, msg_len, L, md, reads, threads=8, slots=2, **sync):
    """decode `reads` with kernel mode 3 and compare with the oracle; the oracle's own counts must reach the last register row"""
    kw = {} if md is None else dict(max_deviation=md)
    with pkg.Decoder(m, r, msg_len, list_size=L, kernel=3, max_slots=slots, **kw, **sync) as dec:
        assert dec.profile()["kernel"] == 3
        got = dec.decode([x["post"] for x in reads], rc=[x["rc"] for x in reads])
    counts = []
    for i, (x, g) in enumerate(zip(reads, got)):
        wm, ws = oracle.OracleCode(m, r, msg_len, rc=x["rc"], **sync).decode(x["post"], L, md, num_threads=threads)
        counts.append(len(wm))
        _same(g, wm, ws, "m=%d L=%d md=%r read %d" % (m, L, md, i))
    assert max(counts) > 64 * (_rows(L) - 1), "no read fills row %d of the oracle's list: %r" % (_rows(L) - 1, counts)


def test_golden_L100_through_decoder():
    m, post, lines = load_case("m6_r1_L100")
    with pkg.Decoder(m["mem_conv"], m["rate"], m["msg_len"], list_size=m["list_size"], max_deviation=m["max_deviation"],
                     kernel=3, max_slots=2, **sync_kw(m)) as dec:
        assert dec.profile()["kernel"] == 3
        res = dec.decode([post], rc=[m["rc"]])[0]
    assert len(lines) > 64 and as_strings(res[0]) == lines


def _against_mode_1(m, r, msg_len, L, md, reads):
    """the same against kernel mode 1 (lva_step_exact: one thread per target, shares no merge code with the wavefront paths)"""
    kw = {} if md is None else dict(max_deviation=md)
    posts, rcs = [x["post"] for x in reads], [x["rc"] for x in reads]
    with pkg.Decoder(m, r, msg_len, list_size=L, kernel=3, max_slots=2, **kw) as dec:
        got = dec.decode(posts, rc=rcs)
    with pkg.Decoder(m, r, msg_len, list_size=L, kernel=1, max_slots=2, **kw) as dec:
        assert dec.profile()["kernel"] == 1
        want = dec.decode(posts, rc=rcs)
    for i, (g, w) in enumerate(zip(got, want)):
        _same(g, w[0], w[1], "m=%d L=%d md=%r read %d against kernel mode 1" % (m, L, md, i))
    assert max(len(w[0]) for w in want) > 64 * (_rows(L) - 1)


# The CPU oracle takes 40-60 s for ONE m = 6 read at L = 256 with max_deviation 20 or unbanded (1.5 s at L = 65, max_deviation 6), and
# the GPU suite has a wall-time limit.  So: every list size against the oracle on the narrow band, forward and rc; the wide band and
# the unbanded decode against the oracle at the list sizes it can afford, and at EVERY list size against kernel mode 1.
@pytest.mark.parametrize("L", LISTS)
def test_banded_m6(oracle, L):
    reads = synth.make_reads(6, 1, 60, 3 if L < 192 else 2, seed0=5100 + L, rc_mode="odd", margin=3.0)
    _against_oracle(oracle, 6, 1, 60, L, 6, reads)


@pytest.mark.parametrize("L,md", [(65, 20), (100, 20), (65, None)])
def test_wide_band_and_unbanded_m6_against_oracle(oracle, L, md):
    reads = synth.make_reads(6, 1, 60, 2, seed0=5400 + L, rc_mode="odd", margin=3.0)
    _against_oracle(oracle, 6, 1, 60, L, md, reads)


@pytest.mark.parametrize("md", [20, None])
@pytest.mark.parametrize("L", LISTS)
def test_wide_band_and_unbanded_m6_against_mode_1(L, md):
    reads = synth.make_reads(6, 1, 60, 3, seed0=5400 + L, rc_mode="odd", margin=3.0)
    _against_mode_1(6, 1, 60, L, md, reads)


def test_m8_rate_three_quarters_with_sync_marker(oracle):
    reads = synth.make_reads(8, 3, 50, 2, seed0=5700, rc_mode="odd", margin=4.0)
    _against_oracle(oracle, 8, 3, 50, 100, 6, reads, threads=16, sync_marker="110", sync_period=9)


def test_one_short_m11_read(oracle):
    reads = synth.make_reads(11, 5, 24, 1, seed0=5900, margin=3.0)
    _against_oracle(oracle, 11, 5, 24, 65, 6, reads, threads=16)


def test_four_message_planes_m6(oracle):
    """msg_len + mem_conv > 192 bits: four planes, so that every plane count of the plane layout is crossed along the read"""
    reads = synth.make_reads(6, 1, 200, 1, seed0=6100, margin=3.0)
    _against_oracle(oracle, 6, 1, 200, 129, 6, reads)
    _against_mode_1(6, 1, 200, 256, 6, synth.make_reads(6, 1, 200, 2, seed0=6150, rc_mode="odd", margin=3.0))


@pytest.mark.parametrize("L", [100, 256])
def test_nan_and_plus_inf_posteriors(oracle, L):
    reads = synth.make_reads(6, 1, 60, 3 if L < 192 else 2, seed0=6300 + L, rc_mode="odd", margin=4.0)
    rng = np.random.default_rng(77 + L)
    for i, x in enumerate(reads):
        p = x["post"].copy()
        u = rng.random(p.shape)
        if i != 1:
            p[u < 0.006] = np.nan
        if i != 0:
            p[(u >= 0.006) & (u < 0.012)] = np.inf
        x["post"] = p
    _against_oracle(oracle, 6, 1, 60, L, 6, reads, slots=3)


@pytest.mark.parametrize("L", [100, 256])
def test_tie_dense_posteriors(oracle, L):
    """quantised posteriors: equal scores everywhere, the heap's order decides which entry comes first"""
    reads = synth.make_reads(6, 1, 60, 3 if L < 192 else 2, seed0=6500 + L, rc_mode="odd", margin=3.0, quantum=0.5)
    _against_oracle(oracle, 6, 1, 60, L, 6, reads)


def _drain(st, got):
    while st.outstanding:
        res = st.poll(wait=True)
        assert res
        got.extend(res)


def test_stream_equals_batch_call():
    L = 128
    reads = [synth.make_read(6, 1, 60, 6700 + i, rc=bool(i % 3 == 0), margin=3.0 + (i % 3)) for i in range(10)]
    with pkg.Decoder(6, 1, 60, list_size=L, max_deviation=20, kernel=3, max_slots=3) as dec:
        want = dec.decode([x["post"] for x in reads], rc=[x["rc"] for x in reads])
        assert max(len(w[0]) for w in want) > 64
        for order in (list(range(10)), [7, 2, 9, 0, 5, 3, 8, 1, 6, 4]):
            got = []
            with dec.stream(queue_cap=2) as st:
                for i in order:                      # more reads than slots and queue places: slots are refilled mid-stream
                    while not st.submit(reads[i]["post"], rc=reads[i]["rc"], tag=i):
                        got.extend(st.poll(wait=True))
                    got.extend(st.poll(wait=False))
                _drain(st, got)
            assert sorted(t for t, _ in got) == list(range(10))
            for t, g in got:
                _same(g, want[t][0], want[t][1], "stream order %r read %d" % (order[:3], t))


def test_agrees_with_mode_1_on_refilled_slots():
    L = 192
    reads = [synth.make_read(6, 1, 60, 6900 + i, rc=bool(i & 1), margin=3.0 + (i % 2)) for i in range(7)]
    posts, rcs = [x["post"] for x in reads], [x["rc"] for x in reads]
    posts[3] = posts[3][:-7].copy()              # reads of different lengths: a slot is refilled while the other is mid-read
    with pkg.Decoder(6, 1, 60, list_size=L, max_deviation=20, kernel=3, max_slots=2) as dec:
        assert dec.profile()["kernel"] == 3 and dec.profile()["slots"] == 2
        got = dec.decode(posts, rc=rcs)
    with pkg.Decoder(6, 1, 60, list_size=L, max_deviation=20, kernel=1, max_slots=2) as dec:
        assert dec.profile()["kernel"] == 1
        want = dec.decode(posts, rc=rcs)
    for i, (g, w) in enumerate(zip(got, want)):
        if isinstance(w, (int, np.integer)):
            assert g == w
        else:
            _same(g, w[0], w[1], "read %d against kernel mode 1" % i)
    assert max(len(w[0]) for w in want if not isinstance(w, (int, np.integer))) > 128


@pytest.mark.parametrize("kernel,L", [(3, 257), (2, 100), (4, 100)])
def test_unsupported_combinations(kernel, L):
    with pytest.raises(LvaError) as e:
        pkg.Decoder(6, 1, 60, list_size=L, kernel=kernel, max_slots=2)
    assert e.value.code == -12                   # LVA_ERR_UNSUPPORTED
