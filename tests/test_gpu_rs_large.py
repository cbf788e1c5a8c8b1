"""SURVEY 8(f) row N4 on the GPU beyond one pass per thread: rs_decode_kernel (csrc/rs_kernels.hip) has 256 threads per
codeword and walks its polynomials with `for (k = tid; k < n; k += 256)`.  tests/test_gpu_rs.py stops at 169 parity symbols
and 733 symbols per block; here the redundancy is 300 .. 4096 (several passes of every such loop, the dynamic-LDS opt-in
beyond 48 KB from 1713 on, the limit of 4096), the erasure count crosses 256 and reaches fec + 1, and the block is
unshortened or shortened by one or two symbols (the closed-form padding term and its parity branch).

Every output symbol and every ok flag is compared with the numpy oracle (oracle/rs_oracle.py, pinned to the reference
program at these redundancies by tests/test_rs_oracle.py); equality throughout.  The fill of a failed column (0xFFFF here)
differs from the padding symbol, so that one cannot pass for the other.  The oracle is what costs time (about 10 s for a
word at fec 4096): each distinct word is decoded once (`_ORACLE`), and launches that only reorder columns reuse it.

Columns of one launch share the erasure list (lva_rs_decode), so "refused" (S > fec) is a property of a launch: the mixed
launches hold clean / at capacity / beyond capacity (given up on) / far beyond columns, and with S == fec a column with one
more error, which the decoder cannot tell from a codeword and miscorrects; a refused launch holds clean and corrupted
columns and must fill them all."""
import hashlib

import numpy as np
import pytest

from nanopore_dna_storage_amd import rs_code
from nanopore_dna_storage_amd._lib import load_library
from oracle import rs_oracle as R

pytestmark = pytest.mark.gpu
N = R.N
PAD, FAIL = 0x3030, 0xFFFF
_ORACLE = {}                       # key -> oracle result, for the life of the module


def _memo(key, fn):
    if key not in _ORACLE:
        _ORACLE[key] = fn()
    return _ORACLE[key]


def gpu_decode(cols, fec, erasures, pad=PAD, fail=FAIL):
    """lva_rs_decode on uint16 [columns][n_total] -> (out [columns][n_total - fec], ok [columns])"""
    cols = np.ascontiguousarray(cols, dtype=np.uint16)
    s, n_total = cols.shape
    er = np.ascontiguousarray(erasures, dtype=np.int32)
    out = np.full((s, n_total - fec), 0xABCD, np.uint16)
    ok = np.full(s, -1, np.int32)
    st = load_library().lva_rs_decode(0, cols.ctypes.data, s, n_total, fec, er.ctypes.data if len(er) else None, len(er),
                                      pad, fail, out.ctypes.data, ok.ctypes.data)
    assert st == 0, (st, load_library().lva_rs_last_error())
    return out, ok


def oracle_decode(col, fec, erasures, pad=PAD, fail=FAIL):
    """what lva_rs_decode must return for one column: R.decode_block on the padded block -> (ok, data symbols | fill)"""
    col = np.asarray(col, dtype=np.int64)
    er = [int(e) for e in erasures]
    key = ("dec", fec, pad, fail, hashlib.sha1(col.astype("<u2").tobytes() + np.asarray(er, "<i4").tobytes()).hexdigest())

    def run():
        shift = N - len(col)
        ok, blk = R.decode_block(np.concatenate([np.full(shift, pad, dtype=np.int64), col]), fec, [shift + e for e in er])
        return bool(ok), (blk[shift:N - fec] if ok else np.full(len(col) - fec, fail, dtype=np.int64))

    return _memo(key, run)


def codewords(fec, n_total, count, seed, pad=PAD):
    """`count` distinct codewords of the code shortened to n_total symbols behind padding `pad` -> int64 [count][n_total].
    Two oracle encodes, whatever the count: c = encode(pad .. | d) and z = encode(0 .. | e); the code is linear, so
    c + a z is a codeword with the same padding for every field element a."""
    rng = np.random.default_rng([300, fec, n_total, seed])
    shift = N - n_total
    d, e = rng.integers(0, 65536, size=(2, n_total - fec))
    c = _memo(("enc", fec, n_total, seed, pad), lambda: R.encode_block(np.concatenate([np.full(shift, pad, dtype=np.int64), d]), fec))[shift:]
    z = _memo(("enc0", fec, n_total, seed), lambda: R.encode_block(np.concatenate([np.zeros(shift, dtype=np.int64), e]), fec))[shift:]
    out = np.empty((count, n_total), dtype=np.int64)
    for k in range(count):
        a = int(rng.integers(1, 65536))
        out[k] = c ^ np.array([R.gmul(int(v), a) for v in z], dtype=np.int64)
    assert len({w.tobytes() for w in out}) == count
    return out


def corrupt(word, erasures, n_err, rng, forced=(), garbage=True):
    """erased symbols become random values (or stay, garbage=False); n_err errors at symbols that are NOT erased, `forced` first"""
    rx = word.copy()
    er = np.asarray(erasures, dtype=np.int64)
    if garbage and len(er):
        rx[er] = rng.integers(0, 65536, size=len(er))
    free = np.setdiff1d(np.arange(len(word)), er)
    must = np.array([p for p in forced if p in set(free.tolist())], dtype=np.int64)[:n_err]
    pos = np.concatenate([must, rng.choice(np.setdiff1d(free, must), size=n_err - len(must), replace=False)]).astype(np.int64)
    assert len(set(pos.tolist())) == n_err and not set(pos.tolist()) & set(er.tolist())
    rx[pos] ^= rng.integers(1, 65536, size=n_err)
    return rx


def check_launch(cols, order, fec, erasures, pad=PAD, fail=FAIL):
    """one launch of the columns of `cols` in `order`: every output symbol and every ok flag against the oracle"""
    got, ok = gpu_decode([cols[i] for i in order], fec, erasures, pad, fail)
    for at, i in enumerate(order):
        want_ok, want = oracle_decode(cols[i], fec, erasures, pad, fail)
        assert int(ok[at]) == int(want_ok), (fec, len(erasures), order, at)
        assert np.array_equal(got[at].astype(np.int64), want), (fec, len(erasures), order, at)


def rotations(n):
    return [[(i + r) % n for i in range(n)] for r in range(n)]


@pytest.mark.parametrize("fec,S", [(300, 258), (1712, 600), (1713, 601), (4096, 3000)])
def test_mixed_outcomes_in_one_launch(fec, S):
    """fec 300: two passes of every strided loop; 1712 / 1713: the last size inside 48 KB of LDS and the first that needs the
    opt-in; 4096: the limit.  Columns with different ends in one launch, each of them at the first, a middle and the last
    position: a workgroup that leaves early through finish() must not disturb its neighbours."""
    n_total = fec + (700 if fec < 4096 else 1904)
    cap = (fec - S) // 2
    assert S > 256 and S + 2 * cap == fec
    rng = np.random.default_rng([310, fec])
    er = np.sort(rng.choice(n_total, size=S, replace=False))
    cw = codewords(fec, n_total, 5, seed=1)
    errors_only = corrupt(cw[4], [], fec // 2, rng)              # decoded in a launch of its own: no erasures there
    cols = [cw[0],                                               # clean: the erased symbols hold their true values
            corrupt(cw[1], er, cap, rng, forced=(0, 1, n_total - 1)),      # exactly at capacity
            corrupt(cw[2], er, cap + 1, rng),                    # S + 2E == fec + 2
            corrupt(cw[3], er, min(fec, n_total - S), rng)]      # far beyond
    if fec < 4096:
        cols.append(corrupt(cw[4], er, cap, rng, garbage=False)) # at capacity again, another codeword
    want = [oracle_decode(c, fec, er) for c in cols]
    sent = [np.array_equal(w[1], c[:n_total - fec]) for w, c in zip(want, cw)]
    assert [w[0] and s for w, s in zip(want, sent)][:2] == [True, True] and all(w[0] and s for w, s in zip(want[4:], sent[4:]))
    assert not (want[2][0] and sent[2]) and not (want[3][0] and sent[3])
    assert not want[3][0]                                        # the word far beyond capacity is given up on
    for order in rotations(len(cols)) if fec < 4096 else [[0, 1, 2, 3], [3, 2, 1, 0]]:
        check_launch(cols, order, fec, er)
    check_launch([errors_only, cw[0]], [0, 1], fec, [])          # errors only, floor(fec / 2) of them
    assert oracle_decode(errors_only, fec, [])[0]
    # S == fec + 1: the launch is refused, clean columns included
    er1 = np.sort(rng.choice(n_total, size=fec + 1, replace=False))
    refused = [cw[0], corrupt(cw[1], er1, 0, rng), cw[2]]
    got, ok = gpu_decode(refused, fec, er1)
    assert not ok.any() and (got == FAIL).all()
    check_launch(refused, [0, 1, 2], fec, er1)


@pytest.mark.parametrize("S", [255, 256, 257, 519, 520, 521])
def test_erasure_counts_around_the_workgroup_width_and_the_redundancy(S):
    """fec 520 > 512: S on either side of 256 (the erasure-locator product grows past one pass while it is built) and
    S in {fec - 1, fec, fec + 1}: one Berlekamp-Massey round, none (the locator is the erasure locator), refused."""
    fec, n_total = 520, 800
    rng = np.random.default_rng([320, S])
    er = np.sort(rng.choice(n_total, size=S, replace=False))
    cw = codewords(fec, n_total, 4, seed=2)
    cap = max(fec - S, 0) // 2
    cols = [corrupt(cw[0], er, cap, rng),                        # at capacity
            corrupt(cw[1], er, cap + 1, rng),                    # one error more
            cw[2],                                               # clean
            corrupt(cw[3], er, 0, rng)]                          # erasures only
    want = [oracle_decode(c, fec, er) for c in cols]
    sent = [np.array_equal(w[1], c[:n_total - fec]) for w, c in zip(want, cw)]
    if S <= fec:
        assert want[0][0] and sent[0] and want[2][0] and sent[2] and want[3][0] and sent[3] and not sent[1]
    else:
        assert not any(w[0] for w in want)
    if S == fec:
        assert want[1][0]                                        # the miscorrection: fec erasures leave no check on the result
    for order in ([0, 1, 2, 3], [1, 2, 3, 0], [2, 3, 0, 1]):
        check_launch(cols, order, fec, er)


@pytest.mark.parametrize("n_total", [N, N - 1, N - 2])
def test_padding_edges(n_total):
    """pad = 0 skips the closed-form padding term and has the largest exponents in the syndrome recurrence; pad = 1 and 2
    take the two branches of its i == 0 case.  Errors at symbol 0, symbol 1 and the last symbol; erasures there too."""
    fec = 300
    rng = np.random.default_rng([330, n_total])
    cw = codewords(fec, n_total, 4, seed=3)
    edge = (0, 1, n_total - 1)
    cols = [corrupt(cw[0], [], 150, rng, forced=edge), cw[1], corrupt(cw[2], [], 151, rng, forced=edge),
            corrupt(cw[3], [], 3, rng, forced=edge)]
    want = [oracle_decode(c, fec, []) for c in cols]
    assert [w[0] for w in want] == [True, True, False, True]
    assert all(np.array_equal(want[i][1], cw[i][:n_total - fec]) for i in (0, 1, 3)) and (want[2][1] == FAIL).all()
    for order in ([0, 1, 2, 3], [2, 3, 0, 1]):
        check_launch(cols, order, fec, [])
    er = np.sort(np.concatenate([[0, 1, n_total - 1], 2 + rng.choice(n_total - 3, size=255, replace=False)]))     # S = 258
    cols = [corrupt(cw[0], er, 21, rng, forced=(2, 3, n_total - 2)), corrupt(cw[1], er, 22, rng), cw[2]]
    want = [oracle_decode(c, fec, er) for c in cols]
    assert want[0][0] and np.array_equal(want[0][1], cw[0][:n_total - fec]) and want[2][0]
    assert not (want[1][0] and np.array_equal(want[1][1], cw[1][:n_total - fec]))
    check_launch(cols, [0, 1, 2], fec, er)
    if n_total < N:                                              # a padding symbol of zero contributes nothing
        cz = codewords(fec, n_total, 1, seed=4, pad=0)
        cols = [corrupt(cz[0], [], 150, rng, forced=edge), cz[0]]
        assert oracle_decode(cols[0], fec, [], pad=0)[0]
        check_launch(cols, [0, 1], fec, [], pad=0)


def test_encode_unshortened_block_at_the_largest_redundancy():
    """lva_rs_encode erasure-decodes the S == fec parity symbols: 4096 of them behind 61439 data symbols, no padding.
    Against R.encode_block, and -- without the oracle's encoder -- every syndrome of the result must be zero."""
    fec = 4096
    rng = np.random.default_rng(340)
    data = rng.integers(0, 65536, size=N - fec)
    reads = [int(v).to_bytes(2, "little") for v in data]
    enc = rs_code.MainEncoder(reads, fec)
    assert len(enc) == N and enc[:N - fec] == reads
    got = np.frombuffer(b"".join(enc), dtype="<u2").astype(np.int64)
    want = _memo(("encode_full", fec, 340), lambda: R.encode_block(data, fec))
    assert np.array_equal(got, want)
    assert not R.syndromes(got, fec).any()


def test_main_decoder_and_encoder_mirror_at_two_passes():
    """rs_code.MainEncoder / MainDecoder(return_ok=True) against R.MainEncoder / R.MainDecoder at fec 300 with 270 reads
    missing: the columns of one call end differently (decoded, given up on) and the flags say which."""
    fec, nd, spr = 300, 500, 4
    total = nd + fec
    rng = np.random.default_rng(350)
    reads = [bytes(rng.integers(0, 256, size=2 * spr, dtype=np.uint8)) for _ in range(nd)]
    enc = rs_code.MainEncoder(reads, fec)
    assert enc == _memo(("main_enc", 350), lambda: R.MainEncoder(reads, fec)) and enc[:nd] == reads
    erased = set(rng.choice(total, size=270, replace=False).tolist())
    rx = [[i, enc[i]] for i in range(total) if i not in erased]
    hit = rng.choice(len(rx), size=16, replace=False)                       # 270 + 2 * 15 == fec: column 0 gets 16, the others 15
    for n, j in enumerate(hit):
        b = np.frombuffer(rx[j][1], dtype="<u2").copy()
        where = slice(0, 1) if n == 15 else slice(None)
        b[where] ^= rng.integers(1, 65536, size=len(b[where])).astype(np.uint16)
        rx[j][1] = b.tobytes()
    dec, ok = rs_code.MainDecoder(rx, fec, total, return_ok=True)
    want = _memo(("main_dec", 350), lambda: R.MainDecoder(rx, fec, total))
    assert dec == want
    cols_ok = [all(d[2 * c:2 * c + 2] == r[2 * c:2 * c + 2] for d, r in zip(want, reads)) for c in range(spr)]
    assert cols_ok == [False, True, True, True] and ok.tolist() == cols_ok
    assert all(d[:2] == b"00" for d in dec)                                  # the column given up on: ASCII '0' fill


def test_argument_limits():
    L = load_library()
    sym = np.zeros((1, 4200), np.uint16)
    out = np.zeros((1, 4200), np.uint16)
    ok = np.zeros(1, np.int32)
    args = (None, 0, 0, FAIL, out.ctypes.data, ok.ctypes.data)                                 # padding symbol 0: the all-zero word is a codeword
    assert L.lva_rs_decode(0, sym.ctypes.data, 1, 4200, 4096, *args) == 0 and ok[0] == 1 and not out[0, :104].any()
    assert L.lva_rs_decode(0, sym.ctypes.data, 1, 4200, 4097, *args) == -10                    # LVA_ERR_ARG: beyond the LDS budget
    assert L.lva_rs_decode(0, sym.ctypes.data, 1, 4096, 4096, *args) == -10                    # n_total == fec: no data symbol
    assert L.lva_rs_decode(0, sym.ctypes.data, 1, 300, 300, *args) == -10
    assert L.lva_rs_encode(0, sym.ctypes.data, 1, 10, 4097, PAD, out.ctypes.data) == -10
    assert L.lva_rs_encode(0, sym.ctypes.data, 1, 0, 4096, PAD, out.ctypes.data) == -10
