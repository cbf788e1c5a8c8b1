"""The posterior and basecall kernels against flappie's own decode code, from the record of tests/golden/flappie_ref.npz
(what the compiled, unmodified transpost_crf_flipflop / decode_crf_flipflop / change_positions returned on the cases of
tests/flappie_cases.py; tests/test_flappie_pin.py holds the CPU yardsticks to the same record).

Criterion (A').  As criterion (A) of tests/test_gpu_transpost.py, with the compiled flappie's own distance from float64 in
place of the numpy restatement's: for a length class S, E(S) = largest |value - float64 value| over its entries,
  E_gpu(S) <= 2 E_flappie(S)   and   max |float64 log-sum-exp of an output block| <= 2 E_flappie(S)
(device expf / logf are specified to about twice glibc's error).  E_flappie is computed here from the recorded posteriors; the
3000-block case uses its recorded scalar.  Every test prints E_gpu, E_flappie and E_ref.

The basecall kernels are integer and float32 add / compare work: on flappie's recorded posteriors they return flappie's bases,
change positions and counts bit for bit.  Nothing is asserted ACROSS the two: the basecall of the device's posteriors may leave
flappie's at a tie of rounding size; the count is printed."""
import numpy as np
import pytest

import nanopore_dna_storage_amd as pkg
import flappie_cases as C
import transpost_ref as T

pytestmark = pytest.mark.gpu

ACCURACY_CASES = [c for c in C.SCORE_CASES if c != C.UNDERFLOW]
BASECALL_CASES = [c for c in C.ALL_CASES if c in C.POST_CASES or C.stores_post(c)]


@pytest.fixture(scope="module")
def dec():
    with pkg.Decoder(6, 1, 60, list_size=4, max_deviation=20, max_slots=4) as d:
        yield d


def _in_place(dec, scores):
    dev, off = dec.upload(scores)
    try:
        dec.posteriors_resident(dev, off)
        return dec.download(dev, off)
    finally:
        dec.free(dev)


def _e_flappie(name):
    fx = C.fixture()
    return C.e_against_f64(name, fx[name + "__post"]) if C.stores_post(name) else float(fx[name + "__e_flappie"])


def _figures(names, got):
    """per length class -> (class, E_gpu, E_flappie, E_ref, max |logsumexp|), printed"""
    cls = {}
    for name, g in zip(names, got):
        assert g.dtype == np.float32 and g.shape == C.case_input(name).shape
        cls.setdefault(len(g), []).append((name, g))
    out = []
    for n, members in sorted(cls.items()):
        e_gpu = max(C.e_against_f64(name, g) for name, g in members)
        e_fl = max(_e_flappie(name) for name, _ in members)
        e_ref = max(C.e_against_f64(name, T.posteriors_flappie_f32(C.case_input(name))) for name, _ in members)
        lse = max(float(np.abs(np.logaddexp.reduce(g.astype(np.float64), axis=1)).max()) for _, g in members)
        print("%d blocks (%s): E_gpu = %.3g, E_flappie = %.3g, E_ref = %.3g, max |logsumexp| = %.3g"
              % (n, ", ".join(name for name, _ in members), e_gpu, e_fl, e_ref, lse))
        out.append((n, e_gpu, e_fl, e_ref, lse))
    return out


def _hold(names, got):
    failed = [(n, e_gpu, e_fl, lse) for n, e_gpu, e_fl, _, lse in _figures(names, got) if not (e_gpu <= 2 * e_fl and lse <= 2 * e_fl)]
    assert not failed, "(A') fails for (blocks, E_gpu, E_flappie, max |logsumexp|): %r" % failed


def test_posteriors_within_twice_flappies_own_error(dec):
    scores = [C.checked_input(c) for c in ACCURACY_CASES]
    assert sorted(len(s) for s in scores) == sorted(C.UNIFORM_LENGTHS + (9, 3000, len(C.case_input("read"))))
    _hold(ACCURACY_CASES, dec.posteriors(scores))


def test_host_call_and_in_place_call_on_a_short_and_a_read_shaped_case(dec):
    names = ["uniform_5", "read"]
    scores = [C.checked_input(c) for c in names]
    host, inp = dec.posteriors(scores), _in_place(dec, scores)
    _hold(names, host)
    _hold(names, inp)
    assert all(np.array_equal(h, i) for h, i in zip(host, inp))


def test_scores_of_80_stay_finite_and_agree_between_entry_points(dec):
    """No accuracy bound: with scores in +-80 nearly every expf(-|d|) of flappie's folds underflows, a log-sum-exp is its
    largest term, and E_flappie measures the rounding of sums near 33 * 80 (0.00055 here), not an expf or a logf -- a bound
    of twice that says nothing about the kernels' functions.  Held instead: the output is finite wherever flappie's is, and
    the host call and the in-place device call return the same bits.  The three figures are printed."""
    x = C.checked_input(C.UNDERFLOW)
    assert np.abs(x).max() > 70 and len(x) == 33
    host, inp = dec.posteriors([x])[0], _in_place(dec, [x])[0]
    _figures([C.UNDERFLOW], [host])
    flappie = C.fixture()[C.UNDERFLOW + "__post"]
    assert np.isfinite(flappie).any() and np.isfinite(host[np.isfinite(flappie)]).all()
    assert host.tobytes() == inp.tobytes()


def _check_basecalls(names, got):
    assert len(got) == len(names)
    wrong = []
    for name, (bases, trans) in zip(names, got):
        want_bases, want_chpos, _, _ = C.recorded_basecall(name)
        if not (bases == want_bases and len(trans) == len(want_chpos) and np.array_equal(trans, want_chpos)):
            wrong.append(name)
    assert not wrong, "basecalls that differ from flappie's: %r" % wrong


def _flappie_posts():
    """flappie's recorded posteriors of the score cases (their inputs checked against the record) and the two posterior inputs"""
    fx = C.fixture()
    inputs = {c: C.checked_input(c) for c in BASECALL_CASES}
    return [fx[c + "__post"] if c in C.SCORE_CASES else inputs[c] for c in BASECALL_CASES]


def test_basecall_kernels_equal_flappie_on_flappies_posteriors(dec):
    """one batch: the 1- and 2-block reads (nothing to report), the all-tie read and the -inf read beside the 513-block read"""
    posts = _flappie_posts()
    assert {1, 2, 9} <= {len(p) for p in posts} and max(len(p) for p in posts) > 500
    assert any(np.isneginf(p).any() for p in posts) and not any(np.isnan(p).any() for p in posts)
    _check_basecalls(BASECALL_CASES, dec.basecall(posts))
    dev, off = dec.upload(posts)
    try:
        got = dec.basecall_resident(dev, off)
    finally:
        dec.free(dev)
    _check_basecalls(BASECALL_CASES, got)


def test_basecall_of_the_devices_own_posteriors_is_reported_not_asserted(dec):
    """the device's posteriors differ from flappie's by rounding, so a tie of that size may fall the other way"""
    names = [c for c in C.SCORE_CASES if C.stores_post(c)]
    got = dec.basecall(dec.posteriors([C.checked_input(c) for c in names]))
    differ = [c for c, (bases, trans) in zip(names, got)
              if bases != C.recorded_basecall(c)[0] or not np.array_equal(trans, C.recorded_basecall(c)[1])]
    print("basecall of the device's posteriors differs from flappie's basecall of its own in %d of %d cases: %r"
          % (len(differ), len(names), differ))
