"""The posterior and basecall yardsticks against flappie's own decode code (CPU).

tests/golden/flappie_ref.npz holds what the compiled, unmodified decode path of the reference's flappie
(oracle/_ref/flappie_decode.out: transpost_crf_flipflop, decode_crf_flipflop, change_positions behind a driver of our own)
returned on the cases of tests/flappie_cases.py.  Every test regenerates its input from the seed and holds its SHA-256
to the record first.

  1. the binary, where oracle/_ref has it, returns the record bit for bit;
  2. oracle/basecall_oracle.c (bc_oracle_basecall, through oracle.basecall) on flappie's posteriors returns flappie's path,
     score bits, change positions and bases bit for bit;
  3. tests/transpost_ref.py::posteriors_flappie_f32 is as far from float64 as flappie is: with E = largest
     |value - float64 value| over a case, E_ref <= 1.05 E_flappie and E_flappie <= 1.05 E_ref, and the restatement lies
     within E_flappie of flappie.  Both are the same float32 operation sequence and differ in numpy's against glibc's
     expf / log1pf only: measured ratios 1.000 ... 1.001, so 5 % would mean another operation order.
     Bit-equality was seen on short reads and is not asserted.  posteriors_scaled_f32 is not flappie's order and is not compared.
"""
import numpy as np
import pytest

import flappie_cases as C
import transpost_ref as T


def _live_post(oracle, name):
    """flappie's posteriors of a score case: the record, or for a case recorded as SHA-256 the binary's, checked against it"""
    fx = C.fixture()
    x = C.checked_input(name)
    if C.stores_post(name):
        return fx[name + "__post"]
    if not oracle.have_flappie_ref():
        pytest.skip("oracle/_ref/flappie_decode.out absent: the posteriors of %s are recorded as SHA-256 only" % name)
    post = oracle.flappie_transpost(x)
    assert C.sha256(post) == str(fx[name + "__post_sha"])
    return post


@pytest.mark.parametrize("name", C.ALL_CASES)
def test_the_binary_returns_the_record(oracle, name):
    C.checked_input(name)
    if not oracle.have_flappie_ref():
        pytest.skip("oracle/_ref/flappie_decode.out absent (built where the reference tree is)")
    fx = C.fixture()
    live = C.record_case(name, oracle)
    assert sorted(live) == sorted(k for k in fx if k.startswith(name + "__"))
    for k, v in live.items():
        v = np.asarray(v)
        assert v.dtype == fx[k].dtype and v.shape == fx[k].shape, k
        assert v.tobytes() == fx[k].tobytes(), k


def test_the_record_holds_every_case_and_nothing_else():
    fx = C.fixture()
    assert {k.split("__")[0] for k in fx} == set(C.ALL_CASES)
    for name in C.ALL_CASES:
        n = C.case_input(name).shape[0]
        assert fx[name + "__path"].shape == (n + 1,) and fx[name + "__path"].dtype == np.int32
        assert len(fx[name + "__chpos"]) == len(fx[name + "__bases"])
        if name in C.SCORE_CASES:
            assert (name + "__post" in fx) == C.stores_post(name) and (name + "__e_flappie" in fx) != C.stores_post(name)
    assert not C.stores_post("uniform_3000") and C.stores_post("read")


@pytest.mark.parametrize("name", C.ALL_CASES)
def test_basecall_oracle_equals_flappie(oracle, name):
    post = _live_post(oracle, name) if name in C.SCORE_CASES else C.checked_input(name)
    want_bases, want_chpos, want_path, want_bits = C.recorded_basecall(name)
    bases, trans, path, score = oracle.basecall(post)
    assert np.array_equal(path, want_path)
    assert int(np.float32(score).reshape(1).view(np.uint32)[0]) == want_bits
    assert np.array_equal(trans, want_chpos)
    assert bases == want_bases


def test_what_the_basecall_cases_cover():
    """the properties the cases were chosen for, read off flappie's record"""
    for name in ("uniform_1", "uniform_2"):                     # change_positions(path, nblk, .) looks at path[1 .. nblk-1] only
        assert C.recorded_basecall(name)[0] == ""
    bases, chpos, path, bits = C.recorded_basecall("zeros_9")
    assert bases == "" and len(chpos) == 0 and not path.any()   # strict '>': the first candidate wins every tie
    assert np.uint32(bits).view(np.float32) < 0                 # 9 blocks of log(1/40)
    bases, _, path, _ = C.recorded_basecall("clean")
    assert "GGGGGG" in bases and (path >= 4).any()              # a homopolymer run, called through flop states
    holes = C.checked_input("holes")
    assert np.isneginf(holes).sum() >= 10 and not np.isnan(holes).any()
    assert C.recorded_basecall("holes")[0] != bases             # the -inf entries moved the path
    assert len(C.recorded_basecall("uniform_3000")[0]) > 2000


@pytest.mark.parametrize("name", list(C.SCORE_CASES))
def test_posterior_yardstick_equals_flappie(oracle, name):
    fx = C.fixture()
    x = C.checked_input(name)
    ref = T.posteriors_flappie_f32(x)
    e_ref = C.e_against_f64(name, ref)
    if C.stores_post(name):
        post = fx[name + "__post"]
        e_flappie = C.e_against_f64(name, post)
    else:
        e_flappie = float(fx[name + "__e_flappie"])
        post = oracle.flappie_transpost(x) if oracle.have_flappie_ref() else None
        if post is not None:
            assert C.sha256(post) == str(fx[name + "__post_sha"]) and C.e_against_f64(name, post) == e_flappie
    line = "%-13s %5d blocks: E_flappie = %.4g, E_ref = %.4g, E_ref / E_flappie = %.4f" % (name, len(x), e_flappie, e_ref, e_ref / e_flappie)
    if post is not None:
        d = np.abs(ref.astype(np.float64) - post.astype(np.float64))
        line += ", %d of %d entries differ, by at most %.3g" % (int((ref.view(np.uint32) != post.view(np.uint32)).sum()), post.size, d.max())
    else:
        line += ", posteriors recorded as SHA-256: entries not compared"
    print(line)
    assert e_ref <= 1.05 * e_flappie, line
    assert e_flappie <= 1.05 * e_ref, line
    if post is not None:
        assert np.array_equal(np.isfinite(ref), np.isfinite(post))
        assert d.max() <= e_flappie, line
