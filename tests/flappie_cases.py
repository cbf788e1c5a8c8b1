"""The one list of cases on which the posterior and basecall yardsticks are pinned to the compiled flappie (test
infrastructure): shared by tests/golden/make_flappie_ref.py, which records what oracle/_ref/flappie_decode.out returns
into tests/golden/flappie_ref.npz, and by tests/test_flappie_pin.py / tests/test_gpu_flappie_pin.py, which regenerate
every input from its seed and check its SHA-256 against the record before they compare anything.

SCORE_CASES: [nblk, 40] float32 transition scores.  flappie turns them into posteriors (transpost_crf_flipflop) and
basecalls ITS OWN posteriors (decode_crf_flipflop + change_positions), the order of flappie.c:266-285.
POST_CASES: [nblk, 40] float32 posterior matrices that flappie only basecalls.

Per case `c` the record holds
  c__in_sha      SHA-256 of the input bytes
  c__post        flappie's posteriors, float32 [nblk, 40]                      (score cases of at most STORE_POST_MAX blocks)
  c__post_sha    SHA-256 of flappie's posteriors, c__e_flappie = max |flappie - posteriors_f64| (longer score cases)
  c__path        flappie's state path, int32 [nblk + 1]
  c__score_bits  the bits of its Viterbi score, uint32
  c__chpos       change_positions(path, nblk, .), int32
  c__bases       "ACGT"[path[pos] % 4] at every change position, uint8 (ASCII)
"""
import hashlib
import os

import numpy as np

from nanopore_dna_storage_amd import synth
import transpost_ref as T

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "flappie_ref.npz")
STORE_POST_MAX = 600
UNIFORM_LENGTHS = (1, 2, 3, 4, 5, 8, 17, 63, 64, 65)


def _uniform(n, bound=synth.SCORE_CLIP):
    return np.random.default_rng([9100, n]).uniform(-bound, bound, (n, 40)).astype(np.float32)


def _read_scores():
    """m=8 r=3/4 msg_len 164: about 500 blocks"""
    return synth.make_read_scores(8, 3, 164, 9200, margin=4.5, sub=0.01, dele=0.01, ins=0.01)["scores"]


def _clean_post():
    """a clean read with homopolymer runs: the path alternates flip / flop inside them"""
    rng = np.random.default_rng(9300)
    bases = rng.integers(0, 4, 110).astype(np.uint8)
    bases[10:16] = 2
    bases[40:43] = 0
    bases[80:82] = 3
    return synth.posteriors_from_bases(bases, rng, margin=9.0)


def _holes_post():
    """the same read with -inf at four entries of its best path and eight others (no NaN)"""
    post = _clean_post().copy()
    rng = np.random.default_rng(9301)
    for blk in (7, 60, 61, 300):
        post[blk, int(np.argmax(post[blk]))] = -np.inf
    post[rng.integers(0, post.shape[0], 8), rng.integers(0, 40, 8)] = -np.inf
    assert not np.isnan(post).any()
    return post


SCORE_CASES = dict([("uniform_%d" % n, (lambda n=n: _uniform(n))) for n in UNIFORM_LENGTHS] + [
    ("read", _read_scores),
    ("uniform_3000", lambda: _uniform(3000)),
    ("zeros_9", lambda: np.zeros((9, 40), np.float32)),              # every candidate ties: the first one wins
    ("pm80_33", lambda: _uniform(33, 80.0)),                         # expf(-|d|) underflows
])
POST_CASES = dict([("clean", _clean_post), ("holes", _holes_post)])
ALL_CASES = list(SCORE_CASES) + list(POST_CASES)
UNDERFLOW = "pm80_33"

_inputs = {}


def case_input(name):
    """the case's input matrix, generated once; do not write to it"""
    if name not in _inputs:
        x = np.ascontiguousarray((SCORE_CASES.get(name) or POST_CASES[name])(), dtype=np.float32)
        assert x.ndim == 2 and x.shape[1] == 40 and x.shape[0] >= 1
        x.setflags(write=False)
        _inputs[name] = x
    return _inputs[name]


def sha256(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def stores_post(name):
    return name in SCORE_CASES and case_input(name).shape[0] <= STORE_POST_MAX


def e_against_f64(name, post):
    """max |post - posteriors_f64(the case's scores)|"""
    return float(np.abs(np.asarray(post, np.float64) - f64(name)).max())


_f64 = {}


def f64(name):
    if name not in _f64:
        _f64[name] = T.posteriors_f64(case_input(name))
    return _f64[name]


def record_case(name, O):
    """what the compiled flappie (O = oracle.oracle, O.have_flappie_ref()) returns on one case -> {key: array}"""
    x = case_input(name)
    rec = {name + "__in_sha": np.str_(sha256(x))}
    if name in SCORE_CASES:
        post = O.flappie_transpost(x)
        if stores_post(name):
            rec[name + "__post"] = post
        else:
            rec[name + "__post_sha"] = np.str_(sha256(post))
            rec[name + "__e_flappie"] = np.float64(e_against_f64(name, post))
    else:
        post = x
    bases, chpos, path, score = O.flappie_basecall(post)
    rec[name + "__path"] = path.astype(np.int32)
    rec[name + "__score_bits"] = np.float32(score).reshape(1).view(np.uint32)[0]
    rec[name + "__chpos"] = chpos.astype(np.int32)
    rec[name + "__bases"] = np.frombuffer(bases.encode("ascii"), np.uint8).copy()
    return rec


_fixture = None


def fixture():
    global _fixture
    if _fixture is None:
        with np.load(FIXTURE, allow_pickle=False) as z:
            _fixture = {k: z[k] for k in z.files}
    return _fixture


def checked_input(name):
    """the regenerated input, after its SHA-256 matched the record (a mismatch: regenerate the fixture)"""
    x = case_input(name)
    assert sha256(x) == str(fixture()[name + "__in_sha"]), \
        "%s: the regenerated input differs from the recorded one -- run tests/golden/make_flappie_ref.py" % name
    return x


def recorded_basecall(name):
    """-> (bases str, change positions int64, path int32, score bits) as flappie returned them"""
    fx = fixture()
    return (fx[name + "__bases"].tobytes().decode("ascii"), fx[name + "__chpos"].astype(np.int64), fx[name + "__path"],
            int(fx[name + "__score_bits"]))
