"""Reading-cost trials without a GPU: the definition in nanopore_dna_storage_amd/trials.py (the order of a trial is a
permutation, depends on seed and trial number, draws uniformly; what a trial reports, on a code small enough to check by
hand, with oracle/rs_oracle.py as the RS decoder), lva_rs_trials' refusals, and the resources of csrc/tr_kernels.hip."""
import os
import re
import subprocess

import numpy as np
import pytest

from nanopore_dna_storage_amd import _lib, trials
from oracle import rs_oracle as RO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
SEED = 20240607            # the uniformity test's constant: a fixed seed makes it deterministic


# ---------------------------------------------------------------- the order of a trial

@pytest.mark.parametrize("n", list(range(1, 71)) + [255, 256, 257, 4097, 10000])
def test_order_is_a_permutation_and_place_its_inverse(n):
    for t in (0, 12345, 2 ** 32 - 1):
        order, place = trials.trial_order(SEED, t, n), trials.trial_place(SEED, t, n)
        assert np.array_equal(np.sort(order), np.arange(n)), (n, t)
        assert np.array_equal(place[order], np.arange(n)), (n, t)


def test_half_bits():
    assert [trials.half_bits(n) for n in (1, 2, 4, 5, 16, 17, 64, 65, 256, 257, 10000, 2 ** 31 - 1)] == [1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 16]


def test_order_depends_on_seed_and_trial():
    a = trials.trial_order(1, 0, 100)
    assert not np.array_equal(a, trials.trial_order(2, 0, 100))
    assert not np.array_equal(a, trials.trial_order(1, 1, 100))
    assert not np.array_equal(a, trials.trial_order(1 + (1 << 32), 0, 100))          # the high word of the seed is part of the key
    assert np.array_equal(a, trials.trial_orders(1, [5, 0], 100)[1])


@pytest.mark.parametrize("n,u", [(6, 3), (37, 12), (100, 40)])
def test_samples_are_uniform(n, u):
    """Over 40 000 trials: the largest |z| of the single-read inclusion frequencies against u / n and of the pair
    co-inclusion frequencies against u (u - 1) / (n (n - 1)), binomial standard deviations.  At most 4 950 roughly normal
    values: a maximum of 5 has a chance of about 0.3 % under uniformity.  (A four-round network gives 13 at n = 6.)"""
    N = 40000
    place = np.concatenate([trials.trial_places(SEED, np.arange(a, a + 5000), n) for a in range(0, N, 5000)])
    inc = (place < u).astype(np.float64)
    assert (inc.sum(axis=1) == u).all()
    p1 = u / n
    z1 = np.abs(inc.mean(axis=0) - p1).max() / np.sqrt(p1 * (1 - p1) / N)
    p2 = u * (u - 1) / (n * (n - 1))
    co = (inc.T @ inc / N)[np.triu_indices(n, 1)]
    z2 = np.abs(co - p2).max() / np.sqrt(p2 * (1 - p2) / N)
    print("n %d u %d: largest |z| single %.2f, pair %.2f" % (n, u, z1, z2))
    assert z1 < 5 and z2 < 5, (z1, z2)


# ---------------------------------------------------------------- a trial, on a tiny code

NO, FEC, BPO, NR = 12, 4, 4, 40


def oracle_decode(reads, redundancy, total, return_ok=False):
    """rs_code.MainDecoder's interface over oracle/rs_oracle.py"""
    oks = []

    def codec(block, erasures):
        ok, out = RO.decode_block(block, redundancy, erasures)
        oks.append(ok)
        return ok, out

    dec = RO.MainDecoder(reads, redundancy, total, codec)
    return (dec, np.array(oks)) if return_ok else dec


@pytest.fixture(scope="module")
def tiny():
    rng = np.random.default_rng(4)
    data = [bytes(rng.integers(0, 256, size=BPO, dtype=np.uint8)) for _ in range(NO - FEC)]
    enc = RO.MainEncoder(data, FEC)
    return dict(enc=np.frombuffer(b"".join(enc), np.uint8).reshape(NO, BPO), original=b"".join(data)[:-2])


def run(tiny, index, reads_to_use, num_trials=3, seed=9, **kw):
    index = np.asarray(index, np.int32)
    payload = tiny["enc"][np.maximum(index, 0)]
    return trials.reference_trials(index, payload, tiny["original"], BPO, FEC, NO, reads_to_use, num_trials, seed,
                                   rs_decode=oracle_decode, **kw)


def test_no_read_used(tiny):
    assert (run(tiny, np.arange(NR) % NO, [0]) == 0).all()


def test_all_reads_clean(tiny):
    got = run(tiny, np.arange(NR) % NO, [NR])
    assert got.shape == (1, 3, 4) and (got == (NR, NO, BPO // 2, 1)).all()


def test_capacity_edge(tiny):
    """exactly num_oligos - redundancy indices: every parity symbol is spent on an erasure; one fewer: refused"""
    assert (run(tiny, np.arange(NR) % (NO - FEC), [NR]) == (NR, NO - FEC, BPO // 2, 1)).all()
    assert (run(tiny, np.arange(NR) % (NO - FEC - 1), [NR]) == (NR, NO - FEC - 1, 0, 0)).all()


def test_nested_samples(tiny):
    """all sample sizes of a trial use one order: passed and present never shrink as the sample grows"""
    index = np.arange(NR) % NO
    index[::5] = -1
    points = [0, 5, 10, 20, 40]
    got, present, payload = run(tiny, index, points, num_trials=6, return_consensus=True)
    assert (np.diff(got[:, :, 0], axis=0) >= 0).all() and (np.diff(got[:, :, 1], axis=0) >= 0).all()
    assert (np.diff(present.astype(int), axis=0) >= 0).all()
    assert (got[-1, :, 0] == (index >= 0).sum()).all() and (got[:, :, 0] <= np.array(points)[:, None]).all()
    assert np.array_equal(present.sum(axis=2), got[:, :, 1])
    assert (payload[present == 1] == np.broadcast_to(tiny["enc"], payload.shape)[present == 1]).all() and (payload[present == 0] == 0).all()
    for j in range(6):                                     # passed, by the definition: the first u of the order that carry an index
        order = trials.trial_order(9, j, NR)
        assert [int((index[order[:u]] >= 0).sum()) for u in points] == got[:, j, 0].tolist()
    assert len({tuple(got[:, j, 0]) for j in range(6)}) > 1          # and the trials differ


def test_first_trial_is_an_offset(tiny):
    index = np.arange(NR) % NO
    index[::3] = -1
    a = run(tiny, index, [8, 16], num_trials=4)
    b = run(tiny, index, [8, 16], num_trials=2, first_trial=2)
    assert np.array_equal(a[:, 2:], b)


# ---------------------------------------------------------------- lva_rs_trials' refusals (no device is touched)

def call(**kw):
    a = dict(device=0, index=np.arange(NR, dtype=np.int32) % NO, payload=np.zeros((NR, BPO), np.uint8), n_reads=NR, bpo=BPO,
             num_oligos=NO, redundancy=FEC, original=np.zeros(30, np.uint8), original_bytes=30,
             reads_to_use=np.array([10, 20], np.int32), n_points=2, seed=1, first_trial=0, n_trials=0, chunk_trials=0,
             out_stats=np.zeros((2, 4, 4), np.int32), out_present=None, out_payload=None)
    a.update(kw)
    ptr = lambda v: None if v is None else v.ctypes.data
    return _lib.load_library().lva_rs_trials(a["device"], ptr(a["index"]), ptr(a["payload"]), a["n_reads"], a["bpo"], a["num_oligos"],
                                             a["redundancy"], ptr(a["original"]), a["original_bytes"], ptr(a["reads_to_use"]),
                                             a["n_points"], a["seed"], a["first_trial"], a["n_trials"], a["chunk_trials"],
                                             ptr(a["out_stats"]), ptr(a["out_present"]), ptr(a["out_payload"]))


def test_no_trials_is_ok():
    assert call() == 0
    assert call(n_reads=0, n_trials=4, index=None, payload=None, reads_to_use=np.zeros(2, np.int32)) == 0


REFUSED = {
    "bytes_per_oligo odd": dict(bpo=5),
    "bytes_per_oligo below 2": dict(bpo=0),
    "num_oligos 0": dict(num_oligos=0),
    "num_oligos above 4096": dict(num_oligos=4097),
    "redundancy 0": dict(redundancy=0),
    "redundancy = num_oligos": dict(redundancy=NO),
    "redundancy above 4096": dict(redundancy=4097),
    "index >= num_oligos": dict(index=np.full(NR, NO, np.int32)),
    "reads_to_use above n_reads": dict(reads_to_use=np.array([10, NR + 1], np.int32)),
    "reads_to_use negative": dict(reads_to_use=np.array([-1, 10], np.int32)),
    "reads_to_use not ascending": dict(reads_to_use=np.array([20, 10], np.int32)),
    "n_points 0": dict(n_points=0),
    "n_points above 64": dict(n_points=65, reads_to_use=np.full(65, 10, np.int32)),
    "trial numbers past 2^32": dict(first_trial=2 ** 32 - 3, n_trials=4),
    "original_bytes 0": dict(original_bytes=0),
    "original_bytes above the data": dict(original=np.zeros(40, np.uint8), original_bytes=(NO - FEC) * BPO + 1),
    "n_reads negative": dict(n_reads=-1),
    "n_trials negative": dict(n_trials=-1),
    "chunk_trials negative": dict(chunk_trials=-1),
    "index NULL": dict(index=None),
    "payload NULL": dict(payload=None),
    "original NULL": dict(original=None),
    "reads_to_use NULL": dict(reads_to_use=None),
    "out_stats NULL": dict(out_stats=None, n_trials=4),
}


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_refusal(what):
    kw = dict(n_trials=4)
    kw.update(REFUSED[what])
    assert call(**kw) == -10, what


def test_trial_numbers_up_to_the_last_are_accepted():
    assert call(first_trial=2 ** 32 - 1, n_trials=0) == 0 and call(first_trial=2 ** 32 - 1, n_trials=2) == -10


def test_python_layer_refuses_before_the_library():
    z = np.zeros((NR, BPO), np.uint8)
    with pytest.raises(ValueError):
        trials.run_trials(np.zeros(NR, np.int32), z, b"x", BPO, FEC, NO, [20, 10], 1, 0)
    with pytest.raises(ValueError):
        trials.run_trials(np.zeros(NR, np.int32), z, b"", BPO, FEC, NO, [10], 1, 0)
    with pytest.raises(_lib.LvaError):
        trials.run_trials(np.full(NR, NO, np.int32), z, b"x", BPO, FEC, NO, [10], 1, 0)


# ---------------------------------------------------------------- the kernels' resources

@pytest.fixture(scope="module")
def meta(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = str(tmp_path_factory.mktemp("asm") / "tr_k.s")
    src = os.path.join(ROOT, "nanopore_dna_storage_amd", "csrc", "tr_kernels.hip")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "--cuda-device-only",
                    "-S", "-o", out, src], check=True, cwd=os.path.dirname(src))
    res = {}
    for b in open(out).read().split("- .agpr_count:")[1:]:
        g = lambda k: re.search(r"\.%s:\s+(\S+)" % k, b).group(1)
        res[g("name")] = dict(vgpr=int(g("vgpr_count")), sgpr=int(g("sgpr_count")), lds=int(g("group_segment_fixed_size")),
                              scratch=int(g("private_segment_fixed_size")))
    return res


def test_no_kernel_uses_scratch(meta):
    names = ("tr_bucket_list", "tr_consensus", "tr_erasures", "rs_trials_kernel", "tr_fold")
    assert len(meta) == len(names), list(meta)
    for kernel in names:
        got = [v for k, v in meta.items() if kernel in k]
        assert len(got) == 1, (kernel, list(meta))
        print(kernel, got[0])
        assert got[0]["scratch"] == 0, (kernel, got[0])
        assert got[0]["vgpr"] <= 128, (kernel, got[0])     # four wavefronts per SIMD stay possible
