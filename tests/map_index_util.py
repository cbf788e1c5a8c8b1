"""What the tests of the read-mapping index share (tests/test_map_index_host.py, tests/test_gpu_map_index.py): read_map's
ReferenceIndex expanded to the direct table that MapIndex.tables() returns, the match masks in numpy, and the sets of oligos
at which an index builder can go wrong.  A case is (oligos, k, max_occ)."""
import numpy as np

from nanopore_dna_storage_amd import read_map as rm
from nanopore_dna_storage_amd.error_profile import _CODE

LETTERS = np.frombuffer(b"ACGT", np.uint8)
RAGGED = lambda k: (1, k - 1, k, k + 1, 63, 64, 65, 127, 128, 129, 1024)


def direct_tables(refs, k, max_occ):
    """-> (offsets uint32 [4^k + 1], lists int32 [pairs], masks uint64 [n, 2, 4, W], info) from the definition"""
    ref = rm.ReferenceIndex(refs, k, max_occ)
    occ = np.zeros(4 ** k + 1, np.int64)
    occ[ref.kmer + 1] = np.diff(ref.off)
    oligos = rm.Oligos(refs)
    W = (int(oligos.lens.max()) + 63) // 64
    masks = np.zeros((len(oligos), 2, 4, W), np.uint64)
    for o in range(len(oligos)):
        codes = _CODE[oligos[o]]
        for r in (0, 1):
            seq = codes[::-1] if r else codes
            for b in range(4):
                pos = np.nonzero(seq == b)[0]
                np.bitwise_or.at(masks[o, r, b], pos >> 6, np.uint64(1) << (pos & 63).astype(np.uint64))
    return np.cumsum(occ).astype(np.uint32), ref.oligo.astype(np.int32), masks, ref.info()


def same_tables(got, want, what=""):
    for name, g, w in zip(("offsets", "lists", "masks"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.dtype, w.shape)
        bad = np.nonzero(g.ravel() != w.ravel())[0]
        assert not len(bad), "%s %s: %d entries differ, the first at %d: got %d want %d" % (what, name, len(bad), bad[0], g.ravel()[bad[0]],
                                                                                           w.ravel()[bad[0]])


def random_oligos(seed, n, m):
    return np.random.default_rng(seed).integers(0, 4, (n, m)).astype(np.uint8)


def ragged(k):
    """one oligo of every length of RAGGED(k): the mask word boundaries, an oligo with no k-mer, one with exactly one"""
    rng = np.random.default_rng(600 + k)
    return [rng.integers(0, 4, m).astype(np.uint8) for m in RAGGED(k)]


def with_n(k, where):
    """five oligos of 5 k + 3 letters with N at `where`: 'first', 'k-1', 'last' or 'every k' (which leaves no k-mer at all)"""
    rng = np.random.default_rng(700 + k)
    m = 5 * k + 3
    at = dict(first=[0], last=[m - 1]).get(where, [k - 1] if where == "k-1" else list(range(k - 1, m, k)))
    out = []
    for _ in range(5):
        o = LETTERS[rng.integers(0, 4, m)].copy()
        o[at] = ord("N")
        out.append(o)
    return out


def shared_prefix(seed=20):
    """2 000 oligos of 100 bases whose first 20 bases are the same: at k = 6 the 15 k-mers of the prefix are held by all"""
    rng = np.random.default_rng(seed)
    refs = rng.integers(0, 4, (2000, 100)).astype(np.uint8)
    refs[:, :20] = refs[0, :20]
    return refs


N_WHERE = ("first", "k-1", "last", "every k")
