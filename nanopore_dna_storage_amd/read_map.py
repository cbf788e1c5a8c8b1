"""Reads mapped to oligos: which oligo a read came from, on which strand, and where in the read it
lies -- for reads that carry no index of their own.  The reference does it with minimap2 (util/align_compute_stats.sh:21-33
maps every basecall against merged.fa, splits the reads by experiment, counts the mapped ones and feeds samtools stats).  No
agreement with minimap2 is claimed: this file is the project's own exact definition in numpy / Python (reference_map) and the
call into the device path (lva_map_reads, csrc/mp_kernels.hip), which is held to it bit for bit (tests/test_gpu_read_map.py).

The definition.  Bytes are read as error_profile reads them: A C G T or 0 1 2 3 are bases, anything else is N and equals
nothing.  Parameters: k (6..12, 10), max_occ (1..65535, 64), cands (1..8, 4), min_votes (>= 1, 2), max_dist (>= 0, ref_len // 4).

  index    the set of distinct pairs (k-mer, oligo) over every oligo and every position 0 .. ref_len - k whose k bases are all
           bases; a k-mer is coded at 2 bits per base, first base most significant.  occ(k-mer) is the number of distinct
           oligos that hold it; every pair whose k-mer has occ > max_occ is dropped (a barcode or homopolymer k-mer shared by
           a whole experiment votes for nobody).  ref_len < k: an empty index, nothing maps.
  votes    strand 0 of a read is its window as given, strand 1 the reverse complement (N stays N).  votes[s][o] is the number
           of positions of the oriented window whose k-mer (no N in it) is paired with o.
  cands    the pairs (s, o) with votes >= min_votes, ordered by (votes descending, strand, oligo); the first `cands` are kept.
  dist     D is the unit-cost matrix of the oligo (rows 0 .. m) against the oriented window x (columns 0 .. n) with
           D[i][0] = i and D[0][j] = 0: the oligo is taken whole, the read's ends are free.  d = min_j D[m][j], e the smallest
           j that attains it.
  winner   the candidate with the smallest (d, place in the candidate order); second is the smallest d among candidates whose
           oligo differs from the winner's, -1 if there is none.
  start    for the winner only: E is the matrix of the reversed oligo against x[0:e] reversed, E[i][0] = i, E[0][j] = j;
           j' is the smallest j with E[m][j] == d (one exists), s = e - j'.  In the coordinates of the window as given the
           aligned part is [s, e) on strand 0 and [n - e, n - s) on strand 1.

Result: out int32 [n, 8] = (ref, best, rc, dist, start, count, votes, second); best is the winner's oligo, ref is best if
dist <= max_dist and -1 otherwise; a read without a candidate (an empty window, n < k, nothing reaches min_votes) is
(-1, -1, 0, -1, 0, 0, 0, -1).  The global distance of x[s:e] to the oligo is d, so
align_profile(bases, res.windows(w), refs, res.ref, res.rc).read[:, 0] == res.dist for every mapped read.

Out of scope: oligo sets of unequal length, chimeric or secondary alignments (the reference drops them with -F 256 and SA:Z:),
an index built on the device."""
import argparse
import ctypes
import sys

import numpy as np

from ._lib import check, load_library
from .error_profile import MAX_READ, MAX_REF, N, _CODE, _arguments

VOTE_RANGE = 4096         # kMpVoteRange of csrc/mp_kernels.h: oligos whose votes one pass of mp_vote counts
K_RANGE = (6, 12)
MAX_CANDS = 8
FIELDS = ("ref", "best", "rc", "dist", "start", "count", "votes", "second")
UNMAPPED = (-1, -1, 0, -1, 0, 0, 0, -1)


def _parameters(ref_len, k, max_occ, cands, min_votes, max_dist):
    if max_dist is None:
        max_dist = ref_len // 4
    if not (K_RANGE[0] <= k <= K_RANGE[1] and 1 <= max_occ <= 65535 and 1 <= cands <= MAX_CANDS and min_votes >= 1 and max_dist >= 0):
        raise ValueError("6 <= k <= 12, 1 <= max_occ <= 65535, 1 <= cands <= 8, min_votes >= 1, max_dist >= 0")
    return int(max_dist)


def _inputs(bases, windows, refs):
    windows = np.ascontiguousarray(windows, dtype=np.int64).reshape(-1, 2)
    bases, windows, refs, _, _ = _arguments(bases, windows, refs, np.zeros(len(windows), np.int32), None)
    return bases, windows, refs


def _kmers(codes, k):
    """the k-mer code of every position of a code array, and whether its k bases are all bases"""
    n = max(len(codes) - k + 1, 0)
    kmer, ok = np.zeros(n, np.int64), np.ones(n, bool)
    for i in range(k if n else 0):
        c = codes[i:i + n]
        kmer = (kmer << 2) | (c & 3)
        ok &= c < N
    return kmer, ok


def _reverse_complement(codes):
    return np.where(codes < N, 3 - codes, N).astype(np.uint8)[::-1]


class ReferenceIndex:
    """the index of the definition: kmer (kept, ascending), off [len(kmer) + 1], oligo (ascending inside a k-mer), dropped"""

    def __init__(self, refs, k, max_occ):
        codes = _CODE[refs]
        parts = []
        for o, row in enumerate(codes):
            kmer, ok = _kmers(row, k)
            parts.append((np.unique(kmer[ok]) << 32) | o)
        pairs = np.unique(np.concatenate(parts + [np.zeros(0, np.int64)]))
        kmer, occ = np.unique(pairs >> 32, return_counts=True)
        keep = occ <= max_occ
        self.n_refs, self.k = len(refs), k
        self.kmer = kmer[keep]
        self.oligo = (pairs & 0xFFFFFFFF)[np.repeat(keep, occ)]
        self.off = np.concatenate([[0], np.cumsum(occ[keep])]).astype(np.int64)
        self.dropped = int((~keep).sum())

    def info(self):
        """(kept distinct k-mers, kept pairs, k-mers dropped by max_occ): what lva_map_index_info reports"""
        return len(self.kmer), len(self.oligo), self.dropped

    def votes(self, codes):
        """int64 [n_refs]: per oligo the positions of the code array whose k-mer it holds"""
        kmer, ok = _kmers(codes, self.k)
        q = kmer[ok]
        at = np.searchsorted(self.kmer, q)
        hit = at < len(self.kmer)
        hit[hit] = self.kmer[at[hit]] == q[hit]
        lo, cnt = self.off[at[hit]], self.off[at[hit] + 1] - self.off[at[hit]]
        where = np.repeat(lo - (np.cumsum(cnt) - cnt), cnt) + np.arange(int(cnt.sum()))       # every list, one after the other
        return np.bincount(self.oligo[where.astype(np.int64)], minlength=self.n_refs)


def _last_row(ref, x, top):
    """row len(ref) of the unit-cost matrix of ref (rows) against x (columns) with D[0] = top and D[i][0] = i; a row at a
    time as error_profile._distance_matrix: D[i][j] - j is the running minimum of t[j] - j, t the other two moves"""
    n = len(x)
    j = np.arange(n + 1, dtype=np.int64)
    row = np.asarray(top, dtype=np.int64)
    for i in range(1, len(ref) + 1):
        t = np.empty(n + 1, np.int64)
        t[0] = i
        cost = (x != ref[i - 1]) | (x == N)
        np.minimum(row[1:] + 1, row[:-1] + cost, out=t[1:])
        row = np.minimum.accumulate(t - j) + j
    return row


def end_distance(ref, x):
    """(d, e) of the definition: the oligo whole, the read's ends free"""
    row = _last_row(ref, x, np.zeros(len(x) + 1, np.int64))
    e = int(np.argmin(row))
    return int(row[e]), e


def start_row(ref, x, e):
    """row m of E: the reversed oligo against x[0:e] reversed, anchored at e"""
    return _last_row(ref[::-1], x[:e][::-1], np.arange(e + 1))


class MapResult:
    """out int32 [n, 8] = (ref, best, rc, dist, start, count, votes, second) (the module's docstring); a column by its name"""

    def __init__(self, out):
        self.out = out

    def __getattr__(self, name):
        if name in FIELDS:
            return self.out[:, FIELDS.index(name)]
        raise AttributeError(name)

    def __len__(self):
        return len(self.out)

    @property
    def mapped(self):
        return int((self.ref >= 0).sum())

    def windows(self, windows):
        """the aligned part of every read in the buffer's coordinates -> int64 [n, 2] = (first base, count), count 0 where
        the read is not mapped: with ref and rc the arguments of error_profile.align_profile"""
        w = np.ascontiguousarray(windows, dtype=np.int64).reshape(-1, 2)
        ok = self.ref >= 0
        return np.stack([w[:, 0] + np.where(ok, self.start, 0), np.where(ok, self.count, 0)], axis=1).astype(np.int64)

    def coverage(self, n_refs):
        """int64 [n_refs, 2]: mapped reads per oligo, forward and reverse; a row's sum is a weight for simulate.weights_to_cdf"""
        ok = self.ref >= 0
        return np.stack([np.bincount(self.ref[ok & (self.rc == s)], minlength=n_refs) for s in (0, 1)], axis=1).astype(np.int64)


def reference_map(bases, windows, refs, k=10, max_occ=64, cands=4, min_votes=2, max_dist=None):
    """The definition (the module's docstring), a read at a time.  bases, windows [n, 2], refs [n_refs, ref_len] as
    error_profile.reference_profile takes them.  -> MapResult"""
    bases, windows, refs = _inputs(bases, windows, refs)
    m = refs.shape[1]
    max_dist = _parameters(m, k, max_occ, cands, min_votes, max_dist)
    index = ReferenceIndex(refs, k, max_occ)
    codes = _CODE[refs]
    out = np.empty((len(windows), 8), np.int32)
    out[:] = UNMAPPED
    for r, (first, count) in enumerate(windows):
        x = _CODE[bases[first:first + count]]
        strands = (x, _reverse_complement(x))
        found = []
        for s in (0, 1):
            v = index.votes(strands[s])
            found += [(-int(v[o]), s, int(o)) for o in np.nonzero(v >= min_votes)[0]]
        found = sorted(found)[:cands]
        if not found:
            continue
        dist = [end_distance(codes[o], strands[s]) for _, s, o in found]
        place = min(range(len(found)), key=lambda c: (dist[c][0], c))
        (d, e), (v, s, o) = dist[place], found[place]
        others = [dist[c][0] for c in range(len(found)) if found[c][2] != o]
        E = start_row(codes[o], strands[s], e)
        assert E.min() == d, "the anchored pass attains the distance"
        jp = int(np.argmax(E == d))
        start = e - jp
        out[r] = (o if d <= max_dist else -1, o, s, d, start if s == 0 else int(count) - e, jp, -v, min(others) if others else -1)
    return MapResult(out)


class MapIndex:
    """The index of a set of equally long oligos (lva_map_index_create: the k-mer table and the oligos' match masks, built on
    the host); owns the handle, a context manager.  refs: [n_refs, ref_len] of 0..3 or characters, or equally long strings."""

    def __init__(self, refs, k=10, max_occ=64):
        self._h = None
        _, _, self.refs = _inputs(b"", np.zeros((0, 2), np.int64), refs)
        self.k, self.max_occ = int(k), int(max_occ)
        _parameters(self.ref_len, self.k, self.max_occ, 1, 1, 0)
        self._L = load_library()
        h = ctypes.c_void_p()
        check(self._L.lva_map_index_create(self.refs.ctypes.data, self.n_refs, self.ref_len, self.k, self.max_occ, ctypes.byref(h)), None)
        self._h = h

    n_refs = property(lambda self: self.refs.shape[0])
    ref_len = property(lambda self: self.refs.shape[1])

    @property
    def handle(self):
        if self._h is None:
            raise ValueError("the index is closed")
        return self._h

    def info(self):
        """(kept distinct k-mers, kept pairs, k-mers dropped by max_occ)"""
        got = (ctypes.c_int64 * 3)()
        check(self._L.lva_map_index_info(self.handle, *(ctypes.addressof(got) + 8 * i for i in range(3))), None)
        return tuple(int(x) for x in got)

    def close(self):
        if self._h is not None:
            self._L.lva_map_index_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        self.close()


def map_reads(bases, windows, index, cands=4, min_votes=2, max_dist=None, device=0, chunk_reads=0):
    """reference_map on the device, all reads in one call (lva_map_reads): the same integers.  index: a MapIndex (its k and
    max_occ); chunk_reads: reads per pass over the device buffers, 0 = as many as fit; the result does not depend on it."""
    bases, windows, _ = _inputs(bases, windows, index.refs)
    max_dist = _parameters(index.ref_len, index.k, index.max_occ, cands, min_votes, max_dist)
    if not len(bases):
        bases = np.zeros(1, np.uint8)              # (every window is empty: something to point at)
    first, count = np.ascontiguousarray(windows[:, 0]), np.ascontiguousarray(windows[:, 1], dtype=np.int32)
    out = np.zeros((len(windows), 8), np.int32)
    check(load_library().lva_map_reads(device, index.handle, bases.ctypes.data, first.ctypes.data, count.ctypes.data, len(windows),
                                       cands, min(int(min_votes), 2 ** 31 - 1), min(max_dist, 2 ** 31 - 1), chunk_reads, out.ctypes.data))
    return MapResult(out)


def build_parser():
    p = argparse.ArgumentParser(description="map basecalled reads to oligos: <out_prefix>.map.tsv (a row per read), "
                                            "<out_prefix>.coverage.tsv (mapped reads per oligo and strand)")
    p.add_argument("--oligos", type=str, required=True, help="the oligo file of helper.encode: one ACGT string per line")
    p.add_argument("--post_manifest", type=str, required=True, help="readid <TAB> ref <TAB> post_path per read (generate_decoded_lists)")
    p.add_argument("--out_prefix", type=str, required=True)
    p.add_argument("--k", type=int, default=10)
    p.add_argument("--max_occ", type=int, default=64)
    p.add_argument("--cands", type=int, default=4)
    p.add_argument("--min_votes", type=int, default=2)
    p.add_argument("--max_dist", type=int, default=None, help="default: a quarter of the oligo length")
    p.add_argument("--chunk", type=int, default=4096, help="reads per pass over the manifest")
    p.add_argument("--device", type=int, default=0)
    return p


def main(argv=None, out=sys.stdout, decoder=None):
    """-> the MapResult of the manifest's reads, their whole basecalls mapped"""
    from . import helper
    from .decoder import Decoder
    a = build_parser().parse_args(argv)
    with open(a.oligos) as f:
        oligos = [ln.strip() for ln in f if ln.strip()]
    with open(a.post_manifest) as f:
        rows = [ln.rstrip("\n").split("\t") for ln in f if ln.strip()]
    if not oligos:
        raise SystemExit("the oligo file is empty")
    own = decoder is None
    # the basecall reads the posterior matrix alone: any code serves a decoder that is made for it
    dec = Decoder(6, 1, 60, list_size=1, max_deviation=20, device=a.device) if own else decoder
    parts = []
    try:
        with MapIndex(oligos, a.k, a.max_occ) as index:
            for at in range(0, len(rows), max(1, a.chunk)):
                with dec.resident([helper.read_post_file(row[2]) for row in rows[at:at + max(1, a.chunk)]]) as (dev, off):
                    calls = [b for b, _ in dec.basecall_resident(dev, off)]
                parts.append(map_reads("".join(calls), whole_windows(calls), index, a.cands, a.min_votes, a.max_dist, device=a.device).out)
    finally:
        if own:
            dec.close()
    res = MapResult(np.concatenate(parts + [np.zeros((0, 8), np.int32)]))
    with open(a.out_prefix + ".map.tsv", "w") as f:
        f.write("readid\t" + "\t".join(FIELDS) + "\n")
        for row, line in zip(rows, res.out.tolist()):
            f.write(row[0] + "\t" + "\t".join(str(v) for v in line) + "\n")
    with open(a.out_prefix + ".coverage.tsv", "w") as f:
        f.write("oligo\tforward\treverse\n")
        for o, (fwd, rev) in enumerate(res.coverage(len(oligos)).tolist()):
            f.write("%d\t%d\t%d\n" % (o, fwd, rev))
    print("reads:", len(rows), "mapped:", res.mapped, file=out)
    return res


def whole_windows(calls):
    """the windows of basecalls laid one after the other, each read whole (at most MAX_READ bases: the first of them)"""
    off = np.concatenate([[0], np.cumsum([len(b) for b in calls])]).astype(np.int64)
    return np.stack([off[:-1], np.minimum(np.diff(off), MAX_READ)], axis=1).reshape(-1, 2)


if __name__ == "__main__":
    main()
