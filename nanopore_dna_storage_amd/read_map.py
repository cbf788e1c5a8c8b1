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

A pooled run.  The reference's data is one sequencing run of thirteen experiments whose oligos differ in length (108 .. 119
bases), mapped against all of them at once.  Everything above is the special case "all oligos equally long, no supplementary
pass" of the following, and every call of that case returns the same integers as before.

  refs     n_refs oligos, each of its own length len[o], 1 <= len[o] <= MAX_REF: strings or code arrays of any lengths, a
           rectangular array, or the tuple (flat uint8 array, int64 offsets [n_refs + 1]).
  index    positions 0 .. len[o] - k of each oligo; an oligo shorter than k contributes nothing.
  dist     D has rows 0 .. len[o].  max_dist: None = len[o] // 4 per oligo, an integer = that value for every oligo, an
           array [n_refs] = a value per oligo; ref = best if d <= max_dist[best].
  winner   the distances of oligos of different lengths are compared as they are, not divided by the length: the oligo a
           read came from is at a few edits, an unrelated one at about 0.4 len[o], and the lengths of a pool differ by a
           tenth, so no normalisation can change which of the two is smaller; raw integers keep the order exact and make
           the equal-length case the same comparison.  A proper prefix of the source oligo is the one exception worth
           knowing: it is at distance 0 as well, and the place in the candidate order decides.
  start    the anchored reverse pass with the winner's own length.
  supplementary pass (min_flank > 0; 0 = none)   for a read with ref >= 0 the aligned part is [start, start + count) of the
           window as given, the left flank [0, start), the right flank [start + count, n).  The longer flank, the left one
           on a tie, is mapped as a read of its own through this same definition with the same parameters, one level
           only, if it has at least min_flank bases; its row's start is reported in the coordinates of the original window.
           Every other read's supplementary row is UNMAPPED.  A read is chimeric when its supplementary ref >= 0: two
           oligos ligated into one read, which the reference drops (-F 256, SA:Z:).  The tools' default of min_flank is
           half the shortest oligo's length.
  groups   optional int32 [n_refs], the experiment of each oligo: MapResult.group is groups[ref] (-1 where ref is -1), and
           MapResult.split gives per group the reads mapped to it and not chimeric -- the reference's
           exp_aligned_i.filtered.sam.

On the device a ragged index, a max_dist array or min_flank > 0 goes through lva_map_reads_pooled (csrc/mq_kernels.hip), held
to this definition bit for bit, out and supp (tests/test_gpu_read_map_pooled.py); everything else through lva_map_reads.

The index on the device.  MapIndex(..., device=d) uploads the oligos and builds the index there (lva_map_index_create_device,
csrc/mi_kernels.hip): the match masks; a histogram of 4^k counters in which every oligo counts each of its distinct k-mers
once; the counters above max_occ cleared; an exclusive prefix sum in three launches (a sum per tile, a scan of the sums, an
add) for the offsets; every kept pair placed in its k-mer's segment by an atomic, then moved to its rank among the segment's
oligos, so that a list is ascending whatever order the atomics ran in.  The tables are the bytes the host builder makes
(MapIndex.tables(), tests/test_gpu_map_index.py) and stay on the device until the index is closed: map_reads with such an
index uploads the reads alone and returns the same integers.  The command line takes --index device.  Out of scope:
error_profile --assign map and pooled --assign map keep the host index, and basecalls still pass through the host."""
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


class Oligos:
    """A set of oligos of any lengths, from what the module's docstring lists under refs (or another Oligos): flat (the bytes
    as given, one oligo after the other), off int64 [n + 1], lens int64 [n]; refs is the rectangular array [n, len] where the
    lengths are all equal, else None.  self[o]: the bytes of oligo o."""

    def __init__(self, refs):
        if isinstance(refs, Oligos):
            self.flat, self.off = refs.flat, refs.off
        elif (isinstance(refs, tuple) and len(refs) == 2 and all(isinstance(x, np.ndarray) and x.ndim == 1 for x in refs)
              and refs[0].dtype == np.uint8 and refs[1].dtype == np.int64):
            self.flat, self.off = np.ascontiguousarray(refs[0]), np.ascontiguousarray(refs[1])
            if len(self.off) < 1 or self.off[0] != 0 or self.off[-1] != len(self.flat):
                raise ValueError("offsets [n_refs + 1] from 0 to the length of the flat array")
        else:
            rows = [np.frombuffer(r.encode("ascii"), np.uint8) if isinstance(r, str) else np.asarray(r, dtype=np.uint8) for r in refs]
            if any(r.ndim != 1 for r in rows):
                raise ValueError("refs [n_refs, ref_len], or a list of oligos")
            self.flat = np.ascontiguousarray(np.concatenate(rows + [np.zeros(0, np.uint8)]))
            self.off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
        self.lens = np.diff(self.off)
        if not len(self.lens) or self.lens.min() < 1 or self.lens.max() > MAX_REF:
            raise ValueError("at least one oligo, each of 1 .. %d bases" % MAX_REF)
        self.refs = self.flat.reshape(len(self.lens), -1) if self.lens.min() == self.lens.max() else None

    def __len__(self):
        return len(self.lens)

    def __getitem__(self, o):
        return self.flat[self.off[o]:self.off[o + 1]]


def _parameters(lens, k, max_occ, cands, min_votes, max_dist, min_flank=0):
    """-> max_dist as int64 [n_refs], from its three forms"""
    lens = np.asarray(lens, dtype=np.int64)
    if max_dist is None:
        max_dist = lens // 4
    elif np.ndim(max_dist) == 0:
        max_dist = np.full(len(lens), int(max_dist), np.int64)
    max_dist = np.asarray(max_dist, dtype=np.int64)
    if max_dist.shape != lens.shape:
        raise ValueError("max_dist: None, an integer or an array [n_refs]")
    if not (K_RANGE[0] <= k <= K_RANGE[1] and 1 <= max_occ <= 65535 and 1 <= cands <= MAX_CANDS and min_votes >= 1 and max_dist.min() >= 0
            and min_flank >= 0):
        raise ValueError("6 <= k <= 12, 1 <= max_occ <= 65535, 1 <= cands <= 8, min_votes >= 1, max_dist >= 0, min_flank >= 0")
    return max_dist


def _groups(groups, n_refs):
    if groups is None:
        return None
    groups = np.ascontiguousarray(groups, dtype=np.int32)
    if groups.shape != (n_refs,) or groups.min() < 0:
        raise ValueError("groups [n_refs], each >= 0")
    return groups


def _inputs(bases, windows):
    windows = np.ascontiguousarray(windows, dtype=np.int64).reshape(-1, 2)
    bases, windows, _, _, _ = _arguments(bases, windows, np.zeros((1, 1), np.uint8), np.zeros(len(windows), np.int32), None)
    return bases, windows


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
        refs = Oligos(refs)
        parts = []
        for o in range(len(refs)):
            kmer, ok = _kmers(_CODE[refs[o]], k)
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
    """out int32 [n, 8] = (ref, best, rc, dist, start, count, votes, second) (the module's docstring); a column by its name.
    supp: the MapResult of the supplementary rows, None where the call made no supplementary pass; groups: the call's."""

    def __init__(self, out, supp=None, groups=None):
        self.out, self.supp, self.groups = out, supp, groups

    def __getattr__(self, name):
        if name in FIELDS:
            return self.out[:, FIELDS.index(name)]
        raise AttributeError(name)

    def __len__(self):
        return len(self.out)

    @property
    def mapped(self):
        return int((self.ref >= 0).sum())

    @property
    def chimeric(self):
        """bool [n]: the supplementary pass found a second oligo in the read"""
        return np.zeros(len(self), bool) if self.supp is None else self.supp.ref >= 0

    @property
    def group(self):
        """int32 [n]: groups[ref], -1 where ref is -1"""
        return self._group(self.groups)

    def _group(self, groups):
        if groups is None:
            raise ValueError("the reads were mapped without groups")
        groups = np.asarray(groups, dtype=np.int32)
        return np.where(self.ref >= 0, groups[np.maximum(self.ref, 0)], -1).astype(np.int32)

    def split(self, groups=None, n_groups=None):
        """per group the numbers of the reads mapped to it and not chimeric (groups: the call's unless given)"""
        g = self._group(self.groups if groups is None else groups)
        g = np.where(self.chimeric, -1, g)
        n_groups = int(np.max(self.groups if groups is None else groups)) + 1 if n_groups is None else n_groups
        return [np.nonzero(g == i)[0] for i in range(n_groups)]

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


def _map_window(x, index, codes, cands, min_votes, max_dist):
    """one window of codes through the definition -> its row, start and count in the coordinates of x"""
    strands = (x, _reverse_complement(x))
    found = []
    for s in (0, 1):
        v = index.votes(strands[s])
        found += [(-int(v[o]), s, int(o)) for o in np.nonzero(v >= min_votes)[0]]
    found = sorted(found)[:cands]
    if not found:
        return UNMAPPED
    dist = [end_distance(codes[o], strands[s]) for _, s, o in found]
    place = min(range(len(found)), key=lambda c: (dist[c][0], c))
    (d, e), (v, s, o) = dist[place], found[place]
    others = [dist[c][0] for c in range(len(found)) if found[c][2] != o]
    E = start_row(codes[o], strands[s], e)
    assert E.min() == d, "the anchored pass attains the distance"
    jp = int(np.argmax(E == d))
    return (o if d <= max_dist[o] else -1, o, s, d, e - jp if s == 0 else len(x) - e, jp, -v, min(others) if others else -1)


def flank(start, count, n):
    """(first base, bases) of the longer unaligned flank of a window of n bases whose aligned part is [start, start + count):
    the left one on a tie"""
    return (0, start) if start >= n - (start + count) else (start + count, n - (start + count))


def reference_map(bases, windows, refs, k=10, max_occ=64, cands=4, min_votes=2, max_dist=None, min_flank=0, groups=None):
    """The definition (the module's docstring), a read at a time.  bases, windows [n, 2] as error_profile.reference_profile
    takes them; refs, max_dist, min_flank, groups as the module's docstring says.  -> MapResult"""
    bases, windows = _inputs(bases, windows)
    refs = Oligos(refs)
    max_dist = _parameters(refs.lens, k, max_occ, cands, min_votes, max_dist, min_flank)
    groups = _groups(groups, len(refs))
    index = ReferenceIndex(refs, k, max_occ)
    codes = [_CODE[refs[o]] for o in range(len(refs))]
    out = np.empty((len(windows), 8), np.int32)
    out[:] = UNMAPPED
    supp = out.copy() if min_flank > 0 else None
    for r, (first, count) in enumerate(windows):
        x = _CODE[bases[first:first + count]]
        out[r] = _map_window(x, index, codes, cands, min_votes, max_dist)
        if supp is not None and out[r, 0] >= 0:
            at, n = flank(int(out[r, 4]), int(out[r, 5]), len(x))
            if n >= min_flank:
                supp[r] = _map_window(x[at:at + n], index, codes, cands, min_votes, max_dist)
                if supp[r, 1] >= 0:
                    supp[r, 4] += at
    return MapResult(out, None if supp is None else MapResult(supp, None, groups), groups)


class MapIndex:
    """The index of a set of oligos: the k-mer table and the oligos' match masks; owns the handle, a context manager.
    device None: built on the host (lva_map_index_create, lva_map_index_create_pooled where the lengths differ), every
    map_reads call uploads it; an ordinal: built on that device from the uploaded oligos (lva_map_index_create_device) and
    resident there until close(), the same tables, and map_reads uploads the reads alone.  refs: what the module's docstring
    lists; groups: optional int32 [n_refs], carried into the results of map_reads.  refs is the rectangular array where the
    lengths are equal, else None; lens [n_refs]; ref_len is the longest."""

    def __init__(self, refs, k=10, max_occ=64, groups=None, device=None):
        self._h = None
        self.oligos = Oligos(refs)
        self.refs, self.lens = self.oligos.refs, self.oligos.lens
        self.groups = _groups(groups, len(self.lens))
        self.k, self.max_occ = int(k), int(max_occ)
        self.device = None if device is None else int(device)
        _parameters(self.lens, self.k, self.max_occ, 1, 1, 0)
        self._L = load_library()
        h = ctypes.c_void_p()
        if self.device is not None:
            check(self._L.lva_map_index_create_device(self.device, self.oligos.flat.ctypes.data, self.oligos.off.ctypes.data, self.n_refs,
                                                      self.k, self.max_occ, ctypes.byref(h)))
        elif self.ragged:
            check(self._L.lva_map_index_create_pooled(self.oligos.flat.ctypes.data, self.oligos.off.ctypes.data, self.n_refs, self.k,
                                                      self.max_occ, ctypes.byref(h)), None)
        else:
            check(self._L.lva_map_index_create(self.refs.ctypes.data, self.n_refs, self.ref_len, self.k, self.max_occ, ctypes.byref(h)), None)
        self._h = h

    n_refs = property(lambda self: len(self.lens))
    ref_len = property(lambda self: int(self.lens.max()))
    ragged = property(lambda self: self.refs is None)

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

    def tables(self):
        """(offsets uint32 [4^k + 1], lists int32 [pairs], masks uint64 [n_refs, 2, 4, ceil(ref_len / 64)]) copied to the host:
        the oligos of k-mer c are lists[offsets[c]:offsets[c + 1]], ascending; the same bytes however the index was built"""
        offsets, lists = np.zeros(4 ** self.k + 1, np.uint32), np.zeros(self.info()[1], np.int32)
        masks = np.zeros((self.n_refs, 2, 4, (self.ref_len + 63) // 64), np.uint64)
        check(self._L.lva_map_index_tables(self.handle, offsets.ctypes.data, lists.ctypes.data, masks.ctypes.data))
        return offsets, lists, masks

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


def map_reads(bases, windows, index, cands=4, min_votes=2, max_dist=None, device=0, chunk_reads=0, min_flank=0):
    """reference_map on the device, all reads in one call: the same integers.  index: a MapIndex (its k, max_occ and groups);
    chunk_reads: reads per pass over the device buffers, 0 = as many as fit; the result does not depend on it.  A ragged
    index, a max_dist array or min_flank > 0 goes through lva_map_reads_pooled, everything else through lva_map_reads.  An
    index built on a device serves the calls on that device: another one is a ValueError."""
    bases, windows = _inputs(bases, windows)
    if index.device is not None and index.device != device:
        raise ValueError("the index lives on device %d, the call is for device %d" % (index.device, device))
    pooled = index.ragged or min_flank > 0 or not (max_dist is None or np.ndim(max_dist) == 0)
    max_dist = np.minimum(_parameters(index.lens, index.k, index.max_occ, cands, min_votes, max_dist, min_flank), 2 ** 31 - 1).astype(np.int32)
    if not len(bases):
        bases = np.zeros(1, np.uint8)              # (every window is empty: something to point at)
    first, count = np.ascontiguousarray(windows[:, 0]), np.ascontiguousarray(windows[:, 1], dtype=np.int32)
    out = np.zeros((len(windows), 8), np.int32)
    supp = np.zeros((len(windows), 8), np.int32) if min_flank > 0 else None
    L = load_library()
    if pooled:
        check(L.lva_map_reads_pooled(device, index.handle, bases.ctypes.data, first.ctypes.data, count.ctypes.data, len(windows), cands,
                                     min(int(min_votes), 2 ** 31 - 1), max_dist.ctypes.data, min(int(min_flank), 2 ** 31 - 1), chunk_reads,
                                     out.ctypes.data, None if supp is None else supp.ctypes.data))
    else:
        check(L.lva_map_reads(device, index.handle, bases.ctypes.data, first.ctypes.data, count.ctypes.data, len(windows),
                              cands, min(int(min_votes), 2 ** 31 - 1), int(max_dist[0]), chunk_reads, out.ctypes.data))
    return MapResult(out, None if supp is None else MapResult(supp, None, index.groups), index.groups)


def build_parser():
    p = argparse.ArgumentParser(description="map basecalled reads to oligos: <out_prefix>.map.tsv (a row per read), "
                                            "<out_prefix>.coverage.tsv (mapped reads per oligo and strand); a pooled run "
                                            "(several oligo files, or --min_flank) also <out_prefix>.<group>.readids.txt")
    p.add_argument("--oligos", type=str, required=True, nargs="+",
                   help="the oligo file of helper.encode: one ACGT string per line; several files: a pooled run, one group per "
                        "file, named by the file's stem")
    p.add_argument("--post_manifest", type=str, required=True, help="readid <TAB> ref <TAB> post_path per read (generate_decoded_lists)")
    p.add_argument("--out_prefix", type=str, required=True)
    p.add_argument("--k", type=int, default=10)
    p.add_argument("--max_occ", type=int, default=64)
    p.add_argument("--cands", type=int, default=4)
    p.add_argument("--min_votes", type=int, default=2)
    p.add_argument("--max_dist", type=int, default=None, help="default: a quarter of the oligo length")
    p.add_argument("--min_flank", type=int, default=None,
                   help="bases an unaligned flank needs for the supplementary pass that flags chimeric reads; 0: no pass, -1: half "
                        "the shortest oligo (the default with several oligo files; with one file the default is no pass)")
    p.add_argument("--chunk", type=int, default=4096, help="reads per pass over the manifest")
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--index", choices=("host", "device"), default="host",
                   help="where the index is built: on the host, uploaded with every chunk, or on --device, resident there for "
                        "the run; the files are the same")
    return p


def read_oligo_files(paths):
    """-> (oligos of all files one after the other, groups int32 [n_refs], the groups' names: the files' stems)"""
    import os
    oligos, groups, names = [], [], []
    for g, path in enumerate(paths):
        with open(path) as f:
            lines = [ln.strip() for ln in f if ln.strip()]
        if not lines:
            raise SystemExit("the oligo file %s is empty" % path)
        oligos += lines
        groups += [g] * len(lines)
        names.append(os.path.splitext(os.path.basename(path))[0])
    if len(set(names)) != len(names):
        raise SystemExit("two oligo files have the same stem")
    return oligos, np.array(groups, np.int32), names


def main(argv=None, out=sys.stdout, decoder=None):
    """-> the MapResult of the manifest's reads, their whole basecalls mapped"""
    from . import helper
    from .decoder import Decoder
    a = build_parser().parse_args(argv)
    oligos, groups, names = read_oligo_files(a.oligos)
    pooled = len(names) > 1 or a.min_flank is not None         # one file and no --min_flank: the outputs as they always were
    min_flank = (-1 if len(names) > 1 else 0) if a.min_flank is None else a.min_flank
    if min_flank < 0:
        min_flank = min(len(o) for o in oligos) // 2
    with open(a.post_manifest) as f:
        rows = [ln.rstrip("\n").split("\t") for ln in f if ln.strip()]
    own = decoder is None
    # the basecall reads the posterior matrix alone: any code serves a decoder that is made for it
    dec = Decoder(6, 1, 60, list_size=1, max_deviation=20, device=a.device) if own else decoder
    parts, supps = [], []
    try:
        with MapIndex(oligos, a.k, a.max_occ, groups if pooled else None, device=a.device if a.index == "device" else None) as index:
            for at in range(0, len(rows), max(1, a.chunk)):
                with dec.resident([helper.read_post_file(row[2]) for row in rows[at:at + max(1, a.chunk)]]) as (dev, off):
                    calls = [b for b, _ in dec.basecall_resident(dev, off)]
                got = map_reads("".join(calls), whole_windows(calls), index, a.cands, a.min_votes, a.max_dist, device=a.device, min_flank=min_flank)
                parts.append(got.out)
                supps.append(got.supp.out if got.supp is not None else np.tile(np.array(UNMAPPED, np.int32), (len(got), 1)))
    finally:
        if own:
            dec.close()
    none = [np.zeros((0, 8), np.int32)]
    if not pooled:
        res = MapResult(np.concatenate(parts + none))
    else:
        res = MapResult(np.concatenate(parts + none), MapResult(np.concatenate(supps + none), None, groups), groups)
        group, chimeric = res.group.tolist(), res.chimeric.tolist()
    with open(a.out_prefix + ".map.tsv", "w") as f:
        f.write("readid\t" + "\t".join(FIELDS + (("group", "chimeric") + tuple("supp_" + x for x in FIELDS) if pooled else ())) + "\n")
        for i, (row, line) in enumerate(zip(rows, res.out.tolist())):
            if pooled:
                line = line + [names[group[i]] if group[i] >= 0 else "-", int(chimeric[i])] + res.supp.out[i].tolist()
            f.write(row[0] + "\t" + "\t".join(str(v) for v in line) + "\n")
    with open(a.out_prefix + ".coverage.tsv", "w") as f:
        f.write("group\toligo\tforward\treverse\n" if pooled else "oligo\tforward\treverse\n")
        for o, (fwd, rev) in enumerate(res.coverage(len(oligos)).tolist()):
            f.write((names[groups[o]] + "\t" if pooled else "") + "%d\t%d\t%d\n" % (o, fwd, rev))
    if not pooled:
        print("reads:", len(rows), "mapped:", res.mapped, file=out)
        return res
    counts = []
    for name, reads in zip(names, res.split(n_groups=len(names))):
        with open("%s.%s.readids.txt" % (a.out_prefix, name), "w") as f:
            f.write("".join(rows[i][0] + "\n" for i in reads))
        counts += [name + ":", len(reads)]
    print("reads:", len(rows), "mapped:", res.mapped, "chimeric:", int(res.chimeric.sum()), *counts, file=out)
    return res


def whole_windows(calls):
    """the windows of basecalls laid one after the other, each read whole (at most MAX_READ bases: the first of them)"""
    off = np.concatenate([[0], np.cumsum([len(b) for b in calls])]).astype(np.int64)
    return np.stack([off[:-1], np.minimum(np.diff(off), MAX_READ)], axis=1).reshape(-1, 2)


if __name__ == "__main__":
    main()
