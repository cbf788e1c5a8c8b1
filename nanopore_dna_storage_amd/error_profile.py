"""The error profile of a set of reads: what the channel did, measured.  Every read is aligned
to the oligo it names and its matches, substitutions, deletions and insertions are tallied by oligo position.  The reference
does this outside the decoder -- util/align_compute_stats.sh:45-52 maps basecalls to oligos with minimap2 and runs samtools
stats, util/compile_plot_stats.py turns the counts into <prefix>.error_stats.csv -- and feeds the rates to its simulator.
Here a read names its oligo already (the index the CRC filter accepted, or a simulator's truth), so what is left is the
alignment and the tally.  This file is the definition in numpy / Python (reference_profile) and the call into the device
path (lva_align_profile, csrc/ep_kernels.hip), which is held to it bit for bit (tests/test_gpu_error_profile.py).

The definition.  A byte is a base if it is A, C, G, T or 0, 1, 2, 3 (basecall characters, lva_encode's codes); any other
byte is N and equals nothing, itself included.  Read i is the window bases[first : first + count]; with its rc flag set the
window is reverse-complemented first (N stays N) and then aligned to the forward reference, so positions are always oligo
positions.  D is the unit-cost global edit-distance matrix, i over reference positions 0 .. ref_len, j over the window
0 .. n, D[i][0] = i, D[0][j] = j.  The walk starts at (ref_len, n) and takes at (i, j) the first move that applies -- the
order is part of the definition, homopolymers make ties the normal case:

  1. diagonal, if i > 0, j > 0 and D[i-1][j-1] + (ref[i-1] != read[j-1]) == D[i][j]: a match or a substitution at i - 1;
  2. up, if i > 0 and D[i-1][j] + 1 == D[i][j]: a deletion at position i - 1;
  3. left: an insertion in front of position i, i in 0 .. ref_len.

Results, all exact integers: read int32 [n, 4] = (distance, substitutions, deletions, insertions) per read, four times -1
for a skipped read (ref_id < 0), which adds nothing to the rest; pos int64 [ref_len + 1, 4] = per oligo position (matches,
substitutions, deletions, bases inserted in front of it); conf int64 [4, 6] = per reference base how often it was read as
A, C, G, T, N or deleted (a reference N counts in no row of conf, but does in pos); ins int64 [5] = inserted bases by value.
"""
import argparse
import sys

import numpy as np

from ._lib import check, load_library

MAX_REF = 1024            # reference positions of one call (the simulator's strand limit)
MAX_READ = 4096           # bases of a read window
N = 4                     # the code of a byte that is no base

_CODE = np.full(256, N, np.uint8)
for _k, _ch in enumerate("ACGT"):
    _CODE[ord(_ch)] = _CODE[_k] = _k


class ErrorProfile:
    """read int32 [n, 4], pos int64 [ref_len + 1, 4], conf int64 [4, 6], ins int64 [5] (the module's docstring)"""

    def __init__(self, read, pos, conf, ins):
        self.read, self.pos, self.conf, self.ins = read, pos, conf, ins

    @property
    def ref_len(self):
        return len(self.pos) - 1

    @property
    def reads(self):
        """reads that were not skipped"""
        return int((self.read[:, 0] >= 0).sum())

    def __eq__(self, other):
        return all(a.dtype == b.dtype and np.array_equal(a, b) for a, b in
                   ((self.read, other.read), (self.pos, other.pos), (self.conf, other.conf), (self.ins, other.ins)))

    def __add__(self, other):
        """the profile of both sets of reads, this one's first"""
        if self.ref_len != other.ref_len:
            raise ValueError("profiles of different reference lengths")
        return ErrorProfile(np.concatenate([self.read, other.read]), self.pos + other.pos, self.conf + other.conf, self.ins + other.ins)

    def aligned(self):
        """reference bases aligned: matches + substitutions + deletions = reads * ref_len"""
        return int(self.pos[:, :3].sum())

    def rates(self):
        """substitutions, deletions and inserted bases per reference base aligned"""
        n = self.aligned()
        if n == 0:
            raise ValueError("no read was aligned")
        return dict(sub=int(self.pos[:, 1].sum()) / n, dele=int(self.pos[:, 2].sum()) / n, ins=int(self.pos[:, 3].sum()) / n)

    def channel(self):
        """The three probabilities in the form Decoder.simulate takes (simulate.py's channel): a base is deleted with
        probability dele, a base that is kept is substituted with probability sub, and each of the ref_len + 1 gaps
        receives a run of insertions that goes on with probability ins, g = ins / (1 - ins) bases on average."""
        n, dels = self.aligned(), int(self.pos[:, 2].sum())
        if n == 0 or n == dels:
            raise ValueError("no base was read")
        g = int(self.pos[:, 3].sum()) / (self.reads * (self.ref_len + 1))
        return dict(sub=int(self.pos[:, 1].sum()) / (n - dels), dele=dels / n, ins=g / (1 + g))

    def write_csv(self, prefix):
        """<prefix>.error_stats.csv in util/compile_plot_stats.py's layout: three sections of position,rate lines, each
        rate = count / reads; positions are oligo positions from 0, insertions in front of position 0 .. ref_len"""
        reads = self.reads
        if reads == 0:
            raise ValueError("no read was aligned")
        with open(prefix + ".error_stats.csv", "w") as f:
            for name, col, rows in (("subs", 1, self.ref_len), ("ins", 3, self.ref_len + 1), ("del", 2, self.ref_len)):
                f.write("%s_pos,%s_rate\n" % (name, name))
                for p in range(rows):
                    f.write(str(p) + "," + str(int(self.pos[p, col]) / reads) + "\n")


def _arguments(bases, windows, refs, ref_id, rc):
    if isinstance(bases, str):
        bases = bases.encode("ascii")
    bases = np.frombuffer(bases, np.uint8) if isinstance(bases, (bytes, bytearray)) else np.ascontiguousarray(bases, dtype=np.uint8)
    if isinstance(refs, (list, tuple)) and refs and isinstance(refs[0], str):
        refs = np.array([np.frombuffer(r.encode("ascii"), np.uint8) for r in refs])
    refs = np.ascontiguousarray(refs, dtype=np.uint8)
    windows = np.ascontiguousarray(windows, dtype=np.int64).reshape(-1, 2)
    ref_id = np.ascontiguousarray(ref_id, dtype=np.int32)
    n = len(windows)
    rc = np.zeros(n, np.uint8) if rc is None else np.ascontiguousarray(np.asarray(rc) != 0, dtype=np.uint8)
    if bases.ndim != 1 or refs.ndim != 2 or ref_id.shape != (n,) or rc.shape != (n,):
        raise ValueError("bases [B], windows [n, 2] = (first base, count), refs [n_refs, ref_len], ref_id [n], rc [n]")
    if not (1 <= refs.shape[1] <= MAX_REF and refs.shape[0] >= 1):
        raise ValueError("1 <= ref_len <= %d, at least one reference" % MAX_REF)
    if n and (windows.min() < 0 or windows[:, 1].max() > MAX_READ or (windows[:, 0] + windows[:, 1]).max() > len(bases)):
        raise ValueError("a window of 0 .. %d bases inside the buffer" % MAX_READ)
    if n and ref_id.max() >= len(refs):
        raise ValueError("ref_id past the references")
    return bases, windows, refs, ref_id, rc


def _distance_matrix(ref, read):
    """D int32 [len(ref) + 1, len(read) + 1]; a row at a time: D[i][j] = min(t[j], D[i][j-1] + 1) with t the minimum over
    the other two moves, so D[i][j] - j is the running minimum of t[j] - j"""
    m, n = len(ref), len(read)
    j = np.arange(n + 1, dtype=np.int32)
    D = np.empty((m + 1, n + 1), np.int32)
    D[0] = j
    for i in range(1, m + 1):
        t = np.empty(n + 1, np.int32)
        t[0] = i
        cost = (read != ref[i - 1]) | (read == N)
        np.minimum(D[i - 1, 1:] + 1, D[i - 1, :-1] + cost, out=t[1:])
        D[i] = np.minimum.accumulate(t - j) + j
    return D


def reference_profile(bases, windows, refs, ref_id, rc=None):
    """The definition (the module's docstring), a read at a time.  bases: uint8 array, bytes or str; windows [n, 2] =
    (first base, count) per read, inside `bases`, windows may overlap; refs [n_refs, ref_len] uint8, or equally long strings;
    ref_id [n] (< 0: the read is skipped); rc [n] or None.  -> ErrorProfile"""
    bases, windows, refs, ref_id, rc = _arguments(bases, windows, refs, ref_id, rc)
    m = refs.shape[1]
    read_out = np.full((len(windows), 4), -1, np.int32)
    pos, conf, ins = np.zeros((m + 1, 4), np.int64), np.zeros((4, 6), np.int64), np.zeros(5, np.int64)
    for r, (first, count) in enumerate(windows):
        if ref_id[r] < 0:
            continue
        ref = _CODE[refs[ref_id[r]]]
        read = _CODE[bases[first:first + count]]
        if rc[r]:
            read = np.where(read < N, 3 - read, N).astype(np.uint8)[::-1]
        D = _distance_matrix(ref, read).tolist()
        ref, read = ref.tolist(), read.tolist()
        i, j = m, int(count)
        sub = dele = insn = 0
        while i > 0 or j > 0:
            if i > 0 and j > 0 and D[i - 1][j - 1] + (ref[i - 1] != read[j - 1] or ref[i - 1] == N) == D[i][j]:
                same = ref[i - 1] == read[j - 1] and ref[i - 1] != N
                pos[i - 1, 0 if same else 1] += 1
                sub += not same
                if ref[i - 1] != N:
                    conf[ref[i - 1], read[j - 1]] += 1
                i, j = i - 1, j - 1
            elif i > 0 and D[i - 1][j] + 1 == D[i][j]:
                pos[i - 1, 2] += 1
                dele += 1
                if ref[i - 1] != N:
                    conf[ref[i - 1], 5] += 1
                i -= 1
            else:
                pos[i, 3] += 1
                ins[read[j - 1]] += 1
                insn += 1
                j -= 1
        read_out[r] = (D[m][int(count)], sub, dele, insn)
    return ErrorProfile(read_out, pos, conf, ins)


def align_profile(bases, windows, refs, ref_id, rc=None, device=0, chunk_reads=0):
    """reference_profile on the device, all reads in one call (lva_align_profile): the same integers.  chunk_reads: reads per
    pass over the device buffers, 0 = as many as fit 1 GiB; the result does not depend on it."""
    bases, windows, refs, ref_id, rc = _arguments(bases, windows, refs, ref_id, rc)
    n, m = len(windows), refs.shape[1]
    if not len(bases):
        bases = np.zeros(1, np.uint8)              # (every window is empty: something to point at)
    first, count = np.ascontiguousarray(windows[:, 0]), np.ascontiguousarray(windows[:, 1], dtype=np.int32)
    read = np.zeros((n, 4), np.int32)
    pos, conf, ins = np.zeros((m + 1, 4), np.int64), np.zeros((4, 6), np.int64), np.zeros(5, np.int64)
    check(load_library().lva_align_profile(device, bases.ctypes.data, first.ctypes.data, count.ctypes.data, n,
                                            refs.ctypes.data, len(refs), m, ref_id.ctypes.data, rc.ctypes.data, chunk_reads,
                                            read.ctypes.data, pos.ctypes.data, conf.ctypes.data, ins.ctypes.data))
    return ErrorProfile(read, pos, conf, ins)


def payload_windows(trans_lists, located):
    """The base window of a located payload: the bases b of the read's basecall with start_pos + 1 <= trans[b] <=
    end_pos + 1 -- helper.find_barcode_pos (helper.py:190-194 of the reference) read backwards: start_pos is the block in
    front of the first base behind the start barcode, end_pos the block in front of the last base before the end barcode.
    trans_lists: per read the transition positions of its basecall (Decoder.basecall); located: per read a dict with ok,
    start_pos, end_pos (Decoder.locate_payload).  -> int64 [n, 2] = (first base, count), (0, 0) where ok is not set."""
    out = np.zeros((len(located), 2), np.int64)
    for i, (t, lc) in enumerate(zip(trans_lists, located)):
        if not lc["ok"]:
            continue
        t = np.asarray(t, dtype=np.int64)
        b = np.nonzero((t >= lc["start_pos"] + 1) & (t <= lc["end_pos"] + 1))[0]
        if len(b):
            out[i] = (b[0], b[-1] - b[0] + 1)
    return out


def profile_decoded(dec, dev, off, located_results, filter_index, oligos, device=None):
    """The real-data path: the profile of the reads of a resident posterior buffer (dev, off) whose payloads were located and
    decoded (located_results: what Decoder.decode_located returns, [(location, result)], or the locations alone) and whose
    list passed the CRC / index filter (filter_index [n]: list_ops.filter_lists' index, -1: none).  One basecall_resident
    call; the windows are payload_windows' of the basecalls, the reference of a read is oligos[filter_index], its
    orientation the location's rc.  oligos: [num_oligos, oligo_len] of 0..3, or ACGT strings.  -> ErrorProfile"""
    located = [lr[0] if isinstance(lr, tuple) else lr for lr in located_results]
    calls = dec.basecall_resident(dev, off)
    win = payload_windows([t for _, t in calls], located)
    base_off = np.zeros(len(calls) + 1, np.int64)
    base_off[1:] = np.cumsum([len(b) for b, _ in calls])
    win[:, 0] += base_off[:-1]
    ok = np.array([bool(lc["ok"]) for lc in located], dtype=bool)
    ref_id = np.where(ok, np.asarray(filter_index, dtype=np.int32), -1).astype(np.int32)
    return align_profile("".join(b for b, _ in calls), win, oligos, ref_id, rc=[bool(lc["rc"]) and bool(lc["ok"]) for lc in located],
                         device=dec.device if device is None else device)


def profile_mapped(dec, dev, off, index, cands=4, min_votes=2, max_dist=None, device=None, min_flank=0):
    """The profile of reads that name no oligo: one basecall_resident call over a resident posterior buffer (dev, off), the
    whole basecalls mapped to the oligos of `index` (a read_map.MapIndex; read_map.map_reads), and the mapped parts aligned to
    the oligo and on the strand the mapping found.  No list is decoded and no barcode is looked for, so reads whose list
    failed the CRC are counted.  -> (ErrorProfile, read_map.MapResult).  An index with groups (a pooled run): one profile per
    group, over the reads mapped to the group and not chimeric (min_flank: read_map's supplementary pass), each one
    align_profile call; the oligos of a group are equally long.  -> ([ErrorProfile per group], read_map.MapResult)"""
    from . import read_map
    device = dec.device if device is None else device
    calls = [b for b, _ in dec.basecall_resident(dev, off)]
    bases, win = "".join(calls), read_map.whole_windows(calls)
    res = read_map.map_reads(bases, win, index, cands, min_votes, max_dist, device=device, min_flank=min_flank)
    if index.groups is None:
        if index.ragged:
            raise ValueError("oligos of unequal length: give the index groups of equally long oligos")
        return align_profile(bases, res.windows(win), index.refs, res.ref, res.rc, device=device), res
    return [align_profile(bases, res.windows(win), refs, ref_id, res.rc, device=device)
            for refs, ref_id in group_references(index, res)], res


def group_references(index, res):
    """per group of a read_map.MapIndex with groups: (the group's oligos [n, len], per read the place of its oligo among them,
    -1 for a read that is unmapped, chimeric or of another group) -- the refs and ref_id of one align_profile call"""
    group = np.where(res.chimeric, -1, res.group)
    parts = []
    for g in range(int(index.groups.max()) + 1):
        members = np.nonzero(index.groups == g)[0]
        if not len(members) or len(set(index.lens[members].tolist())) != 1:
            raise ValueError("group %d holds no oligo, or oligos of unequal length: a profile is per oligo position" % g)
        place = np.full(index.n_refs, -1, np.int32)
        place[members] = np.arange(len(members), dtype=np.int32)
        parts.append((np.stack([index.oligos[o] for o in members]), np.where(group == g, place[np.maximum(res.ref, 0)], -1).astype(np.int32)))
    return parts


def build_parser():
    p = argparse.ArgumentParser(description="error profile of basecalled reads against their oligos: locate, decode, filter, "
                                            "align, <out_prefix>.error_stats.csv")
    p.add_argument("--oligos", type=str, required=True, nargs="+",
                   help="the oligo file of helper.encode: one ACGT string per line; several files (--assign map only): a pooled "
                        "run, one group and one <out_prefix>.<stem>.error_stats.csv per file")
    p.add_argument("--post_manifest", type=str, required=True, help="readid <TAB> ref <TAB> post_path per read (generate_decoded_lists)")
    p.add_argument("--start_barcode", type=str, required=True)
    p.add_argument("--end_barcode", type=str, required=True)
    p.add_argument("--mem_conv", type=int, required=True)
    p.add_argument("--msg_len", type=int, required=True)
    p.add_argument("--rate_conv", type=int, required=True)
    p.add_argument("--list_size", type=int, required=True)
    p.add_argument("--out_prefix", type=str, required=True)
    p.add_argument("--max_deviation", type=int, default=20)
    p.add_argument("--chunk", type=int, default=4096, help="reads per pass over the manifest")
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--assign", choices=("filter", "map"), default="filter",
                   help="a read's oligo: the index its decoded list passed the CRC with, or read_map's mapping of its whole basecall "
                        "(no list is decoded)")
    return p


def main(argv=None, out=sys.stdout, decoder=None):
    """-> the ErrorProfile of the manifest's reads whose list passed the filter (--assign map: that were mapped)"""
    from . import helper, list_ops
    from .decoder import Decoder
    a = build_parser().parse_args(argv)
    if len(a.oligos) > 1:
        if a.assign != "map":
            raise SystemExit("several --oligos files (a pooled run) need --assign map")
        return pooled_main(a, out, decoder)
    with open(a.oligos[0]) as f:
        oligos = [ln.strip() for ln in f if ln.strip()]
    with open(a.post_manifest) as f:
        paths = [ln.rstrip("\n").split("\t")[2] for ln in f if ln.strip()]
    bytes_per_oligo, pad = divmod(a.msg_len - helper.index_len - helper.crc_len, 8)
    if pad > 1 or bytes_per_oligo < 1 or not oligos:
        raise SystemExit("--msg_len is not 12 + 8 * bytes_per_oligo + 8 (+ 1), or the oligo file is empty")
    own = decoder is None
    dec = Decoder(a.mem_conv, a.rate_conv, a.msg_len, list_size=a.list_size, max_deviation=a.max_deviation, device=a.device) if own else decoder
    total, mapped, map_index = None, 0, None
    try:
        if a.assign == "map":
            from .read_map import MapIndex
            map_index = MapIndex(oligos)
        for k in range(0, len(paths), max(1, a.chunk)):
            with dec.resident([helper.read_post_file(p) for p in paths[k:k + max(1, a.chunk)]]) as (dev, off):
                if map_index is not None:
                    part, res = profile_mapped(dec, dev, off, map_index, device=a.device)
                    mapped += res.mapped
                else:
                    chain = dec.decode_located(dev, off, dec.locate_payload_resident(dev, off, a.start_barcode, a.end_barcode))
                    msgs, counts = list_ops.results_to_array([-100 if res is None else res for _, res in chain], dec.list_size, a.msg_len)
                    index, _, _ = list_ops.filter_lists(msgs, counts, bytes_per_oligo, len(oligos), pad=bool(pad), device=a.device)
                    part = profile_decoded(dec, dev, off, chain, index, oligos, device=a.device)
            total = part if total is None else total + part
    finally:
        if map_index is not None:
            map_index.close()
        if own:
            dec.close()
    counted = ["reads:", len(paths)] + (["mapped:", mapped] if a.assign == "map" else [])
    if total is None or total.reads == 0:
        print(*counted, "aligned: 0", file=out)
        return total
    total.write_csv(a.out_prefix)
    r = total.rates()
    print(*counted, "aligned:", total.reads, file=out)
    print("sub %.6f dele %.6f ins %.6f per reference base" % (r["sub"], r["dele"], r["ins"]), file=out)
    return total


def pooled_main(a, out, decoder):
    """--assign map with several oligo files -> [the ErrorProfile of each group, None where no read was mapped to it]"""
    from . import helper
    from .decoder import Decoder
    from .read_map import MapIndex, read_oligo_files
    oligos, groups, names = read_oligo_files(a.oligos)
    with open(a.post_manifest) as f:
        paths = [ln.rstrip("\n").split("\t")[2] for ln in f if ln.strip()]
    own = decoder is None
    dec = Decoder(a.mem_conv, a.rate_conv, a.msg_len, list_size=a.list_size, max_deviation=a.max_deviation, device=a.device) if own else decoder
    totals, mapped, chimeric = [None] * len(names), 0, 0
    try:
        with MapIndex(oligos, groups=groups) as index:
            for k in range(0, len(paths), max(1, a.chunk)):
                with dec.resident([helper.read_post_file(p) for p in paths[k:k + max(1, a.chunk)]]) as (dev, off):
                    parts, res = profile_mapped(dec, dev, off, index, device=a.device, min_flank=int(index.lens.min()) // 2)
                mapped, chimeric = mapped + res.mapped, chimeric + int(res.chimeric.sum())
                totals = [p if t is None else t + p for t, p in zip(totals, parts)]
    finally:
        if own:
            dec.close()
    print("reads:", len(paths), "mapped:", mapped, "chimeric:", chimeric, file=out)
    for name, total in zip(names, totals):
        if total is None or total.reads == 0:
            print(name + ": aligned: 0", file=out)
            continue
        total.write_csv(a.out_prefix + "." + name)
        r = total.rates()
        print("%s: aligned: %d sub %.6f dele %.6f ins %.6f per reference base" % (name, total.reads, r["sub"], r["dele"], r["ins"]), file=out)
    return totals


if __name__ == "__main__":
    main()
