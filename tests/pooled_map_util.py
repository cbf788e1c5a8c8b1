"""What the pooled read-mapping tests share (tests/test_read_map_pooled_host.py, tests/test_gpu_read_map_pooled.py): a plain
full-matrix statement of read_map's definition to hold reference_map to, the nested-prefix index, the constructed chimeric
reads with the rows they must give, and three simulated pools of different codes."""
import numpy as np

N = 4
PREFIXES = (8, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1024)
NESTED = dict(k=8, max_occ=16, cands=8, min_votes=1)
UNMAPPED = [-1, -1, 0, -1, 0, 0, 0, -1]


def flip(read):
    return (3 - np.asarray(read, np.uint8))[::-1].astype(np.uint8)


def pack(reads):
    off = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.int64)
    return np.concatenate(list(reads) + [np.zeros(0, np.uint8)]).astype(np.uint8), np.stack([off[:-1], np.diff(off)], axis=1)


# ---------------------------------------------------------------- the definition, plainly

def full_matrix(ref, x, free):
    """D int32 [len(ref) + 1, len(x) + 1] of the unit-cost recurrence, D[i][0] = i, D[0][j] = 0 (free) or j; every cell from
    its three neighbours, an anti-diagonal at a time"""
    m, n = len(ref), len(x)
    D = np.zeros((m + 1, n + 1), np.int32)
    D[:, 0] = np.arange(m + 1)
    if not free:
        D[0] = np.arange(n + 1)
    cost = ((ref[:, None] != x[None, :]) | (ref[:, None] >= N) | (x[None, :] >= N)).astype(np.int32) if m and n else None
    for s in range(2, m + n + 1):
        i = np.arange(max(1, s - n), min(m, s - 1) + 1)
        j = s - i
        D[i, j] = np.minimum(np.minimum(D[i - 1, j] + 1, D[i, j - 1] + 1), D[i - 1, j - 1] + cost[i - 1, j - 1])
    return D


def plain_row(x, oligos, k, max_occ, cands, min_votes, max_dist):
    """one window of codes through the module docstring of read_map, with sets and full matrices -> the row as a list"""
    kmers = lambda c: [tuple(c[i:i + k]) for i in range(len(c) - k + 1)]
    held = [set(t for t in kmers(o.tolist()) if max(t) < N) for o in oligos]
    occ = {}
    for h in held:
        for t in h:
            occ[t] = occ.get(t, 0) + 1
    strands = (x, np.where(x < N, 3 - x, N).astype(np.uint8)[::-1])
    found = []
    for s in (0, 1):
        for o, h in enumerate(held):
            v = sum(1 for t in kmers(strands[s].tolist()) if t in h and occ[t] <= max_occ)
            if v >= min_votes:
                found.append((-v, s, o))
    found = sorted(found)[:cands]
    if not found:
        return list(UNMAPPED)
    last = [full_matrix(oligos[o], strands[s], True)[-1] for _, s, o in found]
    dist = [(int(row.min()), int(row.argmin())) for row in last]
    place = min(range(len(found)), key=lambda c: (dist[c][0], c))
    (d, e), (v, s, o) = dist[place], found[place]
    E = full_matrix(oligos[o][::-1], strands[s][:e][::-1], False)[-1]
    jp = int(np.argmax(E == d))
    assert E.min() == d
    others = [dist[c][0] for c in range(len(found)) if found[c][2] != o]
    return [o if d <= max_dist[o] else -1, o, s, d, e - jp if s == 0 else len(x) - e, jp, -v, min(others) if others else -1]


# ---------------------------------------------------------------- nested prefixes

def nested(longest, seed=11):
    """One random 1024-mer and its prefixes up to `longest` bases as one index, and per prefix p a read: junk, the prefix,
    junk -- the junk differs from the bases that would continue a match.  -> (oligos, reads, junk in front of each)"""
    rng = np.random.default_rng(seed)
    whole = rng.integers(0, 4, 1024).astype(np.uint8)
    lens = [p for p in PREFIXES if p <= longest]
    oligos = [whole[:p].copy() for p in lens]
    reads, front = [], []
    for p in lens:
        a = int(rng.integers(3, 12))
        tail = (whole[p:p + 9] + 1 + rng.integers(0, 3, len(whole[p:p + 9]))) % 4 if p < 1024 else rng.integers(0, 4, 9)
        head = rng.integers(0, 4, a)
        head[-1] = (whole[0] + 1) % 4
        reads.append(np.concatenate([head, whole[:p], tail]).astype(np.uint8))
        front.append(a)
    return oligos, reads, front


# ---------------------------------------------------------------- constructed chimeric reads

CHIM = dict(k=8, max_occ=64, cands=4, min_votes=2)
CHIM_LENS = (50, 61, 69)              # three groups; 61 and 69 lie on the two sides of a 64-row word


def chimeric_pool(seed=5):
    """4 oligos per group -> (oligos, groups)"""
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 4, m).astype(np.uint8) for m in CHIM_LENS for _ in range(4)], np.repeat(np.arange(3, dtype=np.int32), 4)


def spoil(oligo, edits):
    """`edits` substitutions well inside the oligo: the aligned part stays the whole copy"""
    o = oligo.copy()
    for e in range(edits):
        at = len(o) // 4 + e * (len(o) // 4)
        o[at] = (o[at] + 1) % 4
    return o


def chimeric_reads(seed=6):
    """-> (reads, want, want_supp): rows (ref, rc, dist, start, count) that the construction fixes, None for UNMAPPED.
    Every read is [junk a][X][junk b][Y][junk c] with X, Y copies of two oligos with 0 .. 2 substitutions, either strand, or a
    single oligo between junk.  The set is built for min_flank = MIN_FLANK."""
    rng = np.random.default_rng(seed)
    oligos, _ = chimeric_pool()
    junk = lambda n: rng.integers(0, 4, n).astype(np.uint8)
    reads, want, supp = [], [], []

    def part(o, edits, rc):
        c = spoil(oligos[o], edits)
        return flip(c) if rc else c

    def two(x, ex, rx, y, ey, ry, a, b, c):
        """X at a, Y behind b more; the part with fewer edits is the primary"""
        px, py = part(x, ex, rx), part(y, ey, ry)
        reads.append(np.concatenate([junk(a), px, junk(b), py, junk(c)]))
        rows = [(x, rx, ex, a, len(px)), (y, ry, ey, a + len(px) + b, len(py))]
        first = 0 if ex < ey else 1
        want.append(rows[first]); supp.append(rows[1 - first])

    def single(x, ex, rx, a, c):
        reads.append(np.concatenate([junk(a), part(x, ex, rx), junk(c)]))
        want.append((x, rx, ex, a, len(oligos[x]))); supp.append(None)

    two(0, 0, 0, 5, 1, 0, 7, 6, 9)            # X first, both forward, lengths 50 and 61
    single(2, 1, 0, 12, 20)                   # not chimeric: junk flanks shorter than MIN_FLANK
    two(9, 2, 1, 4, 1, 0, 3, 11, 4)           # Y is the primary: the flank is the left one; X is a reverse strand of 69 bases
    two(6, 1, 1, 10, 2, 1, 0, 0, 0)           # no junk at all: the right flank is Y exactly, both reverse strands
    single(11, 0, 1, 0, 0)                    # the whole read is the oligo: both flanks empty
    two(3, 0, 0, 8, 2, 0, 14, 2, 30)          # Y of 69 bases forward
    # the boundary: the right flank is Y's 50 bases and nothing else = MIN_FLANK; with MIN_FLANK + 1 there is no pass
    two(7, 0, 0, 1, 1, 1, 20, 0, 0)
    # equal flanks: Y and Z of 61 bases on both sides of an exact X, one substitution each; the left one is taken
    py, pz = part(4, 1, 0), part(5, 1, 1)
    reads.append(np.concatenate([py, part(8, 0, 0), pz]))
    want.append((8, 0, 0, 61, 69)); supp.append((4, 0, 1, 0, 61))
    single(1, 2, 1, 30, 49)                   # a junk flank of MIN_FLANK - 1 bases: no pass
    single(1, 2, 0, 30, 50)                   # a junk flank of MIN_FLANK bases: a pass that finds nothing
    return reads, want, supp


MIN_FLANK = 50


def expect(res_out, rows):
    """the rows that a construction fixes against out"""
    for r, row in enumerate(rows):
        got = res_out[r].tolist()
        if row is None:
            assert got == UNMAPPED, (r, got)
        else:
            o, rc, d, start, count = row
            assert got[:6] == [o, o, rc, d, start, count], (r, got, row)


# ---------------------------------------------------------------- three simulated pools

POOLS = (((6, 1, 60), 9), ((6, 1, 72), 7), ((8, 1, 64), 8))          # (mem_conv, rate, msg_len), messages
SET = dict(sub=0.02, dele=0.02, ins=0.01)                            # the channel of tests/test_read_map_host.py's recovery test


def simulated_pools(seed, reads_each=70):
    """-> dict(oligos, groups, bases, win, source (the oligo's number in the merged set), rc, group)"""
    from nanopore_dna_storage_amd import simulate as S
    from nanopore_dna_storage_amd.decoder import encode
    rng = np.random.default_rng(seed)
    oligos, groups, parts, wins, source, rc, group = [], [], [], [], [], [], []
    at = 0
    for g, (code, n_msgs) in enumerate(POOLS):
        pool = rng.integers(0, 2, size=(n_msgs, code[2]), dtype=np.uint8)
        ref = S.reference_reads(*code, reads_each, seed + g, scores=False, pool=pool, rc_mode=3, **SET)
        off = ref["base_offsets"]
        parts.append(ref["bases"])
        wins.append(np.stack([off[:-1] + at, np.diff(off)], axis=1))
        at += len(ref["bases"])
        source.append(ref["source"] + len(oligos))
        rc.append(ref["rc"].astype(np.int32))
        group.append(np.full(reads_each, g, np.int32))
        oligos += list(encode(*code, pool))
        groups += [g] * n_msgs
    return dict(oligos=oligos, groups=np.array(groups, np.int32), bases=np.concatenate(parts), win=np.concatenate(wins),
                source=np.concatenate(source), rc=np.concatenate(rc), group=np.concatenate(group))
