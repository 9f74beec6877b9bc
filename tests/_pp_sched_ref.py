"""Dependence model of the persistent factorisation's task list (gladsgp_amd/csrc/chol.hip).

Written from what the kernel's workgroups wait on -- the flag reads of pp_term / pp_worker (worker
tasks) and pp_chain (the chain) and the stores of pp_zero -- not from pp_for_key, which decides
the order: the model takes ANY list and says whether it is complete and whether workgroups that
dequeue it strictly in order can all end up waiting on tasks nobody has dequeued.

Tiles are 64 x 64, N tile rows.  Per problem the flags are L(i, j) (i >= j), X(i, c) (i > c),
DP(j) and SP(j).  What a task waits for, and what it then sets:

  LT(i, j)    L(i, t), L(j, t) for t < j, then L(j, j)                          -> L(i, j)
  DP(j)       L(j, t) for t < j - 1                                             -> DP(j)
  SP(j)       L(j+1, t), L(j, t) for t < j        (the entry carries i = j + 1) -> SP(j)
  XT(i, c)    for k = c .. i-1: L(i, k) and X(k, c), at k = c L(c, c) instead;
              then L(i, i)                                                      -> X(i, c)
  XT2(i, c)   the same and X(k, c+1) for k > c + 1, L(c+1, c+1) at k = c + 1    -> X(i, c), X(i, c+1)
  Z, ZP       nothing (they zero tiles no task writes)
  chain       step j = 0 .. N-1: waits DP(j) when j >= 2 -> L(j, j); then, when j <= N - 2,
              waits SP(j) when j >= 1 -> L(j+1, j)

A list is an int array of rows (kind, b, i, j); `triples` are one problem's (kind, i, j).
"""
import numpy as np

CHAIN, LT, DP, SP, XT, Z, XT2, ZP = range(8)
ZRUN = 8        # pp_zero: a Z task zeroes up to 8 tile rows of one tile column, a ZP task the
#                 padding tile row over up to 8 tile columns


def padded_tiles(N):
    """Tile rows of the padded L^-1 buffer (padded to a multiple of 128 = two tiles)."""
    return (N + 1) & ~1


# ---- lists -----------------------------------------------------------------------------------

def batched(triples, batch):
    """The documented list of a batch: the chain entries of b = 0 .. batch-1, then each task of
    the per-problem order in turn for b = 0 .. batch-1."""
    t = np.asarray(triples, dtype=np.int64).reshape(-1, 3)
    T = len(t)
    out = np.zeros((batch * (T + 1), 4), dtype=np.int64)
    out[:batch, 1] = np.arange(batch)
    body = out[batch:].reshape(T, batch, 4)
    body[:, :, 0] = t[:, None, 0]
    body[:, :, 1] = np.arange(batch)[None, :]
    body[:, :, 2] = t[:, None, 1]
    body[:, :, 3] = t[:, None, 2]
    return out


def single(triples):
    """One problem's tasks as list rows (b = 0), without a chain entry."""
    t = np.asarray(triples, dtype=np.int64).reshape(-1, 3)
    out = np.zeros((len(t), 4), dtype=np.int64)
    out[:, 0], out[:, 2], out[:, 3] = t[:, 0], t[:, 1], t[:, 2]
    return out


def field_errors(entries):
    """Fields that do not fit the list's encoding (kind | b << 4, i | j << 16 in 32-bit ints)."""
    e = np.asarray(entries, dtype=np.int64).reshape(-1, 4)
    errs = []
    if len(e) and (e.min() < 0):
        errs.append("negative field")
    if len(e) and e[:, 0].max() >= 16:
        errs.append("kind >= 16")
    if len(e) and e[:, 1].max() >= 1 << 27:
        errs.append("b >= 2^27")
    if len(e) and max(e[:, 2].max(), e[:, 3].max()) >= 1 << 16:
        errs.append("i or j >= 2^16")
    return errs


def encode(entries):
    """The int32 words of a list as it sits in the scratch: (kind | b << 4, i | j << 16)."""
    e = np.asarray(entries, dtype=np.int64).reshape(-1, 4)
    assert not field_errors(e)
    return np.stack([e[:, 0] | (e[:, 1] << 4), e[:, 2] | (e[:, 3] << 16)], axis=1).astype(np.int32)


def decode(words):
    w = np.asarray(words, dtype=np.int64).reshape(-1, 2)
    return np.stack([w[:, 0] & 15, w[:, 0] >> 4, w[:, 1] & 0xffff, w[:, 1] >> 16], axis=1)


def layout_errors(entries, batch, groups):
    """A batched list's layout: every entry of problem b at an index congruent to b mod batch,
    and with `groups` queues (queue g = entries groups * k + g) only the problems b % groups == g
    in queue g."""
    e = np.asarray(entries, dtype=np.int64).reshape(-1, 4)
    idx = np.arange(len(e))
    errs = []
    if np.any(idx % batch != e[:, 1]):
        errs.append("an entry of problem b is not at an index = b mod batch")
    if np.any(e[:, 1] >= batch):
        errs.append("b >= batch")
    if groups > 1 and np.any(idx % groups != e[:, 1] % groups):
        errs.append("a queue holds a problem of another queue")
    return errs


# ---- completeness ----------------------------------------------------------------------------

def complete_errors(triples, N, inv):
    """What one problem's list lacks, repeats or should not hold (empty: complete).

    Exactly once each: L(i, j) for i >= j + 2, DP(2 .. N-1), SP(1 .. N-2), with inv X(i, c) for
    i > c and a zero task over every upper tile (r < c < NT) and the padding tile row; nothing
    else; every field within its encoding."""
    t = np.asarray(triples, dtype=np.int64).reshape(-1, 3)
    errs = list(field_errors(single(t)))
    kind, I, J = t[:, 0], t[:, 1], t[:, 2]
    NT = padded_tiles(N)

    def count(shape, rows, cols):
        c = np.zeros(shape, dtype=np.int64)
        np.add.at(c, (rows, cols), 1)
        return c

    def report(name, got, want):
        for r, c in np.argwhere((got == 0) & (want == 1))[:3]:
            errs.append(f"missing {name}({r}, {c})")
        for r, c in np.argwhere(got > want)[:3]:
            errs.append(f"{name}({r}, {c}) produced {got[r, c]} times, expected {want[r, c]}")

    other = ~np.isin(kind, [LT, DP, SP, XT, XT2, Z, ZP])
    if other.any():
        errs.append(f"unexpected kind {kind[other][0]}")
    ii, jj = np.indices((N, N))
    # L tiles of the workers
    m = kind == LT
    bad = m & ~((J >= 0) & (I >= J + 2) & (I < N))
    if bad.any():
        errs.append(f"malformed LT({I[bad][0]}, {J[bad][0]})")
    m &= ~bad
    report("L", count((N, N), I[m], J[m]), (ii >= jj + 2).astype(np.int64))
    # the chain's partial sums
    for k, name, lo, hi in ((DP, "DP", 2, N - 1), (SP, "SP", 1, N - 2)):
        m = kind == k
        bad = m & ~((J >= lo) & (J <= hi))
        if k == SP:
            bad |= m & (I != J + 1)
        if bad.any():
            errs.append(f"malformed {name}({I[bad][0]}, {J[bad][0]})")
        m &= ~bad
        want = ((np.arange(N) >= lo) & (np.arange(N) <= hi)).astype(np.int64)
        report(name, count((1, N), np.zeros(m.sum(), dtype=np.int64), J[m]), want[None, :])
    # L^-1 tiles
    m1, m2 = kind == XT, kind == XT2
    bad = (m1 & ~((J >= 0) & (I > J) & (I < N))) | (m2 & ~((J >= 0) & (I > J + 1) & (I < N)))
    if bad.any():
        errs.append(f"malformed XT({I[bad][0]}, {J[bad][0]})")
    m1 &= ~bad
    m2 &= ~bad
    got = count((N, N), np.concatenate([I[m1], I[m2], I[m2]]),
                np.concatenate([J[m1], J[m2], J[m2] + 1]))
    report("X", got, (ii > jj).astype(np.int64) * (1 if inv else 0))
    # zeroed tiles
    cover = np.zeros((NT, NT), dtype=np.int64)
    for k, i, j in t[(kind == Z) | (kind == ZP)].tolist():
        if k == Z and 0 <= j < i < NT:
            cover[j:min(j + ZRUN, i), i] += 1
        elif k == ZP and NT > N and j == 0 and 0 <= i < NT:
            cover[N:NT, i:min(i + ZRUN, NT)] += 1
        else:
            errs.append(f"malformed zero task ({k}, {i}, {j})")
    ri, ci = np.indices((NT, NT))
    want = ((ri < ci) | (ri >= N)).astype(np.int64) * (1 if inv else 0)
    report("zero", cover, want)
    return errs


# ---- the dependence model --------------------------------------------------------------------

def _reads(kind, i, j, N):
    """The flags a worker task waits for, as (start, stop, step) runs of flag indices:
    L(i, j) at i N + j, X(i, c) at N^2 + i N + c, DP(j) at 2 N^2 + j, SP(j) at 2 N^2 + N + j."""
    if kind == LT:
        return ((i * N, i * N + j, 1), (j * N, j * N + j + 1, 1))
    if kind == DP:
        return ((j * N, j * N + j - 1, 1),)
    if kind == SP:
        return ((i * N, i * N + j, 1), (j * N, j * N + j, 1))
    c, NN = j, N * N
    r = [(i * N + c, i * N + i, 1), (c * N + c, c * N + c + 1, 1)]
    if i - c >= 2:
        r.append((NN + (c + 1) * N + c, NN + (i - 1) * N + c + 1, N))
    if kind == XT2:
        c1 = c + 1
        r.append((c1 * N + c1, c1 * N + c1 + 1, 1))
        if i - c1 >= 2:
            r.append((NN + (c1 + 1) * N + c1, NN + (i - 1) * N + c1 + 1, N))
    r.append((i * N + i, i * N + i + 1, 1))
    return r


def _writes(kind, i, j, N):
    if kind == LT:
        return (i * N + j,)
    if kind == DP:
        return (2 * N * N + j,)
    if kind == SP:
        return (2 * N * N + N + j,)
    if kind == XT:
        return (N * N + i * N + j,)
    return (N * N + i * N + j, N * N + i * N + j + 1)


def _well_formed(kind, i, j, N):
    if kind == LT:
        return 0 <= j and j + 2 <= i < N
    if kind == DP:
        return 2 <= j < N
    if kind == SP:
        return 1 <= j and i == j + 1 and i < N
    if kind == XT:
        return 0 <= j < i < N
    if kind == XT2:
        return 0 <= j and j + 1 < i < N
    return kind in (CHAIN, Z, ZP)


class Profile:
    """stuck[k-1], blocked[k-1] for the prefix of the first k entries: the dequeued worker tasks
    that cannot complete from what that prefix (and the chains dequeued in it) can produce, and
    the same plus the dequeued chains that cannot finish.  Workgroups that dequeue the list in
    order all end up holding such an entry, with nobody left to dequeue what they wait for,
    exactly when blocked >= their number for some prefix.  While every chain is unfinished that is
    stuck >= G - B for G workgroups and B chains."""

    def __init__(self, stuck, blocked):
        self.stuck = np.asarray(stuck, dtype=np.int64)
        self.blocked = np.asarray(blocked, dtype=np.int64)
        self.max_stuck = int(self.stuck.max()) if len(self.stuck) else 0
        self.max_blocked = int(self.blocked.max()) if len(self.blocked) else 0
        self.final_blocked = int(self.blocked[-1]) if len(self.blocked) else 0

    def deadlocks(self, workgroups):
        return self.max_blocked >= workgroups


def profile(entries, N, chains_running=False):
    """The Profile of a list.  chains_running: every problem's chain runs from the start (for one
    problem's tasks listed without its chain entry); else a chain starts at its entry."""
    ents = np.asarray(entries, dtype=np.int64).reshape(-1, 4).tolist()
    NN = N * N
    R = 2 * NN + 2 * N
    DPo, SPo = 2 * NN, 2 * NN + N
    avail, waiters, chain = {}, {}, {}      # per problem; chain: [next step, phase, started]
    stuck = unfinished = 0
    out_s, out_b = [], []

    def state(b):
        if b not in avail:
            avail[b] = bytearray(R)
            waiters[b] = {}
            chain[b] = [0, 0, False]
        return avail[b]

    def advance(b, produced):
        """Run problem b's chain as far as its flags allow."""
        nonlocal unfinished
        av, ch = avail[b], chain[b]
        if not ch[2] or ch[0] >= N:
            return
        while ch[0] < N:
            j = ch[0]
            if ch[1] == 0:
                if j >= 2 and not av[DPo + j]:
                    return
                produced.append(j * N + j)
                av[j * N + j] = 1
                ch[1] = 1
            if j <= N - 2:
                if j >= 1 and not av[SPo + j]:
                    return
                produced.append((j + 1) * N + j)
                av[(j + 1) * N + j] = 1
            ch[0], ch[1] = j + 1, 0
        unfinished -= 1

    def settle(b, todo, produced):
        """Complete what can complete: `todo` tasks to (re)examine, `produced` flags just set."""
        nonlocal stuck
        av, wt = avail[b], waiters[b]
        while todo or produced:
            while produced:
                todo.extend(wt.pop(produced.pop(), ()))
            if not todo:
                break
            task = todo.pop()
            kind, i, j = task
            missing = -1
            for a, z, st in _reads(kind, i, j, N):
                p = av[a:z:st].find(0)
                if p >= 0:
                    missing = a + p * st
                    break
            if missing >= 0:
                wt.setdefault(missing, []).append(task)
                continue
            stuck -= 1
            for w in _writes(kind, i, j, N):
                if not av[w]:
                    av[w] = 1
                    produced.append(w)
            if kind in (DP, SP):
                advance(b, produced)

    for kind, b, i, j in ents:
        if not _well_formed(kind, i, j, N):
            raise ValueError(f"malformed task ({kind}, {i}, {j}) at N = {N}")
        state(b)
        if chains_running and not chain[b][2]:
            chain[b][2] = True
            unfinished += 1
            produced = []
            advance(b, produced)
            settle(b, [], produced)
        if kind == CHAIN:
            if not chain[b][2]:
                chain[b][2] = True
                unfinished += 1
                produced = []
                advance(b, produced)
                settle(b, [], produced)
        elif kind not in (Z, ZP):
            stuck += 1
            settle(b, [(kind, i, j)], [])
        out_s.append(stuck)
        out_b.append(stuck + unfinished)
    return Profile(out_s, out_b)


def queue_profiles(entries, N, groups):
    """One Profile per dequeue queue: queue g holds the entries groups * k + g."""
    e = np.asarray(entries, dtype=np.int64).reshape(-1, 4)
    return [profile(e[g::groups], N) for g in range(groups)]


def launch_deadlocks(entries, N, grid, groups):
    """Whether `grid` workgroups, workgroup w dequeuing queue w % groups in order, can all end up
    waiting (grid % groups == 0 with more than one queue)."""
    assert groups == 1 or grid % groups == 0
    return any(p.deadlocks(grid // groups) for p in queue_profiles(entries, N, groups))
