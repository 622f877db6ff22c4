"""CPU: a numpy model of fz_row_sums (telescope_amd/csrc/tsem_fused.h) — which lane of a 64-lane wave of quads issues which LDS atomic
with which sum — against a plain per-row sum, over every run pattern a wave can hold.

The rule the kernel follows (and `wave_atomics` restates, lane for lane, in the kernel's own order of operations):
  * inside a lane the products of equal neighbouring rows are summed left to right (s1, s2, s3);
  * a lane that lies wholly inside one run that comes in from the left (`open`) hands its sum on; the wave repeats the shift as often
    as its longest chain of open lanes is long;
  * F: a lane with a boundary inside sends the run in front of its FIRST boundary, plus what comes in from the left, to row r0;
  * X1 / X2: the runs behind the first boundary that end at entry 1 / entry 2 (lanes with two or three boundaries) — issued only in
    waves where some lane has one (the wave-uniform branch);
  * L: the run that ends with the lane's last entry, unless the right neighbour continues it.
The products are small integers, so every order of additions gives the same double and the comparison is exact."""
import itertools

import numpy as np

LANES = 64
IDLE_A, IDLE_B, NO_LEFT, NO_RIGHT = 0xFFFF, 0xFFFD, 0xFFFE, 0xFFFC     # the marks of fz_row_sums


def wave_atomics(rows, m, idle):
    """rows, m: [64][4]; idle: [64] bool.  Returns (list of (lane, tag, row, sum), fall-back taken, shift rounds)."""
    r0, r1, r2, r3 = rows.T
    m0, m1, m2, m3 = m.T
    e01, e12, e23 = r1 == r0, r2 == r1, r3 == r2
    n01, n12, n23 = ~e01, ~e12, ~e23
    multi = ((n01 & n12) | (n23 & (n01 | n12))) & ~idle
    s1 = np.where(e01, m0 + m1, m1)
    s2 = np.where(e12, s1 + m2, m2)
    s3 = np.where(e23, s2 + m3, m3)
    a = np.where(idle, IDLE_A, r0)
    b = np.where(idle, IDLE_B, r3)
    prev_b = np.concatenate([[NO_LEFT], b[:-1]])
    next_a = np.concatenate([a[1:], [NO_RIGHT]])
    joins = prev_b == a
    whole = e01 & e12 & e23
    opn = whole & joins
    run = s3.copy()                                           # I of the kernel
    chain = opn.copy()
    rounds = 0
    while chain.any():
        up = np.concatenate([[0.0], run[:-1]])
        run = np.where(opn, s3 + up, run)
        chain = chain & np.concatenate([[False], chain[:-1]])   # chain &= chain << 1
        rounds += 1
    left = np.concatenate([[0.0], run[:-1]])
    carry = np.where(joins, left, 0.0)
    first = np.where(e01, np.where(e12, s2, s1), m0)
    out = []
    for l in np.flatnonzero(~idle & ~whole):
        out.append((l, 'F', r0[l], first[l] + carry[l]))
    fallback = bool(multi.any())
    if fallback:
        for l in np.flatnonzero(~idle & n01 & n12):
            out.append((l, 'X1', r1[l], s1[l]))
        for l in np.flatnonzero(~idle & n23 & ~(e01 & e12)):
            out.append((l, 'X2', r2[l], s2[l]))
    for l in np.flatnonzero(~idle & (next_a != b)):
        out.append((l, 'L', r3[l], run[l]))
    return out, fallback, rounds, int(multi.sum())


def plain_row_sums(rows, m, idle, n_rows):
    want = np.zeros(n_rows)
    live = ~idle
    np.add.at(want, rows[live].ravel(), m[live].ravel())
    return want


def run_ends(rows, idle):
    """number of maximal runs of equal consecutive rows among the entries of the live lanes (a run never crosses an idle lane)"""
    n = 0
    flat = [(l, k) for l in range(LANES) if not idle[l] for k in range(4)]
    for i, (l, k) in enumerate(flat):
        last = i + 1 == len(flat) or flat[i + 1][0] not in (l, l + 1) or rows[flat[i + 1]] != rows[l, k]
        n += last
    return n


class Seen(object):
    def __init__(self):
        self.multi_lanes, self.rounds, self.tags, self.waves = set(), set(), set(), 0


def check(rows, idle, rng, seen, what):
    rows = np.asarray(rows, dtype=np.int64)
    idle = np.asarray(idle, dtype=bool)
    m = rng.randint(1, 1 << 20, size=(LANES, 4)).astype(np.float64)
    m[idle] = 0.0                                             # an idle lane is one whose four values are zeros
    n_rows = int(rows.max()) + 1
    atoms, fallback, rounds, n_multi = wave_atomics(rows, m, idle)
    got = np.zeros(n_rows)
    per_lane = np.zeros(LANES, dtype=int)
    for lane, tag, row, v in atoms:
        got[row] += v
        per_lane[lane] += 1
        seen.tags.add(tag)
    want = plain_row_sums(rows, m, idle, n_rows)
    assert np.array_equal(got, want), (what, np.flatnonzero(got != want)[:5])
    assert len(atoms) == run_ends(rows, idle), (what, 'one atomic per run end', len(atoms), run_ends(rows, idle))
    assert per_lane[idle].sum() == 0, (what, 'an idle lane issued an atomic')
    assert per_lane.max(initial=0) <= 4
    if not fallback:
        assert per_lane.max(initial=0) <= 2, (what, 'more than F and L without the fall-back')
    assert fallback == (n_multi > 0)
    seen.multi_lanes.add(n_multi)
    seen.rounds.add(rounds)
    seen.waves += 1


def rows_from(patterns, joins):
    """rows [64][4] from each lane's equality pattern (e01, e12, e23) and whether its first entry continues the left lane's last"""
    rows = np.zeros((LANES, 4), dtype=np.int64)
    r = 0
    for l in range(LANES):
        if l > 0 and not joins[l]:
            r += 1
        rows[l, 0] = r
        for k in range(3):
            if not patterns[l][k]:
                r += 1
            rows[l, k + 1] = r
    return rows


PATTERNS = list(itertools.product((False, True), repeat=3))


def test_every_lane_pattern_with_every_neighbourhood():
    """all 8 equality patterns of a lane x all 8 of its left and of its right neighbour x joined or not to either, at the wave's
    first lane, inside it, across its middle and at its last lane; the other lanes are drawn at random"""
    rng = np.random.RandomState(20)
    seen = Seen()
    none = np.zeros(LANES, dtype=bool)
    for pos in (0, 1, 32, 62, 63):
        for pl, pc, pr in itertools.product(PATTERNS, repeat=3):
            for jl, jr in itertools.product((False, True), repeat=2):
                pats = [PATTERNS[i] for i in rng.randint(0, 8, LANES)]
                joins = list(rng.random_sample(LANES) < 0.5)
                pats[pos] = pc
                joins[pos] = jl
                if pos > 0:
                    pats[pos - 1] = pl
                if pos < LANES - 1:
                    pats[pos + 1] = pr
                    joins[pos + 1] = jr
                check(rows_from(pats, joins), none, rng, seen, ('neighbourhood', pos, pl, pc, pr, jl, jr))
    assert seen.tags == {'F', 'X1', 'X2', 'L'}
    assert seen.waves == 5 * 512 * 4


def test_idle_lanes_at_the_tail():
    """0 .. 64 idle lanes at the end of the wave (the tail of a sub-block), after every pattern of the last live lane; an idle lane's
    index words are zeros (it lies past the sub-block's end) or whatever the quad held"""
    rng = np.random.RandomState(21)
    seen = Seen()
    for n_idle in range(LANES + 1):
        for pat in PATTERNS:
            for zeros in (True, False):
                pats = [PATTERNS[i] for i in rng.randint(0, 8, LANES)]
                joins = list(rng.random_sample(LANES) < 0.5)
                if n_idle < LANES:
                    pats[LANES - n_idle - 1] = pat
                rows = rows_from(pats, joins)
                idle = np.arange(LANES) >= LANES - n_idle
                if zeros:
                    rows[idle] = 0
                check(rows, idle, rng, seen, ('idle tail', n_idle, pat, zeros))
    assert 0 in seen.multi_lanes


def test_chains_of_open_lanes():
    """a run that spans 0 .. 63 whole lanes behind the lane it starts in (the shift loop iterates as often), starting at the first
    entry or inside lane 0, ending inside a lane, at a lane's end or at the wave's end"""
    rng = np.random.RandomState(22)
    seen = Seen()
    none = np.zeros(LANES, dtype=bool)
    for length in range(LANES):
        for start_inside in (False, True):
            for end in ('lane end', 'inside'):
                pats = [(False, False, False)] * LANES        # every other entry is a row of its own
                joins = [False] * LANES
                pats[0] = (False, True, True) if start_inside else (True, True, True)
                for l in range(1, length + 1):
                    pats[l], joins[l] = (True, True, True), True
                if end == 'inside' and length + 1 < LANES:
                    pats[length + 1], joins[length + 1] = (True, False, True), True
                check(rows_from(pats, joins), none, rng, seen, ('chain', length, start_inside, end))
    assert seen.rounds >= set(range(0, LANES)), sorted(set(range(LANES)) - seen.rounds)


def test_the_case_split_of_the_fall_back_is_covered():
    """no lane, exactly one lane and all 64 lanes with two or three boundaries inside; in between, every count of such lanes"""
    rng = np.random.RandomState(23)
    seen = Seen()
    none = np.zeros(LANES, dtype=bool)
    one = [p for p in PATTERNS if sum(not e for e in p) <= 1]
    many = [p for p in PATTERNS if sum(not e for e in p) >= 2]
    assert len(one) == 4 and len(many) == 4
    for n_multi in range(LANES + 1):
        for rep in range(8):
            lanes = rng.permutation(LANES)[:n_multi]
            pats = [one[i] for i in rng.randint(0, 4, LANES)]
            for l in lanes:
                pats[l] = many[rng.randint(0, 4)]
            joins = list(rng.random_sample(LANES) < 0.5)
            check(rows_from(pats, joins), none, rng, seen, ('fall-back', n_multi, rep))
    assert {0, 1, LANES} <= seen.multi_lanes, sorted(seen.multi_lanes)
    assert seen.multi_lanes == set(range(LANES + 1))


def test_any_entry_order_gives_the_row_sums():
    """the row order only makes the runs long: rows drawn at random (runs of one entry, rows that come back) still sum right"""
    rng = np.random.RandomState(24)
    seen = Seen()
    for rep in range(200):
        rows = rng.randint(0, 1 + rep % 7, size=(LANES, 4))
        idle = rng.random_sample(LANES) < 0.1
        # (run_ends counts maximal runs of consecutive equal rows, which is what the rule issues for any order)
        check(rows, idle, rng, seen, ('random order', rep))
