"""The "fill" insert policy (cdlrm_plan_assign_fill) restated in numpy, one table at a time, plus the
reference policy's collision rule for the CPU controls, and the inputs the host and the GPU tests share.

Contract (per window, per table, after the probe):
  * count[u] = lookups of uniq[u] in the window; priority = min(count, 65535); out-of-range ids count nowhere;
  * a claimant is a unique index that missed and whose set has an unprotected way (a way no index of the window hits);
  * inside a set the claimants are ordered by priority descending, then index ascending;
  * the set's free ways are its unprotected ways, empty ones (tag -1) first, then occupied ones, each ascending;
  * the claimant of rank r takes the r-th free way; rank >= number of free ways: not inserted.
Nothing here reads the GPU code or the reference tree."""
import numpy as np

CLAMP = 65535


def window_counts(uniq, row, n_rows):
    """Lookups of every entry of the sorted list `uniq` in `row`; ids outside [0, n_rows) or not in the list count nowhere."""
    row = np.asarray(row, dtype=np.int64)
    row = row[(row >= 0) & (row < n_rows)]
    cnt = np.zeros(len(uniq), dtype=np.int64)
    if len(uniq) == 0 or len(row) == 0:
        return cnt
    pos = np.searchsorted(uniq, row)
    pos[pos == len(uniq)] = 0
    ok = uniq[pos] == row
    np.add.at(cnt, pos[ok], 1)
    return cnt


def probe(tags, uniq):
    """-> (hit [U] bool, prot [P, ways] bool): which unique indices are cached, which ways this window hits."""
    P = tags.shape[0]
    hit = (tags[uniq % P] == uniq[:, None]).any(axis=1) if len(uniq) else np.zeros(0, dtype=bool)
    prot = np.isin(tags, uniq) & (tags != -1)          # (a tag lives in set tag % P: the match is in the index's own set)
    return hit, prot


def claimants(tags, uniq):
    """-> (hit, prot, kept): kept = positions into uniq of the claimants, ascending."""
    hit, prot = probe(tags, uniq)
    P = tags.shape[0]
    has_free = ~prot.all(axis=1)
    kept = np.nonzero(~hit & has_free[uniq % P])[0]
    return hit, prot, kept


def free_way_order(tags, prot, occupied_first=False):
    """-> (order [P, ways]: the set's free ways in the order they are handed out, then the others; nfree [P])."""
    ways = tags.shape[1]
    avail = ~prot
    empty = tags == -1
    first, second = (avail & ~empty, avail & empty) if occupied_first else (avail & empty, avail & ~empty)
    cls = np.where(first, 0, np.where(second, 1, 2))
    order = np.argsort(cls * ways + np.arange(ways)[None, :], axis=1, kind="stable")
    return order, avail.sum(axis=1)


def plan_fill(tags, uniq, counts=None, *, clamp=True, occupied_first=False):
    """One table's plan under the fill policy.  tags [P, ways] int64, uniq sorted int64, counts [U] or None (all equal).
    -> dict(hit, kept, placed [M] bool, way [M] (the way of a placed claimant; -1 otherwise), nfree_of [M] ...)."""
    P, ways = tags.shape
    hit, prot, kept = claimants(tags, uniq)
    idx = uniq[kept]
    sets = idx % P
    pri = np.zeros(len(kept), dtype=np.int64) if counts is None else np.asarray(counts, dtype=np.int64)[kept]
    if clamp:
        pri = np.minimum(pri, CLAMP)
    o = np.lexsort((idx, -pri, sets))                  # by set, then priority descending, then index ascending
    s_sorted = sets[o]
    start = np.searchsorted(s_sorted, s_sorted, side="left")
    rank = np.empty(len(kept), dtype=np.int64)
    rank[o] = np.arange(len(kept)) - start
    order, nfree = free_way_order(tags, prot, occupied_first)
    placed = rank < nfree[sets]
    way = np.full(len(kept), -1, dtype=np.int64)
    way[placed] = order[sets[placed], rank[placed]]
    return dict(hit=hit, prot=prot, kept=kept, idx=idx, sets=sets, placed=placed, way=way, nfree=nfree,
                expected_inserts=int(np.minimum(np.bincount(sets, minlength=P), nfree).sum()))


def plan_reference(tags, uniq, rng):
    """The reference's rule: every claimant draws one of its set's unprotected ways uniformly (here: from `rng`); a
    contested slot goes to the claimant latest in ascending-index order."""
    P, ways = tags.shape
    hit, prot, kept = claimants(tags, uniq)
    idx = uniq[kept]
    sets = idx % P
    avail = ~prot
    nfree = avail.sum(axis=1)
    asc = np.argsort(np.where(avail, 0, 1) * ways + np.arange(ways)[None, :], axis=1, kind="stable")
    pick = (rng.random_sample(len(kept)) * nfree[sets]).astype(np.int64)
    way = asc[sets, pick] if len(kept) else np.zeros(0, dtype=np.int64)
    slot = sets * ways + way
    last = np.full(P * ways, -1, dtype=np.int64)
    np.maximum.at(last, slot, np.arange(len(kept)))
    placed = last[slot] == np.arange(len(kept)) if len(kept) else np.zeros(0, dtype=bool)
    return dict(hit=hit, prot=prot, kept=kept, idx=idx, sets=sets, placed=placed, way=np.where(placed, way, -1), nfree=nfree)


def commit(tags, plan):
    """Apply a plan to `tags` in place.  -> (winner claimant ids ascending, evicted tag per winner, -1 = the way was empty)."""
    w = np.nonzero(plan["placed"])[0]
    s, y = plan["sets"][w], plan["way"][w]
    assert len(np.unique(s * tags.shape[1] + y)) == len(w), "a slot was claimed twice"
    old = tags[s, y].copy()
    tags[s, y] = plan["idx"][w]
    return w, old


def victims(plan, U):
    """Positions into uniq that stay outside the cache after the commit."""
    out = ~plan["hit"]
    out[plan["kept"][plan["placed"]]] = False
    return np.nonzero(out)[0]


def lookup_hits(tags, row):
    """Lookups of `row` that are resident in `tags`."""
    P = tags.shape[0]
    row = np.asarray(row, dtype=np.int64)
    return int((tags[row % P] == row[:, None]).any(axis=1).sum())


# ---- the inputs the bit-exact GPU test runs, shared with the host controls ------------------------------------------

LN_EMB = [7, 1000, 20011]
SETS = [7, 53, 211]
# The four counts of the clamp case add up to 266 605 lookups of ONE table, so the rectangle is [3, 300 000] (the next round
# figure above that sum), not ~210 000.
N_WIN = 300_000
CLAMP_COUNTS = [65534, 65535, 65536, 70000]     # in ascending index order: with the clamp the last three tie and go in index
CLAMP_SET = 5                                   # order, the smallest index (65 534) last; without it the order is by count


def clamp_indices():
    P = SETS[2]
    return [CLAMP_SET + P * k for k in (3, 11, 40, 77)]


def initial_tags(ways, seed=7):
    """Table 0 fully resident (its windows are all hits), tables 1 and 2 with about a third of the ways occupied."""
    rng = np.random.RandomState(seed + ways)
    out = []
    for k, (n, P) in enumerate(zip(LN_EMB, SETS)):
        tags = np.full((P, ways), -1, dtype=np.int64)
        if k == 0:
            for v in range(n):
                tags[v % P, v % ways] = v
        else:
            per_set = (n - 1) // P                      # every set has at least this many indices
            for s in range(P):
                nocc = min(int(rng.binomial(ways, 0.35)), per_set)
                res = s + P * rng.choice(per_set, size=nocc, replace=False)
                tags[s, rng.choice(ways, size=nocc, replace=False)] = res
            if k == 2:                                  # the clamp case's set starts empty: its indices are all claimants
                tags[CLAMP_SET, :] = -1
        out.append(tags)
    return out


def windows(nwin=3, seed=21):
    """nwin rectangles [3, N_WIN]: Zipf and uniform lookups mixed (uniques of table 2 well above its slots at few ways);
    table 2 of window 0 holds the clamp case; table 0 (7 rows, all resident) only ever hits."""
    rng = np.random.RandomState(seed)
    out = []
    ci = clamp_indices()
    for w in range(nwin):
        rows = []
        for k, n in enumerate(LN_EMB):
            z = (rng.zipf(1.2, size=N_WIN).astype(np.int64) * 2654435761) % n
            # the uniform half draws from a subset of the rows that changes with the window: residents the next window does
            # not read leave occupied ways free, so windows 1 and 2 evict
            sub = np.sort(rng.permutation(n)[:max(1, int(n * 0.45))]) if k else np.arange(n)
            u = sub[rng.randint(0, len(sub), size=N_WIN)].astype(np.int64)
            row = np.where(rng.random_sample(N_WIN) < 0.5, z, u)
            if k == 2:
                clash = np.isin(row, ci)
                row[clash] = (row[clash] + 1) % n       # (index + 1 lies in the next set: never another clamp index)
                if w == 0:
                    at = rng.permutation(N_WIN)[:sum(CLAMP_COUNTS)]
                    row[at] = np.repeat(ci, CLAMP_COUNTS)
            rows.append(row)
        out.append(np.stack(rows))
    return out


def run_windows(tags, wins, ln_emb=LN_EMB, use_counts=True, **variant):
    """The restated fill policy over consecutive windows, every table.  tags: list of [P, ways] (changed in place).
    -> per window and table: dict(uniq, plan, winners, evicted, victims, tags after the commit)."""
    out = []
    for win in wins:
        per = []
        for k, tg in enumerate(tags):
            row = win[k]
            uniq = np.unique(row)
            plan = plan_fill(tg, uniq, window_counts(uniq, row, ln_emb[k]) if use_counts else None, **variant)
            w, old = commit(tg, plan)
            per.append(dict(uniq=uniq, plan=plan, winners=w, evicted=old, victims=victims(plan, len(uniq)), tags=tg.copy()))
        out.append(per)
    return out
