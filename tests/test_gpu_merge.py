"""GPU tests of the top-K merge kernels alone (bote_merge.hip: merge_wide_kernel,
merge_kernel, pick_counters_kernel), through the library's test entry
bote_test_merge (not part of the ABI): the caller supplies every record slot
of every input list and gets back all KP slots of every result list and the
result's two counters.

Every sweep, batch, shard merge and evolve level reports through these
kernels, and a wrong slot or a dropped record shows only as one entry missing
from some top-K, so they are checked here directly against a sort.  The
contract pinned (DESIGN.md §4 "Merge kernels, direct"): the input lists are
sorted by (key, rank) and end at a REC_MAX terminator or hold K records
(whatever follows the terminator is stale memory); kbound[o] is at least the
union's K-th key; the output is the K least records of the union in (key,
rank) order, padded to KP slots with REC_MAX.  The merge tree's kernel reads
whole lists (KP slots, padded with REC_MAX) and keeps the KP least, whatever
K is; equal records in two lists are a multiset there and both are kept (the
one-launch merge takes distinct records: configs of distinct blocks).

Expected values come from numpy.lexsort by (key, rank), never from the model
(tests/test_merge_model.py); the model only asserts that a case reaches the
path its name claims (head_bound, prefix_counts, wide_select).  One launch
carries up to 8 objectives with one key pattern each, which also checks the
o * KP indexing and the list stride.  Stale slots hold records below every
real record: one read as a record comes out first.

Two edits of the kernels that no output can show (both were run against this
file and pass, as they must).  Exchanging upper_bound_rec and lower_bound_rec
in merge_kernel's rank loop only reverses the order of equal records among
themselves: records are (key, rank) and nothing else, so the slots hold the
same values.  Making both calls lower_bound_rec puts equal records into one
slot and fails every tree case here.  Dropping `c == i` from the heads'
kept-prefix count changes it only for an empty list followed by a stale
record that passes the key tests, and the head then visited is slot 0, the
terminator itself: with WIDE_HEAD = 2 that adds (REC_MAX) heads above every
real head, which leaves the K-th least head, or the absence of a bound, as it
was.  What keeps stale records out of the result is the prefix count's `go`
chain; letting it run on (`go = true`) fails the fill and list-count cases."""
import ctypes as C
import random

import numpy as np
import pytest

from fantoch_amd import _lib
from tests.test_merge_model import (ONES, REC_MAX, WIDE_FEW, WIDE_HEAD, WIDE_RANK_MAX, WIDE_SLACK, block_lists, dump,
                                    head_bound, prefix_counts, wide_select)

pytestmark = pytest.mark.gpu

KP = _lib.KP
WIDE_SORT = 4096  # bote_merge.hip: the windowed path sorts K running + (WIDE_SORT - K) gathered records
WIDE_MERGE_LISTS = 4096  # bote_kernels.hpp: more lists take the tree
CHAIN, WIDE, LEVEL = 0, 1, 2  # bote_test_merge's modes
U = np.uint64
RANK0 = 2**20  # real ranks start here: the stale records' ranks lie below

# one key pattern per objective (the model's seed_rows patterns, on records)
PATTERNS = ["means", "cov", "equal", "ties5", "extremes", "low_bit", "nan_tail", "ties_wide"]


def keys_of(pattern, n, K, rng):
    if pattern == "means":  # sums of latencies, below 2^21, with ties
        return rng.normal(40000, 3000, n).astype(np.int64).clip(0, 2**21 - 1).astype(U)
    if pattern == "cov":  # bits of positive f64 values: spread over more than 2^62
        return (10.0 ** rng.uniform(-300, 300, n)).view(U)
    if pattern == "equal":  # the ranks decide (wide_select's mx == mn)
        return np.full(n, 40000, U)
    if pattern == "ties5":  # heavy ties: the select walks every digit down to the key, then the ranks
        return rng.choice(np.array([1000, 1001, 1003, 1010, 2**40], U), n)
    if pattern == "extremes":  # a range of 2^64 - 2: the first pass has no prefix (s_hi == 64)
        return rng.choice(np.array([0, 2**63, ONES - 1], U), n)
    if pattern == "low_bit":  # distinct even keys 2^20 apart, the (K+1)-th least = the K-th least | 1
        k = np.arange(n, dtype=U) * U(2**20) + U(24690)
        if n > K:
            k[K] = k[K - 1] | U(1)
        rng.shuffle(k)
        return k
    if pattern == "nan_tail":  # NaN-COV keys (all ones, real ranks) at the lists' tails beside real keys
        k = rng.normal(40000, 3000, n).astype(np.int64).clip(0).astype(U)
        return np.where(rng.random(n) < 0.2, U(ONES), k)
    if pattern == "ties_wide":  # heavy ties 2^12 apart: a tie class of <= WIDE_FEW heads ends in the small-bin finish
        return rng.choice(np.array([1000, 5096, 9192, 13288, 2**40], U), n)
    raise ValueError(pattern)


def ranks_of(pattern, n, rng):
    """Distinct ranks >= RANK0.  Tied patterns: a dense cluster with a tenth of
    the ranks 2^41 below it, so a rank select over them spans more than 2^40
    and its first digit's bin holds nearly all of them; else spread over
    n * 2^42."""
    p = rng.permutation(n).astype(U)
    if pattern in ("equal", "ties5", "ties_wide"):
        return p + U(RANK0) + np.where(rng.random(n) < 0.1, U(0), U(2**41))
    return p * U(2**42) + rng.integers(0, 2**42, n, dtype=U) + U(RANK0)


def records(pattern, n, K, rng):
    return np.stack([keys_of(pattern, n, K, rng), ranks_of(pattern, n, rng)], axis=1)


def sorted_fill(ids, n_ids, recs, cap):
    """out[i] = the `cap` least (key, rank) records with id i (numpy.lexsort),
    padded with REC_MAX; also each id's record count."""
    out = np.full((n_ids, cap, 2), U(ONES))
    order = np.lexsort((recs[:, 1], recs[:, 0], ids))
    ids, recs = ids[order], recs[order]
    start = np.searchsorted(ids, np.arange(n_ids))
    pos = np.arange(len(ids)) - start[ids]
    k = pos < cap
    out[ids[k], pos[k]] = recs[k]
    return out, np.bincount(ids, minlength=n_ids)


def k_least(recs, K):
    """The sort: the K least of `recs` by (key, rank), padded to KP slots."""
    out, _ = sorted_fill(np.zeros(len(recs), np.int64), 1, recs, K)
    return np.concatenate([out[0], np.full((KP - K, 2), U(ONES))])


def stale_block(n_lists, n_obj):
    """Slots nobody fills: records (0, slot), below every real record."""
    buf = np.zeros((n_lists, n_obj, KP, 2), U)
    buf[..., 1] = np.arange(KP, dtype=U)
    return buf


def tuples(a):
    return list(map(tuple, a.tolist()))


_ARGTYPES = [C.c_int, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
             C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]


def merge(mode, src, K, alt=None, kbound=None, sel=None, cap=0, counters=(11, 22), counters_alt=None, out_stride=0):
    """bote_test_merge on src (and alt): record slots [list][objective][KP][key, rank]."""
    L = _lib.lib()
    L.bote_test_merge.argtypes = _ARGTYPES
    n_lists, n_obj = src.shape[:2]
    alt_lists = 0 if alt is None else len(alt)
    groups = (max(n_lists, alt_lists) + 7) // 8 if mode == LEVEL else 1
    a = [None if x is None else np.ascontiguousarray(x, dtype=U)
         for x in (src, alt, kbound, None if sel is None else [sel], counters, counters_alt)]
    out, outc = np.zeros((groups, n_obj, KP, 2), U), np.zeros(2, U)
    p = _lib.ptr
    rc = L.bote_test_merge(0, mode, p(a[0]), n_lists, p(a[1]), alt_lists, n_obj, K, p(a[2]), p(a[3]), cap, p(a[4]),
                           p(a[5]), out_stride, p(out), p(outc))
    _lib.check(rc)
    return out, [int(x) for x in outc]


def assert_lists(got, want, names):
    for o, name in enumerate(names):
        bad = np.nonzero((got[o] != want[o]).any(axis=1))[0]
        assert bad.size == 0, (f"objective {o} ({name}): {bad.size} slots differ, first {bad[0]}: "
                               f"got {tuple(map(hex, got[o][bad[0]].tolist()))} want "
                               f"{tuple(map(hex, want[o][bad[0]].tolist()))}")


def assert_distinguishing(recs, want, K):
    """A dropped or swapped record cannot go unseen: the expected list holds
    more than one distinct record, and the K-th and (K+1)-th least differ."""
    n = min(len(recs), K)
    if n >= 2:
        assert len(np.unique(want[:n], axis=0)) > 1
    if len(recs) > K:
        both = sorted_fill(np.zeros(len(recs), np.int64), 1, recs, K + 1)[0][0]
        assert tuple(both[K - 1]) != tuple(both[K])


# ------------------------------------------------------------ wide merge --
class WideCase:
    """n_obj objectives of `n_lists` lists: each list the K least of its own
    records (a block's list), dumped by the model's dump() in a shuffled block
    order (or kept whole with kbound all ones: bounded=False), packed into
    record slots over stale records, with the sort's expectation."""

    def __init__(self, n_lists, K, lengths, patterns, seed, bounded=True):
        rng = np.random.default_rng(seed)
        self.K, self.patterns, self.n_lists = K, patterns, n_lists
        self.src = stale_block(n_lists, len(patterns))
        self.kbound = np.full(len(patterns), ONES, U)
        self.want = np.zeros((len(patterns), KP, 2), U)
        self.dumped, self.recs = [], []
        lengths = np.asarray(lengths)
        ids = np.repeat(np.arange(n_lists), lengths)
        order = list(range(n_lists))
        random.Random(seed).shuffle(order)
        for o, pat in enumerate(patterns):
            recs = records(pat, len(ids), K, rng)
            arr, cnt = sorted_fill(ids, n_lists, recs, K)  # each block keeps its K least
            cnt = np.minimum(cnt, K)
            recs = arr[np.arange(K)[None, :] < cnt[:, None]]  # the undumped lists' real records
            lists = [tuples(arr[i, :cnt[i]]) for i in range(n_lists)]
            if bounded:
                dumped, bound = dump(lists, K, order)
            else:
                dumped, bound = [L + [REC_MAX] for L in lists], ONES
            m = np.array([len(L) - 1 for L in dumped])
            keep = np.arange(K)[None, :] < m[:, None]
            self.src[:, o, :K][keep] = arr[keep]
            # a list of K records has no terminator: slot K is never read
            t = np.nonzero(m < K)[0]
            self.src[t, o, m[t]] = U(ONES)
            self.kbound[o] = bound
            self.want[o] = k_least(recs, K)
            assert_distinguishing(recs, self.want[o], K)
            self.dumped.append(dumped)
            self.recs.append(recs)

    def gathered(self, o, b0=None):
        """The model's bound record and gathered count of objective o."""
        b0 = int(self.kbound[o]) if b0 is None else b0
        bk, br = head_bound(self.dumped[o], self.K, b0)
        return (bk, br), sum(prefix_counts(self.dumped[o], self.K, b0, bk, br))

    def check(self, mode=WIDE, **kw):
        kw.setdefault("kbound", self.kbound)
        got, counters = merge(mode, self.src, self.K, **kw)
        assert_lists(got[0], self.want, self.patterns)
        return counters


def mixed_lengths(n_lists, K, seed):
    """Empty, one-record, shorter-than-the-heads and full lists side by side;
    few full ones among many lists (the union stays small)."""
    rng = np.random.default_rng(seed)
    if n_lists in (49, 50, 51):  # K = 100: 50 x WIDE_HEAD heads are the first to bound
        return np.full(n_lists, K)
    if n_lists <= 64:
        return rng.choice([0, 1, 2, 3, K, 3 * K], n_lists)
    full = rng.random(n_lists) < 32 / n_lists
    return np.where(full, K, rng.choice([0, 1, 2, 3, 7], n_lists))


COUNTS = [1, 3, 4, 5, 49, 50, 51, 255, 256, 257, 4095, 4096]  # 4 lists per thread, the wave, the launch limit
EDGES = ([(n, 100) for n in COUNTS] + [(n, k) for n in (1, 4, 5, 50, 256, 257, 4096) for k in (1, 128)] +
         [(n, k) for n in (3, 49, 51, 255, 4095) for k in (2, 127)])


@pytest.mark.parametrize("n_lists,K", EDGES)
def test_wide_list_count_edges_and_key_patterns(n_lists, K):
    """Every list count edge and K, eight key patterns per launch."""
    case = WideCase(n_lists, K, mixed_lengths(n_lists, K, n_lists), PATTERNS, 1000 * n_lists + K)
    keys = {p: r[:, 0] for p, r in zip(PATTERNS, case.recs)}
    if len(keys["cov"]) >= 100:
        assert int(keys["cov"].max()) - int(keys["cov"].min()) > 2**62
        assert {int(k) for k in keys["extremes"]} == {0, 2**63, ONES - 1}
        assert len(np.unique(keys["ties5"])) == 5 and len(np.unique(keys["equal"])) == 1
        assert int(case.recs[3][:, 1].max()) - int(case.recs[3][:, 1].min()) > 2**40
    if K == 100 and n_lists in (49, 50, 51):  # the heads' bound first applies at 50 lists
        bound = case.gathered(0)[0]
        assert (bound == (ONES, ONES)) == (n_lists == 49), bound
    assert case.check() == [11, 22]


def head_select(case, o):
    """How the model's bound record of objective o is found: "none" (fewer than
    K heads), "single" (one head at the K-th key), "aux" (the small-bin finish
    ranked by (key, rank)) or "rank" (a rank select among the tied heads, with
    their ranks and the K-th's place among them)."""
    K, b0 = case.K, int(case.kbound[o])
    heads = []
    for L in case.dumped[o]:
        for r in L[:min(WIDE_HEAD, K)]:
            if r == REC_MAX or r[0] == ONES or r[0] > b0:
                break
            heads.append(r)
    ks = wide_select([k for k, _ in heads], K, WIDE_SLACK, stop_early=False, aux=[rk for _, rk in heads])
    if ks is None:
        return "none", [], 0
    bk, left, inbin, _, kaux = ks
    if inbin <= 1:
        return "single", [], 0
    tied = [rk for k, rk in heads if k == bk]
    return ("aux" if kaux is not None else "rank"), tied, left


def first_pass_excess(vals, need):
    """Values beyond the need-th in the bin a radix select's first pass picks
    (above WIDE_SLACK: the select needs a second pass)."""
    mn, mx = min(vals), max(vals)
    s_lo = max((mx - mn).bit_length() - 10, 0)
    bins = sorted((v - mn) >> s_lo for v in vals)
    d = bins[need - 1]
    return sum(1 for b in bins if b <= d) - need


@pytest.mark.parametrize("n_lists", [64, 256, 1024])
def test_wide_tied_heads_every_record_a_head(n_lists):
    """Lists of two records: every record is a head, so the K-th least head
    record is the union's K-th record and the bound record (bk, br) must keep
    it.  Tied keys reach the small-bin finish (has_aux) with few heads in the
    tie class and the rank select with many; the tied ranks span more than
    2^40 with nearly all in the first digit's bin, so that select needs
    several radix passes."""
    K = 100
    pats = ["ties_wide", "ties5", "equal", "extremes", "means"]
    case = WideCase(n_lists, K, np.full(n_lists, 2), pats, 77 + n_lists)
    how = {p: head_select(case, o) for o, p in enumerate(pats)}
    print({p: (h[0], len(h[1])) for p, h in how.items()})
    for o, p in enumerate(pats):
        if p != "means":
            assert how[p][0] in ("aux", "rank"), (p, how[p][0])  # heads tie at the K-th key
        assert K <= case.gathered(o)[1] <= WIDE_RANK_MAX  # one pass
    if n_lists == 64:  # 128 heads over 5 keys: a tie class of <= WIDE_FEW
        assert how["ties_wide"][0] == "aux" and 1 < len(how["ties_wide"][1]) <= WIDE_FEW
    else:
        # (the K-th head lies deep inside its tie class only where the class is large)
        for p in ("ties5", "ties_wide", "equal") if n_lists == 1024 else ("equal",):
            kind, tied, left = how[p]
            assert kind == "rank" and len(tied) > WIDE_FEW
            assert max(tied) - min(tied) > 2**40
            assert first_pass_excess(tied, left) > WIDE_SLACK
    case.check()


def test_wide_nan_keys_fill_the_tail_in_rank_order():
    """Fewer than K records with a real key in the union: NaN-COV records (key
    all ones, real rank) take the remaining places, in rank order, and decide
    the K-th place."""
    K, n_lists = 100, 40
    rng = np.random.default_rng(5)
    ids = np.repeat(np.arange(n_lists), 30)
    keys = np.where(rng.random(len(ids)) < 0.95, U(ONES), rng.integers(0, 2**21, len(ids), dtype=U))
    src, kbound, want, names = stale_block(n_lists, 2), np.full(2, ONES, U), np.zeros((2, KP, 2), U), ["nan", "all_nan"]
    for o in range(2):
        recs = np.stack([keys if o == 0 else np.full(len(ids), ONES, U), ranks_of("means", len(ids), rng)], axis=1)
        real = int((recs[:, 0] != U(ONES)).sum())
        assert real < K < len(recs) and (o == 1 or real > 1)
        arr, cnt = sorted_fill(ids, n_lists, recs, K)
        src[:, o, :30] = arr[:, :30]
        src[:, o, 30] = U(ONES)
        want[o] = k_least(recs, K)
        assert_distinguishing(recs, want[o], K)
        assert int(want[o][K - 1][0]) == ONES and int(want[o][K - 1][1]) != ONES  # a NaN record at the K-th place
    got, _ = merge(WIDE, src, K, kbound=kbound)
    assert_lists(got[0], want, names)


@pytest.mark.parametrize("K", [1, 100, 128])
def test_wide_fill(K):
    """Every list empty; a union smaller than K; lists of 0 and 1 records
    followed by stale records below every real key, enough of them that the
    heads would bound the merge if they counted; full lists with nothing
    after them (K = KP)."""
    n = 120
    empty = WideCase(n, K, np.zeros(n, int), PATTERNS, 1)
    assert (empty.want == U(ONES)).all()
    empty.check()
    few = WideCase(n, K, (np.arange(n) % 40 == 0).astype(int) * 2, PATTERNS, 2)
    if K > 6:
        assert 1 < len(few.recs[0]) < K
    few.check()
    short = WideCase(n, K, np.arange(n) % 2, PATTERNS, 3)  # 0 and 1 records: each followed by a terminator and stale slots
    assert (short.src[:, :, 2:, 0] == 0).all()  # stale keys of 0 from slot 2 on
    assert (short.src[0::2, :, 0] == U(ONES)).all() and (K == 1 or (short.src[1::2, :, 1] == U(ONES)).all())
    short.check()
    full = WideCase(50, K, np.full(50, K), PATTERNS, 4, bounded=False)
    if K == KP:
        assert not (full.src[:, :, :, 1] < RANK0).any()  # every slot a real record
    full.check()


@pytest.mark.parametrize("extra", [0, 1])
def test_wide_gathered_count_at_the_one_pass_limit(extra):
    """K = 128, 32 lists, no bound from kbound or the heads (64 heads < K):
    exactly WIDE_RANK_MAX = 32 x 32 records gathered take the one-pass rank
    path, one more the windowed path."""
    K, lengths = 128, np.full(32, 32)
    lengths[17] += extra
    case = WideCase(32, K, lengths, PATTERNS, 9 + extra, bounded=False)
    for o in range(len(PATTERNS)):
        bound, total = case.gathered(o)
        assert bound == (ONES, ONES) and total == WIDE_RANK_MAX + extra
    case.check()


def windows(cnt, room):
    """The windowed path's passes over the lists' gathered counts."""
    off = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    total, w0, n = int(np.sum(cnt)), 0, 0
    while w0 < total:
        nxt = total
        for c, o in zip(cnt, off):
            if c and o >= w0 and o + c - w0 > room:
                nxt = min(nxt, int(o))
        w0, n = nxt, n + 1
    return n


@pytest.mark.parametrize("n_lists,K,n_windows", [(49, 100, 2), (63, 128, 3)])
def test_wide_windowed_path(n_lists, K, n_windows):
    """Full lists and no bound at all: 4,900 records in two windows, 8,064 in three."""
    case = WideCase(n_lists, K, np.full(n_lists, K), PATTERNS, n_lists, bounded=False)
    for o in range(len(PATTERNS)):
        bound, total = case.gathered(o)
        assert bound == (ONES, ONES) and total == n_lists * K
        assert total > WIDE_RANK_MAX and total > WIDE_SORT - K
        assert windows(prefix_counts(case.dumped[o], K, ONES), WIDE_SORT - K) == n_windows
    case.check()


def test_wide_heavy_ties_over_4096_lists_are_bounded_by_rank():
    """The model's test_heavy_ties_at_the_kth_key_are_bounded_by_rank at 4,096
    lists of 8 records: the key bound alone would gather far more than
    WIDE_RANK_MAX records, the tied heads' rank bound keeps them near K."""
    blocks, per_block, K = 4096, 8, 100
    rng = np.random.default_rng(7 + blocks)
    ids = np.repeat(np.arange(blocks), per_block)
    src, want = stale_block(blocks, 2), np.zeros((2, KP, 2), U)
    for o in range(2):
        ranks = rng.permutation(blocks * per_block).astype(U) + U(RANK0)  # the blocks' ranks interleave
        keys = rng.choice(np.array([1000, 1000, 1000, 1001, 1003, 1010], U), len(ids))
        recs = np.stack([keys, ranks], axis=1)
        arr, _ = sorted_fill(ids, blocks, recs, K)
        dumped, kb = dump([tuples(a) for a in arr[:, :per_block]], K, list(range(blocks)))
        assert kb == ONES and all(len(L) == per_block + 1 for L in dumped)
        src[:, o, :per_block] = arr[:, :per_block]
        src[:, o, per_block] = U(ONES)
        bk, br = head_bound(dumped, K, kb)
        keys_only = sum(prefix_counts(dumped, K, kb, bk, ONES))
        tight = sum(prefix_counts(dumped, K, kb, bk, br))
        assert keys_only > WIDE_RANK_MAX and K <= tight <= 2 * K + 64, (tight, keys_only)
        want[o] = k_least(recs, K)
        assert_distinguishing(recs, want[o], K)
    got, _ = merge(WIDE, src, K, kbound=np.full(2, ONES, U))
    assert_lists(got[0], want, ["ties", "ties"])


@pytest.mark.parametrize("mode", [WIDE, CHAIN])
@pytest.mark.parametrize("sel", [None, "cap", "cap+1"])
def test_wide_device_side_choice(mode, sel):
    """sel null or *sel == cap: src, its counters, and kbound is honoured (a
    bound below the union's K-th key, outside the contract, cuts the result at
    that key); *sel == cap + 1: alt, with another list count and other
    counters, and a kbound of 0 is ignored.  In chain mode kbound && sel is
    what picks the one-launch merge: its result is padded from slot K on,
    where the tree (sel null) keeps the KP least."""
    K, cap = 100, 1 << 20
    src = WideCase(70, K, mixed_lengths(70, K, 70), PATTERNS, 70)
    alt = WideCase(37, K, mixed_lengths(37, K, 37), PATTERNS, 37, bounded=False)
    kw = dict(alt=alt.src, counters=(11, 22), counters_alt=(33, 44), cap=cap)
    if sel == "cap+1":
        got, counters = merge(mode, src.src, K, kbound=np.zeros(len(PATTERNS), U), sel=cap + 1, **kw)
        assert_lists(got[0], alt.want, PATTERNS)
        assert counters == [33, 44]
        return
    if sel is None and mode == CHAIN:  # the tree on whole lists: pack them again, padded, with nothing stale
        whole = np.full_like(src.src, U(ONES))
        want = np.zeros_like(src.want)
        for o, recs in enumerate(src.recs):
            ids = np.repeat(np.arange(src.n_lists), [len(L) - 1 for L in src.dumped[o]])
            kept = np.concatenate([np.array(L[:-1], U).reshape(-1, 2) for L in src.dumped[o]])
            whole[:, o] = sorted_fill(ids, src.n_lists, kept, KP)[0]
            want[o] = k_least(kept, KP)
        assert any(int(w[K][0]) != ONES for w in want)  # more than K records: the tree keeps them
        got, counters = merge(CHAIN, whole, K, kbound=src.kbound, counters=(11, 22))
        assert_lists(got[0], want, PATTERNS)
        assert counters == [11, 22]
        return
    # a bound at the (K/2)-th key of the union: honoured, the result ends at that key
    cut, want = np.zeros(len(PATTERNS), U), np.zeros_like(src.want)
    for o, recs in enumerate(src.recs):
        cut[o] = src.want[o][K // 2][0]
        want[o] = k_least(recs[recs[:, 0] <= cut[o]], K)
    assert any((w != s).any() for w, s in zip(want, src.want))
    for kbound, expect in ((src.kbound, src.want), (cut, want)):
        got, counters = merge(mode, src.src, K, kbound=kbound, sel=None if sel is None else cap, **kw)
        assert_lists(got[0], expect, PATTERNS)
        assert counters == [11, 22]


# ------------------------------------------------------------ merge tree --
class TreeCase:
    """`n_lists` whole lists per objective (KP slots, sorted, padded with
    REC_MAX): ties across lists (equal keys with different ranks), the same
    record in two lists, NaN keys; and the sort's expectation per group of 8
    lists (one level) and over all lists (the chain)."""

    def __init__(self, n_lists, seed, patterns=PATTERNS):
        rng = np.random.default_rng(seed)
        self.n_lists, self.patterns = n_lists, patterns
        self.src = np.zeros((n_lists, len(patterns), KP, 2), U)
        groups = (n_lists + 7) // 8
        self.level = np.zeros((groups, len(patterns), KP, 2), U)
        self.chain = np.zeros((len(patterns), KP, 2), U)
        if n_lists <= 65:
            lengths = rng.choice([0, 1, 5, 40, KP], n_lists)
        else:
            lengths = np.where(rng.random(n_lists) < 16 / n_lists, KP, rng.choice([0, 1, 2, 3], n_lists))
        lengths[0] = KP - 8  # (the union holds more than KP records; room for the copies below)
        if n_lists > 1:
            lengths[1] = KP - 12
            lengths[-1] = min(lengths[-1], KP - 12)
        ids = np.repeat(np.arange(n_lists), lengths)
        for o, pat in enumerate(patterns):
            recs = records(pat, len(ids), KP, rng)
            lid = ids
            if n_lists > 1:  # the same records in two lists: 8 of list 0's also in list 1, 4 of them in the last too
                dup = recs[lid == 0][:8]
                recs = np.concatenate([recs, dup, dup[:4]])
                lid = np.concatenate([lid, np.full(8, 1), np.full(4, n_lists - 1)])
            self.src[:, o], cnt = sorted_fill(lid, n_lists, recs, KP)
            assert cnt.max() <= KP
            self.level[:, o], _ = sorted_fill(lid // 8, groups, recs, KP)
            self.chain[o] = k_least(recs, KP)
            assert_distinguishing(recs, self.chain[o], KP)


TREE_COUNTS = [1, 7, 8, 9, 64, 65, 513, 4097]  # one group, one level, two, ... one past the wide limit
_tree_cases = {}


def tree_case(n_lists):
    if n_lists not in _tree_cases:
        _tree_cases[n_lists] = TreeCase(n_lists, 500 + n_lists)
    return _tree_cases[n_lists]


@pytest.mark.parametrize("n_lists", TREE_COUNTS)
def test_tree_one_level(n_lists):
    """One launch_merge level writing its output lists out_stride != list_stride
    apart (as the batch does): every group of 8 lists into its KP least."""
    case = tree_case(n_lists)
    lstride = len(PATTERNS) * KP
    got, _ = merge(LEVEL, case.src, KP, out_stride=lstride + 1 + n_lists % 5)
    for g in range(len(case.level)):
        assert_lists(got[g], case.level[g], [f"group {g} {p}" for p in PATTERNS])


@pytest.mark.parametrize("K", [100, KP])
@pytest.mark.parametrize("n_lists", TREE_COUNTS)
def test_tree_chain(n_lists, K):
    """The chain without kbound: the tree down to one list (the KP least,
    whatever K) and the plain counter copy."""
    case = tree_case(n_lists)
    got, counters = merge(CHAIN, case.src, K, counters=(5, 2**64 - 3))
    assert_lists(got[0], case.chain, PATTERNS)
    assert counters == [5, 2**64 - 3]


def test_tree_past_the_wide_limit_with_kbound_and_sel():
    """4,097 lists with kbound and sel: one list too many for the one-launch
    merge, so the chain runs the tree (records beyond slot K survive) and
    pick_counters."""
    case, small = tree_case(4097), tree_case(9)
    assert case.n_lists == WIDE_MERGE_LISTS + 1 and int(case.chain[0][KP - 1][0]) != ONES
    kw = dict(kbound=np.full(len(PATTERNS), ONES, U), alt=small.src, counters=(1, 2), counters_alt=(3, 4), cap=7)
    got, counters = merge(CHAIN, case.src, 100, sel=7, **kw)
    assert_lists(got[0], case.chain, PATTERNS)
    assert counters == [1, 2]
    got, counters = merge(CHAIN, case.src, 100, sel=8, **kw)
    assert_lists(got[0], small.chain, PATTERNS)
    assert counters == [3, 4]


@pytest.mark.parametrize("n_lists", [8, 65])
def test_tree_unsorted_list_takes_the_bitonic_fallback(n_lists):
    """One list with two records out of order: its group sorts (block_bitonic)
    instead of ranking, the other groups rank; the result is the same."""
    case = tree_case(n_lists)
    src = case.src.copy()
    for o in range(len(PATTERNS)):
        L = src[1, o]
        assert tuple(L[3]) != tuple(L[60]) and int(L[60][1]) != ONES
        L[[3, 60]] = L[[60, 3]]
    got, _ = merge(LEVEL, src, KP, out_stride=len(PATTERNS) * KP + 3)
    for g in range(len(case.level)):
        assert_lists(got[g], case.level[g], [f"group {g} {p}" for p in PATTERNS])
    got, _ = merge(CHAIN, src, KP)
    assert_lists(got[0], case.chain, PATTERNS)


@pytest.mark.parametrize("n_lists,alt_lists", [(65, 9), (9, 65), (7, 8)])
@pytest.mark.parametrize("over", [False, True])
def test_tree_device_side_choice_pads_the_surplus_groups(n_lists, alt_lists, over):
    """alt_lists above and below n_lists, *sel on either side of cap: the
    groups cover the larger input and the surplus ones emit padding lists; the
    chain merges them away and pick_counters copies the chosen counters."""
    src, alt = tree_case(n_lists), tree_case(alt_lists)
    cap = 2**40
    chosen = alt if over else src
    kw = dict(alt=alt.src, sel=cap + 1 if over else cap, cap=cap, counters=(11, 22), counters_alt=(33, 44))
    got, _ = merge(LEVEL, src.src, KP, out_stride=2 * len(PATTERNS) * KP, **kw)
    assert len(got) == (max(n_lists, alt_lists) + 7) // 8
    for g in range(len(got)):
        want = chosen.level[g] if g < len(chosen.level) else np.full_like(got[g], U(ONES))
        assert_lists(got[g], want, [f"group {g} {p}" for p in PATTERNS])
    got, counters = merge(CHAIN, src.src, 100, **kw)  # (no kbound: the tree)
    assert_lists(got[0], chosen.chain, PATTERNS)
    assert counters == ([33, 44] if over else [11, 22])


def test_model_lists_through_both_merges():
    """The model's own block_lists (Python tuples, small keys with heavy ties)
    through dump() and the one-launch merge, and whole through the tree."""
    K, n = 10, 130
    lists = [[(k + 10, r) for k, r in L] for L in block_lists(random.Random(3), n, 30, K, 7)]  # above the stale keys
    recs = np.array([r for L in lists for r in L], U)
    dumped, bound = dump(lists, K, random.Random(4).sample(range(n), n))
    src, whole = stale_block(n, 1), np.full((n, 1, KP, 2), U(ONES))
    for i, L in enumerate(dumped):
        src[i, 0, :len(L)] = np.array(L, U)
        whole[i, 0, :K] = np.array(lists[i], U)
    assert_distinguishing(recs, k_least(recs, K), K)
    got, _ = merge(WIDE, src, K, kbound=np.array([bound], U))
    assert_lists(got[0], k_least(recs, K)[None], ["model"])
    got, _ = merge(CHAIN, whole, K)
    assert_lists(got[0], k_least(recs, KP)[None], ["model"])


def test_bad_arguments_are_refused_before_any_launch():
    src = np.full((1, 1, KP, 2), U(ONES))
    L = _lib.lib()
    L.bote_test_merge.argtypes = _ARGTYPES
    p = _lib.ptr
    c, out, outc = np.zeros(2, U), np.zeros((1, 1, KP, 2), U), np.zeros(2, U)

    def rc(mode=CHAIN, s=src, n_lists=1, alt=None, alt_lists=0, n_obj=1, K=1, sel=None, counters=c, ca=None, stride=0):
        return L.bote_test_merge(0, mode, p(s), n_lists, p(alt), alt_lists, n_obj, K, None, p(sel), 0, p(counters),
                                 p(ca), stride, p(out), p(outc))

    assert rc() == 0
    out[:] = 0
    assert rc(s=None) == -1 and rc(counters=None) == -1 and rc(n_lists=0) == -1  # BOTE_E_ARG
    assert rc(alt=src) == -1 and rc(alt_lists=1) == -1  # alt without its count, and the reverse
    assert rc(sel=c) == -1 and rc(sel=c, alt=src, alt_lists=1) == -1  # sel without alt, without counters_alt
    assert rc(mode=3) == -1
    assert rc(n_obj=9) == -4 and rc(n_obj=0) == -4  # BOTE_E_RANGE
    assert rc(K=KP + 1) == -4 and rc(K=0) == -4
    assert rc(mode=WIDE, n_lists=WIDE_MERGE_LISTS + 1) == -4
    assert rc(mode=WIDE, alt=src, alt_lists=WIDE_MERGE_LISTS + 1) == -4
    assert rc(mode=LEVEL, stride=KP - 1) == -4
    assert (out == 0).all()  # only the first call wrote
