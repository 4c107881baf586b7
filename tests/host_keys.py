"""TEST INFRASTRUCTURE: the host side of the sweep tests that build their
expected top-K lists from the CPU oracle's per-client values
(OraclePlanet.compute_stats): the configs in colex order, one slot's columns,
a slot's key by each objective kind's definition, and the K least (key, rank)."""
import itertools
import math

import numpy as np

from fantoch_amd import _lib

MEAN, MAX, MDTM = _lib.OBJ_MEAN, _lib.OBJ_MAX, _lib.OBJ_MDTM


def colex_positions(ns, n):
    """Every n-subset of range(ns) as ascending positions, in colex rank order."""
    c = np.array(list(itertools.combinations(range(ns), n)), dtype=np.uint32)
    return c[np.lexsort(tuple(c[:, j] for j in range(n)))]  # (the last key, p[n-1], is the primary one)


def colex_rank(c):
    return sum(math.comb(int(x), j + 1) for j, x in enumerate(c))


def supersets(ns, n, pinned):
    """The n-supersets of `pinned` among ns positions sorted by full colex rank, and those ranks."""
    free = [x for x in range(ns) if x not in pinned]
    cfgs = [tuple(sorted(set(pinned) | set(c))) for c in itertools.combinations(free, n - len(pinned))]
    cfgs.sort(key=colex_rank)
    return np.array(cfgs, dtype=np.uint32), np.array([colex_rank(c) for c in cfgs], dtype=np.uint64)


def slot_values(vals, slot, nc, n):
    """compute_stats' columns of one slot: Input clients for slots 0..4, the n members for 5..9."""
    if slot < 5:
        return vals[:, slot * nc:(slot + 1) * nc]
    return vals[:, 5 * nc + (slot - 5) * n:5 * nc + (slot - 4) * n]


def top_of(keys, k, ranks=None):
    """The k least (key, rank) of per-config keys, ascending (ranks: ascending; default the index)."""
    keys = np.asarray(keys, dtype=np.uint64)
    ranks = np.arange(len(keys)) if ranks is None else np.asarray(ranks)
    order = np.lexsort((ranks, keys))[:k]
    return [(int(keys[i]), int(ranks[i])) for i in order]


def key_of(kind, v):
    """Per-config key of one slot's values (ncfg, count); H of MDTM by its
    definition, the sum of the positive (count * x - sum)."""
    v = np.asarray(v).astype(np.int64)
    c, s = v.shape[1], v.sum(axis=1)
    s64 = s.astype(np.uint64)
    if kind == MEAN:
        return s64
    if kind == MDTM:
        h = np.maximum(c * v - s[:, None], 0).sum(axis=1)
        assert int(s.max()) < (1 << 27) - 1 and int(h.max()) < 1 << 37
        return (h.astype(np.uint64) << np.uint64(27)) | s64
    u = v.astype(np.uint64)
    if kind == MAX:
        return (u.max(axis=1) << np.uint64(32)) | s64
    assert _lib.is_pctl(kind)
    idx, whole = _lib.percentile_index(kind & 0xFFFF, c)
    a = np.sort(u, axis=1)
    twice = 2 * a[:, 0] if idx == 0 else a[:, idx - 1] + a[:, idx] if whole else 2 * a[:, idx - 1]
    return (twice << np.uint64(32)) | s64
