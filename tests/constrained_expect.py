"""TEST INFRASTRUCTURE: the CPU side of the constrained-sweep tests
(tests/test_gpu_constrained.py, tests/test_constrained_bounds.py).  A constrained
sweep's expected lists are the CPU oracle's complete order (OraclePlanet.sweep
with K = every config, as tests/test_gpu_census.py takes it) filtered to the
admitted ranks and cut to K; a constraint's key per config is the key of its own
complete list's record for that config."""
import math

import numpy as np

from fantoch_amd import _lib

U64 = (1 << 64) - 1
SCORE, MEAN, COV, MAX, MDTM = _lib.OBJ_SCORE, _lib.OBJ_MEAN, _lib.OBJ_COV, _lib.OBJ_MAX, _lib.OBJ_MDTM
AF1, FF1, AF2, FF2, E = 0, 1, 2, 3, 4
OBJS = [(SCORE, 0), (MEAN, AF1), (MEAN, FF1), (COV, AF1), (COV, 5 + FF1), (MEAN, E)]
RP = (110.0, 35.0, 0.0, 15.0)
NAN_KEY = 0x7FF8000000000000

# The cases of the issue's table: constraints as ((kind, slot), d), the bound being the key of record
# total // d of the constraint's own complete list; then per n the admitted count and the number of
# admitted valid configs (the complete SCORE list of the constrained sweep; None: not stated).
CASES = {
    "cov_ff1C": ([((COV, 5 + FF1), 3)], {3: (381, 2), 5: (5169, 227)}),
    "mean_e": ([((MEAN, E), 3)], {3: (381, 0), 5: (5174, 62)}),
    "mean_ff1": ([((MEAN, FF1), 3)], {3: (382, 0), 5: (5180, 0)}),
    "mean_ff1_and_cov_af1": ([((MEAN, FF1), 3), ((COV, AF1), 2)], {3: (190, None), 5: (2449, None)}),
}


def full_order(o, R, n, objs=OBJS):
    """The oracle's complete ordered lists over the n-subsets of R regions (every region a server
    and a client) as Python-int (key, rank) tuples, and the valid count."""
    srv = np.arange(R, dtype=np.uint32)
    total = math.comb(R, n)
    tops, valid, digest = o.sweep(srv, srv, n, 0, total, objs, total, RP, 2, 8)
    lists = [[(int(k), int(r)) for k, r in t] for t in tops]
    assert all(len(t) == (valid if kind == SCORE else total) for t, (kind, _) in zip(lists, objs))
    assert all(t == sorted(t) for t in lists)
    return lists, valid, digest


def bound_at(lst, index):
    """The key of record `index` of a complete list."""
    return lst[index][0]


def admitted_ranks(lists, objs, cons):
    """The ranks whose key is <= max_key for every constraint (kind, slot, max_key); each
    constraint's (kind, slot) must be among `objs`, whose complete list gives the keys."""
    adm = None
    for kind, slot, max_key in cons:
        lst = lists[objs.index((kind, slot))]
        ok = {r for k, r in lst if k <= max_key}
        adm = ok if adm is None else adm & ok
    return adm


def filtered(lists, adm, K, n_lists=None):
    """The constrained sweep's lists: each complete list's admitted records, cut to K."""
    out = []
    for lst in lists[:n_lists]:
        recs = [rec for rec in lst if rec[1] in adm]
        out.append(recs[:K])
    return out


def case_constraints(lists, objs, total, case):
    """The (kind, slot, max_key) triples of a CASES entry."""
    return [(k, s, bound_at(lists[objs.index((k, s))], total // d)) for (k, s), d in CASES[case][0]]
