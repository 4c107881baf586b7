"""Streaming evolving search: Search::sorted_evolving_configs (search.rs:97-178)
without the stored configs.

The reference ranks every config of every n, then joins the levels n = 3 -> 5
-> ... -> 13: each level a valid superset of the one before whose Atlas means
lie min_mean_decrease below it (super_configs, search.rs:378-419).  That needs
every config of every n in memory.  Here level 0 is one unpinned sweep for the
K best valid configs, and every further level is a bounded batch of pinned
sweeps (PinnedBatch with prev_sums, DESIGN.md §4 "Streaming evolving search"):
the K best valid supersets of each config at the ends of the kept chains, the
reference's filter applied by the kernels.  Between levels a beam keeps the
best partial chains.

When nothing was cut (`exhaustive`: no list came back full and the beam kept
everything) the result is sorted_evolving_configs itself: the same chains with
the same scores, equal scores ordered by colex ranks here and by enumeration
order in the reference."""
from __future__ import annotations

import time
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .bote import DevicePlanet, PinnedBatch, RankingParams, Sweep, eval_configs, max_f

BATCH_MAX_SETS = 1024  # include/bote_hip.h BOTE_BATCH_MAX_SETS
_SIGN = np.uint64(0x8000000000000000)


def score_key(score) -> np.ndarray:
    """A SCORE record's key: ~orderable(score), the device's (bote_device.hpp
    orderable_f64): ascending keys are descending scores, NaN one quiet value,
    -0.0 and 0.0 distinct."""
    x = np.array(score, dtype=np.float64, ndmin=1)
    b = x.view(np.uint64).copy()
    b[np.isnan(x)] = np.uint64(0x7FF8000000000000)
    ob = np.where(b >> np.uint64(63) != 0, ~b, b | _SIGN)
    return ~ob


def key_score(key) -> np.ndarray:
    """The f64 score of a SCORE record's key, bit for bit: the inverse of score_key."""
    ob = ~np.array(key, dtype=np.uint64, ndmin=1)
    bits = np.where(ob >> np.uint64(63) != 0, ob & ~_SIGN, ~ob)
    return np.ascontiguousarray(bits, dtype=np.uint64).view(np.float64)


def beam_select(scores, ranks, beam: Optional[int]) -> Tuple[np.ndarray, bool]:
    """The order and the cut of one selection step.  scores: (P,) f64 partial
    scores; ranks: (P, L) colex ranks per level.  Returns the indices of the kept
    chains, best first: score descending (the records' order, score_key), then the
    tuple of ranks ascending; the `beam` best (None: all), and whether any was cut."""
    if beam is not None and beam < 0:
        raise ValueError("beam must be None or >= 0")
    scores = np.asarray(scores, dtype=np.float64).reshape(-1)
    if not len(scores):
        return np.zeros(0, np.int64), False
    ranks = np.asarray(ranks, dtype=np.uint64).reshape(len(scores), -1)
    cols = [ranks[:, j] for j in range(ranks.shape[1] - 1, -1, -1)]  # (lexsort: the last key is the primary)
    # (-0.0 ranks as 0.0, the F64 order)
    order = np.lexsort(cols + [score_key(scores + 0.0)])
    cut = beam is not None and len(order) > beam
    return (order[:beam] if cut else order), cut


@dataclass
class LevelStats:
    n: int
    frontier: int     # distinct configs extended (level 0: 0)
    batches: int      # PinnedBatch launches (level 0: the one sweep counts 0)
    chains: int       # partial chains after the level's selection
    kernel_ms: float  # sum of the level's kernel times


@dataclass
class EvolveResult:
    chains: List[Tuple[float, List[int]]]  # (score, [colex rank per level]), best first
    exhaustive: bool
    levels: List[LevelStats]
    ns: List[int]            # the levels' config sizes
    servers: np.ndarray
    wall_s: float = 0.0
    scores: np.ndarray = field(default_factory=lambda: np.zeros(0))  # the chains' scores as f64

    def configs_of(self, chain) -> List[List[int]]:
        """Region ids per level of one entry of `chains` (or of its rank list)."""
        ranks = chain[1] if isinstance(chain, tuple) else chain
        return [[int(self.servers[p]) for p in _lib.colex_unrank(int(r), n, len(self.servers))]
                for r, n in zip(ranks, self.ns)]


class Evolve:
    """The streaming evolving search over `servers` (region ids, ascending for the
    fast kernels) and `clients`: levels ranking.min_n, min_n + 2, .., max_n, all five
    ranking parameters.  K: records kept per list (the level-0 sweep's and every
    set's); beam: partial chains kept after each level (None: all)."""

    def __init__(self, dp: DevicePlanet, servers: Sequence[int], clients: Sequence[int], ranking: RankingParams,
                 beam: Optional[int] = None, K: int = 100, kernel: Optional[str] = None):
        if ranking.min_n < 2 or ranking.max_n > 16 or ranking.max_n < ranking.min_n or \
                (ranking.max_n - ranking.min_n) % 2:
            raise ValueError("evolving levels need 2 <= min_n <= max_n <= 16 and max_n - min_n even")
        if beam is not None and beam < 1:
            raise ValueError("beam must be None or >= 1")
        self.dp, self.ranking, self.beam, self.K, self.kernel = dp, ranking, beam, K, kernel
        self.servers, self.clients = _lib.u32(servers), _lib.u32(clients)
        self.ns = list(range(ranking.min_n, ranking.max_n + 1, 2))
        if self.ns[-1] > len(self.servers):
            raise ValueError("max_n is larger than the server list")

    def _extensions(self, n: int, prev_n: int, frontier: np.ndarray):
        """The bounded batches over the frontier (colex ranks of prev_n-configs): per
        frontier config its SCORE list at n as (keys, ranks), and the level's counters."""
        ns = len(self.servers)
        pos = np.stack([_lib.colex_unrank(int(r), prev_n, ns) for r in frontier])
        s1 = eval_configs(self.dp, self.servers, self.clients, prev_n, configs=pos, values=False).s1
        prev = np.ascontiguousarray(s1[:, [_lib.SLOT_AF1, _lib.SLOT_AF2]])
        if max_f(prev_n) < 2:
            prev[:, 1] = 0  # (no such slot; the f = 2 limit reads "no bound")
        lists, full, ms, batches = [], False, 0.0, 0
        for b0 in range(0, len(frontier), BATCH_MAX_SETS):
            b = PinnedBatch(self.dp, self.servers, self.clients, n, pos[b0:b0 + BATCH_MAX_SETS],
                            [(_lib.OBJ_SCORE, 0)], K=self.K, ranking=self.ranking, kernel=self.kernel,
                            prev_sums=prev[b0:b0 + BATCH_MAX_SETS])
            b.launch()
            for r in b.result():
                top = np.array(r.tops[0], dtype=np.uint64).reshape(-1, 2)
                full = full or len(top) >= self.K
                lists.append((top[:, 0], top[:, 1]))
            ms += b.kernel_ms()
            batches += 1
        return lists, full, ms, batches

    def run(self) -> EvolveResult:
        t0 = time.perf_counter()
        sw = Sweep(self.dp, self.servers, self.clients, self.ns[0], [(_lib.OBJ_SCORE, 0)], K=self.K,
                   ranking=self.ranking, digest=False, kernel=self.kernel)
        sw.launch()
        res = sw.result()
        top = np.array(res.tops[0], dtype=np.uint64).reshape(-1, 2)
        exhaustive = res.valid <= self.K
        scores, ranks = key_score(top[:, 0]), top[:, 1].reshape(-1, 1)
        keep, cut = beam_select(scores, ranks, self.beam)
        exhaustive = exhaustive and not cut
        scores, ranks = scores[keep], ranks[keep]
        levels = [LevelStats(self.ns[0], 0, 0, len(scores), sw.kernel_ms())]
        for prev_n, n in zip(self.ns, self.ns[1:]):
            if not len(scores):
                levels.append(LevelStats(n, 0, 0, 0, 0.0))
                continue
            frontier, which = np.unique(ranks[:, -1], return_inverse=True)
            lists, full, ms, batches = self._extensions(n, prev_n, frontier)
            exhaustive = exhaustive and not full
            # every chain times every record of its end's list
            cnt = np.array([len(k) for k, _ in lists], dtype=np.int64)
            start = np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.int64)
            ekey = np.concatenate([k for k, _ in lists]) if len(lists) else np.zeros(0, np.uint64)
            erank = np.concatenate([r for _, r in lists]) if len(lists) else np.zeros(0, np.uint64)
            per = cnt[which]
            rep = np.repeat(np.arange(len(scores)), per)
            first = np.concatenate([[0], np.cumsum(per)[:-1]]).astype(np.int64)
            e = start[which][rep] + (np.arange(len(rep)) - np.repeat(first, per))
            # (the reference's left-to-right sum: score3 + score5 + ...)
            scores = scores[rep] + key_score(ekey[e]) if len(rep) else np.zeros(0)
            ranks = np.concatenate([ranks[rep], erank[e].reshape(-1, 1)], axis=1)
            keep, cut = beam_select(scores, ranks, self.beam)
            exhaustive = exhaustive and not cut
            scores, ranks = scores[keep], ranks[keep]
            levels.append(LevelStats(n, len(frontier), batches, len(scores), ms))
        chains = [(float(s), [int(x) for x in r]) for s, r in zip(scores, ranks)]
        return EvolveResult(chains, bool(exhaustive), levels, list(self.ns), self.servers,
                            time.perf_counter() - t0, np.array(scores, dtype=np.float64))
