"""GPU test of the top-K seed kernel alone (bote_merge.hip seed_kernel), through
the library's test entry bote_test_seed (not part of the ABI): per row, the
K-th least of nsamp u64 keys, all-ones when the row has fewer than K keys.

A seed that is too high changes no sweep result (only the lists' fill cost)
and one that is too low shows only as records missing from a golden top-K, so
the kernel is checked here directly against a sort: one launch of 8 rows of
different key patterns (test_merge_model.seed_rows) per (nsamp, K)."""
import ctypes as C

import numpy as np
import pytest

from fantoch_amd import _lib
from tests.test_merge_model import ONES, seed_rows

pytestmark = pytest.mark.gpu

# 32768 = 32 keys x 1,024 threads: the last size held in registers; 32769 re-reads memory
NSAMP = [1, 99, 100, 101, 1024, 1025, 4096, 32768, 32769]
KS = [1, 100, 128]


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("nsamp", NSAMP)
def test_seed_is_the_kth_least_key(nsamp, K):
    L = _lib.lib()
    L.bote_test_seed.argtypes = [C.c_int, _lib._u64p, C.c_uint32, C.c_uint32, C.c_uint32, _lib._u64p]
    keys = np.ascontiguousarray(seed_rows(nsamp, K, np.random.default_rng(1000 * nsamp + K)))
    got = np.zeros(len(keys), np.uint64)
    _lib.check(L.bote_test_seed(0, keys.reshape(-1), nsamp, len(keys), K, got))
    want = [int(np.sort(r)[K - 1]) if nsamp >= K else ONES for r in keys]
    print(f"nsamp={nsamp} K={K} got={[hex(int(x)) for x in got]}")
    assert [int(x) for x in got] == want
