"""The group kernel's step (client loop, moments, validity, digest, keys)
against the exact generic kernel on a synthetic planet of 16 regions: valid
count, digest and all five top-K lists, over every config of the rank space
(n = 7: 11,440 configs).

The cases are the step's paths: whole client quads and each partial last quad
(nc % 4 = 1, 2, 3), steps with more distinct (p1, p2) pairs than a wave has
client-line slots next to steps that fit them, and the other instantiations of
the register-lookup (PERM) kernels that share the step's code (n = 5, 6).  A
planet of 36 regions adds the member-binned client loop (32 clients and more)
with the same four quad remainders, on a rank window.
"""
import itertools

import numpy as np
import pytest

from fantoch_amd import _lib
from fantoch_amd.bote import DEFAULT_OBJECTIVES, DEFAULT_RANKING, DevicePlanet, Sweep
from fantoch_amd.planet import Planet

pytestmark = pytest.mark.gpu

# client-line slots a wave gets at most (bote_capi_sweep.hip group_geometry)
MAX_LINE_SLOTS = 16


@pytest.fixture(scope="module")
def planets():
    return {R: DevicePlanet(Planet.synthetic(R)) for R in (16, 36)}


def _sweep(dp, R, clients, n, kernel, rb=0, re=None):
    srv = np.arange(R, dtype=np.uint32)
    sw = Sweep(dp, srv, clients, n, DEFAULT_OBJECTIVES, K=100, ranking=DEFAULT_RANKING, digest=True, kernel=kernel)
    assert sw.kernel_path() == kernel
    sw.launch(rb, sw.total if re is None else re)
    r = sw.result()
    return r.valid, r.digest, r.tops


def _check(dp, R, clients, n, rb=0, re=None):
    want = _sweep(dp, R, clients, n, "generic", rb, re)
    got = _sweep(dp, R, clients, n, "group", rb, re)
    assert got[0] == want[0], "valid count"
    assert got[1] == want[1], "digest"
    assert len(got[2]) == len(DEFAULT_OBJECTIVES) == 5
    for o, (g, w) in enumerate(zip(got[2], want[2])):
        assert g == w, f"top-K list of objective {o}"
    return want


def test_all_regions_are_clients(planets):
    """(a) nc = 16: whole quads."""
    valid, _, tops = _check(planets[16], 16, np.arange(16, dtype=np.uint32), 7)
    assert valid > 0 and all(tops), "the case must exercise the valid path and every list"


@pytest.mark.parametrize("nc", [13, 14, 15])
def test_partial_last_quad(planets, nc):
    """(b) 13, 14, 15 clients: a last quad of 1, 2, 3 clients."""
    assert nc % 4 == nc - 12
    _check(planets[16], 16, np.arange(nc, dtype=np.uint32), 7)


def _pairs_per_step(p3):
    """Distinct (p1, p2) among each 64-config step of a group whose smallest
    fixed position is p3: its C(p3, 3) low parts in colex order, from the
    group's first rank (low = 0)."""
    low = sorted(itertools.combinations(range(p3), 3), key=lambda c: c[::-1])
    return [len({(c[1], c[2]) for c in low[i:i + 64]}) for i in range(0, len(low), 64)]


def test_steps_with_and_without_client_lines(planets):
    """(c) The window is one whole group from its first rank (low = 0): fixed
    positions (12, 13, 14, 15), C(12, 3) = 220 configs in steps of 64.  Its
    first step holds the pairs (1,2), (1,3), (2,3), (1,4), ...: 25 of them,
    more than any wave has line slots, so it runs the four-source loop; its
    later steps hold 16, 13 and 4, which fit the slots (R = 16 leaves the LDS
    for all 16; the second step fills them exactly).  The product library
    exposes no path statistic, so the mix is asserted from the rank order
    itself."""
    per_step = _pairs_per_step(12)
    assert per_step == [25, 16, 13, 4]
    assert per_step[0] > MAX_LINE_SLOTS and all(k <= MAX_LINE_SLOTS for k in per_step[1:])
    base = sum(_lib.binomial(p, i + 1) for i, p in enumerate((12, 13, 14, 15), start=3))
    assert list(_lib.colex_unrank(base, 7, 16)) == [0, 1, 2, 12, 13, 14, 15]
    total = _lib.binomial(16, 7)
    assert base + 220 == total
    _check(planets[16], 16, np.arange(16, dtype=np.uint32), 7, base, total)
    # and a window that begins inside the group, after its no-lines step
    _check(planets[16], 16, np.arange(16, dtype=np.uint32), 7, base + 64, total)


@pytest.mark.parametrize("n", [5, 6])
def test_other_register_lookup_kernels(planets, n):
    """(d) n = 5 and 6: the other PERM instantiations."""
    _check(planets[16], 16, np.arange(16, dtype=np.uint32), n)


@pytest.mark.parametrize("nc", [16, 13])
def test_three_table_qtab_kernel(planets, nc):
    """n = 10 is the first config size with three leaderless quorum tables
    (qe = 8 next to qa1 = 6 and qa2 = 7): the LDS qtab path with its second
    member plane.  All C(16, 10) = 8,008 configs, whole quads and a last quad
    of one client; 282 of them are valid at nc = 16 (CPU oracle)."""
    valid, _, tops = _check(planets[16], 16, np.arange(nc, dtype=np.uint32), 10)
    if nc == 16:
        assert valid > 0 and all(tops)


@pytest.mark.parametrize("nc", [33, 34, 35, 36])
def test_binned_client_loop(planets, nc):
    """32 clients and more run the member-binned client loop, whose epilogue
    reads and clears the lane's bins: a group's first 40,000 ranks at R = 36
    (so steps with and without client lines), every quad remainder."""
    # the group of fixed positions (30, 31, 32, 33): C(30, 3) = 4,060 configs, then its successors
    base = sum(_lib.binomial(p, i + 1) for i, p in enumerate((30, 31, 32, 33), start=3))
    assert list(_lib.colex_unrank(base, 7, 36))[:3] == [0, 1, 2]
    valid, _, _ = _check(planets[36], 36, np.arange(nc, dtype=np.uint32), 7, base, base + 40_000)
    assert valid > 0
