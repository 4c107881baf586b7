"""A sweep handle may be destroyed after its planet: bote_sweep_destroy keeps the
planet's device itself and never reads the planet.  A garbage collector that
finalises a DevicePlanet before the Sweep (or MultiDeviceSearch) built on it --
Python's does, in any order, for objects it frees together -- used to make the
destroy switch to a device number read from freed memory, and the refusal stayed
behind as the thread's last HIP error for the next launch to report."""
import numpy as np
import pytest

from fantoch_amd import _lib
from fantoch_amd.bote import DEFAULT_OBJECTIVES, DEFAULT_RANKING, DevicePlanet, MultiDeviceSearch, Sweep
from fantoch_amd.planet import Planet

pytestmark = pytest.mark.gpu


def drop_planet(dp):
    """Destroy the planet handle now, as its finaliser would."""
    _lib.check(_lib.lib().bote_planet_destroy(dp.h))
    dp.h = None


def launched(dp, srv):
    sw = Sweep(dp, srv, srv, 5, DEFAULT_OBJECTIVES, K=20, ranking=DEFAULT_RANKING, digest=True)
    sw.launch()
    r = sw.result()
    return sw, (r.tops, r.valid, r.digest)


def test_sweep_and_search_outlive_their_planet():
    p = Planet.new()
    srv = np.arange(p.R, dtype=np.uint32)
    keep = DevicePlanet(p)
    _, want = launched(keep, srv)
    for _ in range(4):  # (several: freed planets of one size chain through the allocator's free list)
        dp = DevicePlanet(p)
        sw, got = launched(dp, srv)
        assert got == want
        h = MultiDeviceSearch([dp, dp], srv, srv, 5, K=20)
        h.launch()
        assert h.result().tops == want[0]
        drop_planet(dp)
        _lib.check(_lib.lib().bote_search_destroy(h.h))
        h.h = None
        _lib.check(_lib.lib().bote_sweep_destroy(sw.h))
        sw.h = None
        # the next launch reports no error left behind by the destroys
        assert launched(keep, srv)[1] == want
