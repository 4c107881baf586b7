"""Host-side pieces of bench.py (CPU): the work-per-config figures DESIGN.md
§5 quotes, the workload table, the CPU-share rule and a small run of the
CPU baseline (the oracle over a seeded uniform rank sample, with the
workload's key set and objectives)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_work_per_config_figures():
    # SURVEY.md §8d W, and the documented replacement W' 
    assert bench.work_per_config(7, 64) == 2955
    assert bench.work_per_config_group(7, 64) == 968
    assert bench.work_per_config_group(6, 128) == 1780
    assert bench.work_per_config_keys(6, 128) == 2632


def test_workloads_name_the_baseline_configs():
    w = bench.workloads()
    assert (w["r64n7"]["R"], w["r64n7"]["n"], w["r64n7"]["keys"]) == (64, 7, 0)
    assert (w["r128n6"]["R"], w["r128n6"]["n"], w["r128n6"]["keys"]) == (128, 6, 1)
    assert w["r128n6_base"]["keys"] == 0
    assert w["gcp"]["R"] is None


def test_cpu_share_follows_omp_num_threads(monkeypatch):
    monkeypatch.setenv("OMP_NUM_THREADS", "1")
    assert bench.host_cpu_share() == 1
    monkeypatch.setenv("OMP_NUM_THREADS", "not-a-number")
    assert bench.host_cpu_share() >= 1


@pytest.mark.parametrize("keys", [0, 1])
def test_cpu_baseline_small_sample(monkeypatch, keys):
    from fantoch_amd.bote import CONFIG5_OBJECTIVES, DEFAULT_OBJECTIVES
    from fantoch_amd.planet import Planet

    monkeypatch.setenv("OMP_NUM_THREADS", "2")
    objs = CONFIG5_OBJECTIVES if keys else DEFAULT_OBJECTIVES
    cb = bench.cpu_baseline(Planet.synthetic(64), 5, keys=keys, objectives=objs, budget_s=0.05, nsample=600,
                            cap_s=0.05)
    assert cb["kind"] == "port" and cb["unit"] == "configs/s" and cb["cores"] == 2
    assert cb["value"] > 0 and cb["single_thread"]["value"] > 0
    assert f"{len(objs)} objectives" in cb["sample"]
    assert ("extended key set" in cb["sample"]) == bool(keys)
    assert "drawn uniformly" in cb["sample"]


def test_profile_figures_only_for_the_profiled_build():
    """the line's VALU issue utilisation and HBM traffic come from
    profiles/pmc.json / traffic.json; they are quoted only when those were
    measured on the library being benched (bench.lib_build)."""
    pmc = {"valu_insts_per_config": 869.0, "clock_ghz": 2.35, "build": "aaaa", "source": "x"}
    traffic = {"bytes": 7.5e7, "build": "aaaa"}
    valu, tb, stale = bench.profile_figures(pmc, traffic, "aaaa", 621216192, 14.45)
    assert valu["same_build"] and 0.4 < valu["util"] < 0.6
    assert tb == 7.5e7 and stale == []
    valu, tb, stale = bench.profile_figures(pmc, traffic, "bbbb", 621216192, 14.45)
    assert valu["util"] is None and not valu["same_build"]
    assert tb is None and len(stale) == 2
    # a figure without a build (before round 5) is never quoted
    valu, tb, stale = bench.profile_figures(dict(pmc, build=None), None, "bbbb", 1, 1.0)
    assert valu["util"] is None and tb is None and len(stale) == 1


def test_dump_outputs_round_trips_a_result(tmp_path):
    """--dump-outputs: every record's key comes back as the figure it orders by
    (include/bote_hip.h bote_topk_record), short lists are padded with -1, and
    the 64-bit digest is exact as two 32-bit halves."""
    import numpy as np

    from fantoch_amd import _lib
    from fantoch_amd.bote import SweepResult, _orderable

    scores = np.array([250.5, 0.0, -3.25])
    covs = np.array([0.125, 0.5])
    tops = [[(int(k), r) for k, r in zip(~_orderable(scores), (7, 8, 9))],
            [(1234, 5), (1234, 6), (99999, 1)],
            [(int(k), r) for k, r in zip(covs.view(np.uint64), (621216191, 3))]]
    objs = [(_lib.OBJ_SCORE, 0), (_lib.OBJ_MEAN, _lib.SLOT_AF1), (_lib.OBJ_COV, _lib.SLOT_AF1)]
    digest = 0xFEDCBA9876543210
    bench.dump_outputs(str(tmp_path / "d"), objs, 4, SweepResult(tops, 32380967, digest), prefix="p_")
    got = {n: np.load(tmp_path / "d" / f"p_{n}.npy") for n in ("tops_value", "tops_rank", "tops_count", "valid",
                                                              "digest")}
    assert all(a.dtype == np.float64 for a in got.values())
    assert got["tops_count"].tolist() == [3, 3, 2] and got["valid"].tolist() == [32380967]
    assert got["tops_value"].tolist() == [[250.5, 0.0, -3.25, -1], [1234, 1234, 99999, -1], [0.125, 0.5, -1, -1]]
    assert got["tops_rank"].tolist() == [[7, 8, 9, -1], [5, 6, 1, -1], [621216191, 3, -1, -1]]
    assert (int(got["digest"][0]) << 32) | int(got["digest"][1]) == digest


def test_lib_build_is_the_loaded_library():
    from fantoch_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    b = bench.lib_build()
    assert len(b) == 16 and int(b, 16) >= 0
