"""CPU: the numpy oracle of the safety stage (tests/safety_oracle.py) against the reference's own
outputs recorded in tests/golden/safety.npz (tests/golden/make_safety_goldens.py), and the scenario
table of cvae_amd.safety against the constants of csrc/cvae_safety.h."""
import os
import re

import numpy as np
import pytest

import safety_checks as sc
import safety_oracle as so
from conftest import ROOT
from cvae_amd import safety


@pytest.fixture(scope="module")
def gold():
    return sc.load()


def test_fixture_covers_what_the_issue_asks(gold):
    meta, logs, pairs = gold
    assert {m["scene"] for m in meta["logs"].values()} == {0, 1, 2, 3}
    assert {m["has_time"] for m in meta["logs"].values()} == {True, False}
    assert meta["logs"]["BEHAVIOR_UnpredictableMovementTown04"]["status"] == safety.NO_WINDOW
    assert {m["scene"] for m in meta["pairs"].values()} == {0, 1, 2, 3}
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "safety.npz")) < 1 << 20


def test_recorded_logs_match_reference(gold):
    meta, logs, _ = gold
    worst = 0.0
    for name, m in meta["logs"].items():
        rec, cols = so.record(logs[name]["log"], m["scene"], rows=True)
        err = sc.check_log_case(m, logs[name], rec, cols)
        print(f"{name}: PET scaled error (oracle vs reference) {err:.3e}")
        worst = max(worst, err)
    print(f"worst {worst:.3e} (recorded {sc.PET_MEASURED_ORACLE:.3e}, bound {sc.PET_BOUND:.3e})")


def test_merge_matches_reference(gold):
    meta, _, pairs = gold
    for name, m in meta["pairs"].items():
        merged, start, L = so.merge(pairs[name]["log"], pairs[name]["track"])
        got = {k: merged[k] for k in safety.EGO_COLUMNS}
        got.update(start=start, L=L)
        print(name, sc.check_merge(m, pairs[name], got))


def test_merged_metrics_match_reference(gold):
    meta, _, pairs = gold
    near = 0
    for name, m in meta["pairs"].items():
        rec, cols = so.track_record(pairs[name]["log"], pairs[name]["track"], m["scene"], rows=True)
        err, n = sc.check_track_case(m, pairs[name], rec, cols)
        print(f"{name}: PET scaled error {err:.3e}, rows with |denom| < 1e-6: {n}")
        near += n
    assert near == 0  # the fixtures hold no row whose TTC sign or NaN status may differ


def test_dynamic_sub_window_label_slice():
    """result.loc[:first - 1] after reset_index: empty for first = 0, rows before the hit otherwise"""
    w = {"ego_ax": np.array([100.0, 0.0, 0.0]), "ego_x": np.zeros(3)}
    assert not so.sub_window(w, 1).any()
    w["ego_ax"] = np.array([0.0, 0.0, 250.0])
    assert so.sub_window(w, 1).tolist() == [True, True, False]
    w["ego_ax"] = np.zeros(3)
    assert so.sub_window(w, 1).all()


def test_gradient_segment_of_one_row_is_zero():
    log = {k: np.arange(5.0) for k in safety.COLUMNS}
    merged, start, L = so.merge(log, np.array([[4.0, 4.0, 0.3, 2.0], [9.0, 9.0, 0.3, 2.0]]))
    assert (start, L) == (4, 1) and merged["ego_ax"][4] == 0.0 and merged["ego_ay"][4] == 0.0


def test_scenario_table_matches_kernel_constants():
    """one table: safety.SCENARIOS (the oracle's) and the SF_* constants of csrc/cvae_safety.h"""
    txt = open(os.path.join(ROOT, "defensive-model-vae_amd", "csrc", "cvae_safety.h")).read()
    c = {k: float(v) for k, v in re.findall(r"^#define (SF_[A-Z0-9_]+) (-?[0-9.]+(?:e-?[0-9]+)?)\b", txt, re.M)}
    S = safety.SCENARIOS
    assert (c["SF_EPS_V"], c["SF_EPS_DET"]) == (safety.EPS_V, safety.EPS_DET)
    assert [c["SF_DT_" + k] for k in ("STATIC", "DYNAMIC", "PREDICTABLE", "UNPREDICTABLE")] == [s["dt"] for s in S]
    assert c["SF_STATIC_END_Y"] == S[0]["end_y"] and (c["SF_SUB_STATIC_LO"], c["SF_SUB_STATIC_HI"]) == S[0]["sub"]
    assert (c["SF_DYNAMIC_START_YAW"], c["SF_DYNAMIC_END_X"], c["SF_SUB_DYNAMIC_AX"]) == \
        (S[1]["start_yaw"], S[1]["end_x"], S[1]["sub"])
    assert (c["SF_PREDICTABLE_START_Y"], c["SF_PREDICTABLE_END_Y"], c["SF_SUB_PREDICTABLE_X"]) == \
        (S[2]["start_y"], S[2]["end_y"], S[2]["sub"])
    assert (c["SF_UNPRED_DIST"], c["SF_UNPRED_AX"], c["SF_UNPRED_END_YAW"], c["SF_UNPRED_END_X"]) == \
        (S[3]["dist"], S[3]["ax"], S[3]["end_yaw"], S[3]["end_x"])
    assert (c["SF_SUB_LANE_X1"], c["SF_SUB_LANE_Y1"], c["SF_SUB_LANE_X2"], c["SF_SUB_LANE_Y2"]) == S[3]["sub"]
    names = re.search(r"enum \{ SF_FRAME = 0,(.*?)SF_NCOL \}", txt, re.S).group(1)
    cols = ["frame"] + [n.strip()[3:].lower() for n in names.split(",") if n.strip()]
    assert cols == [k.replace("sim_time", "time") for k in safety.COLUMNS]
    rec = re.search(r"enum \{ SF_R_STATUS = 0,(.*?)SF_REC \}", txt, re.S).group(1)
    assert len([n for n in rec.split(",") if n.strip()]) + 1 == len(safety.RECORD_FIELDS)


def test_summary_population_view():
    rec = {"status": np.array([0, 0, 1, 0]), "ttc_min": np.array([2.0, 1.0, np.nan, 3.0]),
           "pet_min": np.array([np.nan, 0.5, np.nan, np.nan])}
    s = safety.summary(rec)
    assert s["window_share"] == 0.75 and s["ttc_min_min"] == 1.0 and s["ttc_min_median"] == 2.0
    assert s["pet_min_count"] == 1 and s["pet_min_p05"] == 0.5
    assert safety.scene_id("vae_offset_sce3_cond") == 2 and safety.scene_id("DynamicBlindTown05") == 1
