"""GPU checks of cvae_amd.safety (csrc/cvae_safety.h through cvae_safety_metrics).

Sections 1-3 compare the device with the reference's own outputs (tests/golden/safety.npz) at the
bounds written down in tests/safety_checks.py.  The synthetic edge shapes are compared with the
numpy oracle (tests/safety_oracle.py, itself bit-equal to the reference on the fixtures) through
the same checks and the same per-column bounds: integer fields, NaN patterns and every copied
value (x, y, the log's own columns, TTC and JERK of unmerged rows) exactly, the rest at the section
1-3 bounds.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.join(os.path.dirname(HERE), "defensive-model-vae_amd")]
import safety_checks as sc  # noqa: E402
import safety_oracle as so  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def S():
    from cvae_amd import safety
    return safety


@pytest.fixture(scope="module")
def gold():
    return sc.load()


def rec_of(out, p, S):
    return {k: (int(out[k][p]) if out[k].dtype.kind == "i" else float(out[k][p])) for k in S.RECORD_FIELDS}


def cols_of(out, p, S):
    return {k: out[k][p] for k in S.ROW_COLUMNS}


# ---- 1. recorded logs ------------------------------------------------------------------------------
def test_recorded_logs_match_reference(S, gold):
    meta, logs, _ = gold
    worst = 0.0
    for scene in range(4):
        names = [n for n, m in meta["logs"].items() if m["scene"] == scene]
        L = S.SceneLogs([sc.log_columns(logs[n]["log"]) for n in names], scene)
        out = S.log_safety(L, rows=True)
        for p, n in enumerate(names):
            err = sc.check_log_case(meta["logs"][n], logs[n], rec_of(out, p, S), cols_of(out, p, S))
            print(f"{n}: PET scaled error (device vs reference) {err:.3e}")
            worst = max(worst, err)
    print(f"worst PET scaled error {worst!r} (recorded {sc.PET_MEASURED_DEVICE:.3e}, bound {sc.PET_BOUND:.3e})")


# ---- 2. merge ----------------------------------------------------------------------------------------
def test_merge_matches_reference(S, gold):
    meta, _, pairs = gold
    for n, m in meta["pairs"].items():
        L = S.SceneLogs([sc.log_columns(pairs[n]["log"])], m["scene"])
        got = S.merge_tracks([pairs[n]["track"]], L, [0])[0]
        print(n, "measured maxima (ulp of |v| / |yaw|; share of the ax, ay bound):", sc.check_merge(m, pairs[n], got))


# ---- 3. merged metrics -------------------------------------------------------------------------------
def test_merged_metrics_match_reference(S, gold):
    """the fixtures hold 0 rows with |denom| < 1e-6 (the only rows whose TTC sign / NaN may differ)"""
    meta, _, pairs = gold
    near = 0
    for n, m in meta["pairs"].items():
        L = S.SceneLogs([sc.log_columns(pairs[n]["log"])], m["scene"])
        out = S.track_safety([pairs[n]["track"]], L, [0], rows=True)
        err, k = sc.check_track_case(m, pairs[n], rec_of(out, 0, S), cols_of(out, 0, S))
        print(f"{n}: PET scaled error {err:.3e}, rows with |denom| < 1e-6: {k}")
        near += k
    assert near == 0


# ---- 4. edge shapes ----------------------------------------------------------------------------------
def synth_log(scene, n, seed, has_time=True, sub=True, start=True, end=True, uniform=True):
    """a log whose scenario window opens around n/4 and closes around 3n/4"""
    r = np.random.default_rng(seed)
    i = np.arange(n, dtype=np.float64)
    f = i / max(n - 1, 1)
    log = {k: r.uniform(-1.0, 1.0, n) for k in S_COLUMNS}
    log["frame"] = i if uniform else np.cumsum(r.integers(1, 4, n)).astype(np.float64)
    log["sim_time"] = np.cumsum(r.uniform(0.015, 0.03, n))
    for k in ("ego_vx", "sv1_vx", "sv2_vx"):
        log[k] = r.uniform(0.5, 2.0, n)
    for k in ("ego_vy", "sv1_vy", "sv2_vy"):
        log[k] = r.uniform(3.0, 9.0, n)
    log["ego_yaw"] = r.uniform(80.0, 100.0, n)
    log["sv1_yaw"] = r.uniform(-20.0, 20.0, n)
    log["sv2_yaw"] = r.uniform(160.0, 200.0, n)
    q = n // 4
    if scene == 0:
        log["ego_x"], log["ego_y"] = -192.0 + 0.01 * i, (-10.0 + 110.0 * f if end else -10.0 + 60.0 * f)
        log["sv2_vx"][:q] = 0.0
        if not start:
            log["sv2_vy"][:] = 0.0
        log["sv2_x"] = -199.0 + 9.0 * f if sub else np.full(n, -100.0)
    elif scene == 1:
        log["ego_x"], log["ego_y"] = (-150.0 - 50.0 * f if end else -150.0 - 10.0 * f), 0.01 * i
        log["sv1_yaw"] = np.where(i >= q, -160.0, 0.0) if start else np.zeros(n)
        log["ego_ax"] = r.uniform(-3.0, 3.0, n)
        if sub:
            log["ego_ax"][n // 2] = 150.0
        else:
            log["ego_ax"][q if start else 0] = 150.0  # the window's first row: .loc[:-1] is empty
    elif scene == 2:
        log["ego_x"], log["ego_y"] = 155.0 + 0.01 * i, (60.0 - 160.0 * f if end else 60.0 - 100.0 * f)
        if not start:
            log["sv1_vx"][:] = 0.0
        log["sv1_x"] = 150.0 + 10.0 * f if sub else np.full(n, 200.0)
    else:
        log["ego_x"], log["ego_y"] = np.full(n, 16.0) + 0.01 * f, 200.0 - 200.0 * f
        log["sv1_x"] = 9.0 + 8.0 * f if sub else np.full(n, 9.0)
        log["sv1_y"] = log["ego_y"] - 20.0
        log["sv1_ax"] = np.where(i < 3 * q, 0.5, 0.05 if end else 0.0)
        log["sv1_ax"][:q] = 0.0
        if not start:
            log["sv1_ax"][:] = 0.0
        log["sv1_yaw"] = np.full(n, -95.0)
    if not has_time:
        del log["sim_time"]
    return log


S_COLUMNS = ("frame", "sim_time", "ego_x", "ego_y", "ego_vx", "ego_vy", "ego_ax", "ego_ay", "ego_yaw", "sv1_x",
             "sv1_y", "sv1_vx", "sv1_vy", "sv1_ax", "sv1_yaw", "sv2_x", "sv2_y", "sv2_vx", "sv2_vy", "sv2_yaw")


def synth_track(log, s, n, seed):
    """a track of n rows starting beside log row s and following the log's ego path"""
    r = np.random.default_rng(seed)
    m = len(log["ego_x"])
    idx = np.minimum(s + np.arange(n), m - 1)
    t = np.empty((n, 4))
    t[:, 0] = log["ego_x"][idx] + 1e-4
    t[:, 1] = log["ego_y"][idx] + 1e-4
    t[:, 2] = np.deg2rad(90.0) + r.uniform(-0.15, 0.15, n)
    t[:, 3] = r.uniform(3.0, 20.0, n)
    return t


def check_vs_oracle(S, out, p, log, track, scene, merged=None):
    """track p of a rows=True result against the oracle; track None = the log as recorded"""
    m, case = sc.oracle_case(log, track, scene)
    rec, cols = rec_of(out, p, S), cols_of(out, p, S)
    if m["status"]:
        sc.check_no_window(m, rec, cols)
    elif track is None:
        sc.check_log_case(m, case, rec, cols)
    else:
        sc.check_track_case(m, case, rec, cols)
    if merged is not None and m["status"] != S.EMPTY:
        sc.check_merge(m, case, merged)
    return m


@pytest.mark.parametrize("scene", [0, 1, 2, 3])
def test_track_lengths_and_shared_log(S, scene):
    """lengths 0, 1, 2, 3, 63, 64, 65, 129; start at the last row (L = 1); a track longer than the
    rows that remain; a track ending inside the window; 65 tracks on one log; uniform and
    non-uniform frame steps"""
    for uniform in (True, False):
        log = synth_log(scene, 200, 10 + scene, uniform=uniform, has_time=uniform)
        tracks = [synth_track(log, 40 + 3 * k, n, k) for k, n in enumerate((0, 1, 2, 3, 63, 64, 65, 129))]
        tracks.append(synth_track(log, 199, 5, 20))      # start at the log's last row: L = 1
        tracks.append(synth_track(log, 150, 129, 21))    # longer than the rows that remain
        tracks.append(synth_track(log, 60, 40, 22))      # ends inside the scenario window
        tracks += [synth_track(log, 3 * k, 30 + k, 30 + k) for k in range(54)]
        assert len(tracks) == 65
        L = S.SceneLogs([log], scene)
        out = S.track_safety(tracks, L, [0] * len(tracks), rows=True)
        merged = S.merge_tracks(tracks, L, [0] * len(tracks))
        assert merged[0] is None
        for p, t in enumerate(tracks):
            check_vs_oracle(S, out, p, log, t, scene, merged[p])
        assert out["status"][0] == S.EMPTY and out["L"][8] == 1 and out["start"][8] == 199
        assert out["start"][9] + out["L"][9] == 200
        two = S.track_safety(tracks[4:6], L, [0, 0], rows=True)
        for p in range(2):
            check_vs_oracle(S, two, p, log, tracks[4 + p], scene)


@pytest.mark.parametrize("scene", [0, 1, 2, 3])
def test_windows_and_sub_windows(S, scene):
    """no start row (NO_WINDOW), no end row (window to the end), each sub-window empty and
    non-empty, a log without sim_time — logs as recorded and with a track merged"""
    logs = [synth_log(scene, 150, 1, sub=True), synth_log(scene, 150, 2, sub=False),
            synth_log(scene, 150, 3, start=False), synth_log(scene, 150, 4, end=False),
            synth_log(scene, 150, 5, has_time=False), synth_log(scene, 70, 6, uniform=False)]
    L = S.SceneLogs(logs, scene)
    out = S.log_safety(L, rows=True)
    for p, g in enumerate(logs):
        check_vs_oracle(S, out, p, g, None, scene)
    assert out["status"][2] == S.NO_WINDOW and out["i1"][3] == -1 and out["i0"][3] >= 0
    assert out["n_sub"][0] > 0 and out["n_sub"][1] == 0
    tracks = [synth_track(g, 30, 90, 40 + k) for k, g in enumerate(logs)]
    outm = S.track_safety(tracks, L, np.arange(len(logs)), rows=True)
    for p, (g, t) in enumerate(zip(logs, tracks)):
        check_vs_oracle(S, outm, p, g, t, scene)


def test_one_row_window_nan_rows_tie_and_empty_population(S):
    # a window of one row: JERK all NaN
    log = synth_log(0, 80, 7)
    log["ego_y"][:] = -1.0
    log["ego_y"][50] = 90.0  # the only row with ego_y > 0 also ends the window
    L = S.SceneLogs([log], 0)
    out = S.log_safety(L, rows=True)
    assert (out["i0"][0], out["i1"][0], out["n_window"][0], out["jerk_count"][0]) == (50, 50, 1, 0)
    assert np.isnan(out["JERK"][0]).all() and np.isnan(out["jerk_mean"][0])
    check_vs_oracle(S, out, 0, log, None, 0)
    # NaN ego_x rows, one of them at the true minimum; and a tie in the distance: the lowest index wins
    log = synth_log(2, 100, 8)
    t = synth_track(log, 40, 20, 1)
    log["ego_x"][[3, 40, 77]] = np.nan
    log["ego_x"][60], log["ego_y"][60] = log["ego_x"][20], log["ego_y"][20]
    tie = synth_track(log, 20, 10, 2)
    tie[0, :2] = log["ego_x"][20], log["ego_y"][20]
    L = S.SceneLogs([log], 2)
    out = S.track_safety([t, tie], L, [0, 0], rows=True)
    want = [check_vs_oracle(S, out, 0, log, t, 2), check_vs_oracle(S, out, 1, log, tie, 2)]
    assert want[0]["start"] != 40 and want[1]["start"] == 20 and out["start"][1] == 20
    # P = 0
    out = S.track_safety([], L, [])
    assert all(len(out[k]) == 0 for k in S.RECORD_FIELDS)
    assert S.summary(out)["n_tracks"] == 0


# ---- 5. determinism and geometry ---------------------------------------------------------------------
def test_bit_identical_across_order_and_geometry(S, gold):
    meta, _, pairs = gold
    n = "sce3_exp8_2"
    log, tr = pairs[n]["log"], pairs[n]["track"]
    L = S.SceneLogs([sc.log_columns(log), synth_log(2, 300, 3)], 2)
    tracks = [tr[k:k + 100 + 37 * k] for k in range(12)] + [synth_track(synth_log(2, 300, 3), 50, 120, 9)]
    lot = [0] * 12 + [1]
    base = S.track_safety(tracks, L, lot, rows=True)
    perm = np.random.default_rng(0).permutation(len(tracks))
    inv = np.argsort(perm)
    runs = [S.track_safety(tracks, L, lot, rows=True, block_waves=w) for w in (1, 4, 8)]
    sh = S.track_safety([tracks[i] for i in perm], L, [lot[i] for i in perm], rows=True)
    runs.append({k: (v[inv] if isinstance(v, np.ndarray) else [v[i] for i in inv])
                 for k, v in sh.items() if k != "row_offsets"})
    runs.append(S.track_safety(tracks, L, lot, rows=True))
    for r in runs:
        for k in S.RECORD_FIELDS:
            assert sc.bit_equal(r[k], base[k]), k
        for k in S.ROW_COLUMNS:
            assert all(sc.bit_equal(a, b) for a, b in zip(r[k], base[k])), k


# ---- 6. invalid input (with a device present: nothing is launched) -----------------------------------
def test_invalid_input_raises(S):
    from cvae_amd._lib import CvaeError
    log = synth_log(0, 50, 1)
    L = S.SceneLogs([log], 0)
    t = synth_track(log, 10, 10, 1)
    with pytest.raises(CvaeError, match="log_of_track outside the logs"):
        S.track_safety([t], L, [1])
    nan_log = dict(log, ego_x=np.full(50, np.nan))
    with pytest.raises(CvaeError, match="no finite ego_x/ego_y row"):
        S.track_safety([t], S.SceneLogs([nan_log], 0), [0])
    import torch
    st = torch.from_numpy(t).cuda()
    with pytest.raises(CvaeError, match="end at n_rows"):
        S.track_safety((st, np.array([0, 9], np.int64)), L, [0])
    with pytest.raises(CvaeError, match="monotone"):
        S.track_safety((st, np.array([0, 12, 10], np.int64)), L, [0, 0])


# ---- 7. pipeline -------------------------------------------------------------------------------------
def test_checkpoint_safety_equals_staged_host_run(S, monkeypatch):
    """generate -> track on the device -> safety, against generate -> mpc.track_batch on the host
    -> track_safety.  As in test_gpu_validate, the fixed test weights do not produce increasing
    times, so the generator is replaced by one returning the sce1 log tracks of mpc.npz."""
    from cvae_amd import mpc, tools
    M = np.load(os.path.join(HERE, "golden", "mpc.npz"))
    wps = [M[f"c{k}/waypoints"] for k in (2, 3)]
    start_states = np.array([M[f"c{k}/init"] for k in (2, 3)])

    def fake_generate(model_path, start_points, seq_len, dim, latent_dim, z=None, device=None):
        out = np.stack([w[:, [2, 0, 1]] for w in wps])
        out[:, 0, 0] = -0.01
        return out

    monkeypatch.setattr(tools, "generate_trajectories", fake_generate)
    log = synth_log(0, 600, 5, has_time=False)
    log["ego_x"] = np.linspace(wps[0][0, 0], wps[0][-1, 0], 600)
    log["ego_y"] = np.linspace(wps[0][0, 1] - 5.0, wps[0][-1, 1] + 5.0, 600)
    L = S.SceneLogs([log], "sce1")
    tm = {}
    r = S.checkpoint_safety("ckpt.pth", start_states, L, [0, 0], seq_len=10, dim=3, latent_dim=8, timings=tm)
    assert set(tm) == {"generate", "track", "safety"}
    host = mpc.track_batch([w.copy() for w in wps], start_states, prediction_horizon=30, control_horizon=20, dt=0.02)
    rh = S.track_safety([st for _, st, _ in host], L, [0, 0])
    for k in S.RECORD_FIELDS:
        assert sc.bit_equal(r[k], rh[k]), k
    assert (r["L"] > 2).all() and (r["status"] == S.OK).any() and (r["ttc_count"] + r["jerk_count"]).max() > 0
