"""Shared by tests/test_safety_oracle.py (numpy oracle vs goldens, CPU) and tests/test_gpu_safety.py
(device vs goldens): the fixture loader and the comparisons, with the bounds of both.

Bounds (none of them derived from what the code under test returns):

* TTC / JERK of recorded logs: bit-equal (one IEEE subtraction and one division each).
* PET: per row |pet - pet_ref| / (|t1_ref| + |t2_ref|) <= ``PET_BOUND``.  The error is a few ulp of
  cos / sin / hypot amplified by 1/|sin| of the angle between the rays (worst amplification among the
  reference's valid rows 7.7e3, so the scale is 1e-12).  Measured against the reference: numpy oracle
  ``PET_MEASURED_ORACLE``, device ``PET_MEASURED_DEVICE``; the bound is 8x the larger.
* merge: x, y bit-equal; vx, vy, yaw within 4 * 2^-52 relative (one transcendental, one product);
  ax, ay within 64 * 2^-52 * max|v| / min(hd, hs) absolute (a cancelling combination of three
  neighbours).
* metrics of a merged log: TTC within 8 * 2^-52 * (|v_ego| + |v_sv|) / |denom| relative; JERK
  within (the ax / ay bounds of both rows) / |dt| plus 4 ulp; the window's ego columns at the merge
  bounds (copies bit-equal); PET within ``PET_MERGED_FACTOR`` * ``PET_BOUND``
  (the merged vx, vy and yaw each carry up to 4 ulp more, yaw's scaled by |theta| <= pi: about
  4 + 4 + 13 ulp on top of the 8 of four transcendental calls, under 4x).
* means: rel 1e-12 (n <= 1500 non-negative terms, reordering error < n * 2^-53), plus the column's
  own bound.
"""
import json
import os

import numpy as np

import safety_oracle as so
from cvae_amd.safety import COLUMNS, EGO_COLUMNS

HERE = os.path.dirname(os.path.abspath(__file__))
U = 2.0 ** -52
PET_MEASURED_ORACLE = 0.0      # numpy oracle vs the reference, all fixtures (same libm: bit-equal)
PET_MEASURED_DEVICE = 2.6637757552309663e-15  # device vs the reference, worst of the section 1 fixtures (MI355X)
PET_BOUND = 8 * max(PET_MEASURED_ORACLE, PET_MEASURED_DEVICE)
PET_MERGED_FACTOR = 4.0
MAX_EXCLUDED = 1e-3            # share of rows on a validity threshold that may be left out


def load():
    """(meta, logs, pairs): logs[name] / pairs[name] = dict with 'log' (column dict), the
    reference's 'TTC' / 'PET' / 'JERK' and, for pairs, 'track' and 'merged' (7 x L, from start)."""
    z = np.load(os.path.join(HERE, "golden", "safety.npz"))
    meta = json.loads(str(z["meta"]))
    out = {}
    for group, prefix in (("logs", "a/"), ("pairs", "b/")):
        out[group] = {}
        for name, m in meta[group].items():
            d = {"log": {c: np.array(a) for c, a in zip(m["columns"], z[prefix + name + "/cols"])}}
            for k in ("TTC", "PET", "JERK", "track", "merged"):
                if f"{prefix}{name}/{k}" in z.files:
                    d[k] = np.array(z[f"{prefix}{name}/{k}"])
            out[group][name] = d
    return meta, out["logs"], out["pairs"]


def reference_merged(case, m):
    """the reference's merged log of a pair: the source log cut at start + L with its ego columns"""
    n = m["start"] + m["L"]
    log = {k: np.array(c[:n]) for k, c in case["log"].items()}
    for k, c in zip(EGO_COLUMNS, case["merged"]):
        log[k][m["start"]:] = c
    return log


def same_nan(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b))


def bit_equal(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def pet_error(ref_log, scene, i0, i1, pet_ref, pet_got):
    """(max scaled error, excluded rows, max |t1| + |t2| of the valid rows): rows whose validity may
    flip are the reference's own threshold rows (|t1| < 1e-6, |t2| < 1e-6, ||det| - 1e-12| < 1e-13); all others must agree in
    validity"""
    w = {k: c[i0:(None if i1 < 0 else i1 + 1)] for k, c in ref_log.items()}
    o = so.SCENARIOS[scene]["pet"]
    _, t1, t2, det = so.pet_two_rays(w["ego_x"], w["ego_y"], w["ego_vx"], w["ego_vy"], w["ego_yaw"], w[o + "_x"],
                                     w[o + "_y"], w[o + "_vx"], w[o + "_vy"], w[o + "_yaw"], parts=True)
    with np.errstate(all="ignore"):
        edge = (np.abs(t1) < 1e-6) | (np.abs(t2) < 1e-6) | (np.abs(np.abs(det) - 1e-12) < 1e-13)
        keep = ~edge
        assert np.array_equal(np.isnan(pet_ref[keep]), np.isnan(pet_got[keep])), "PET validity differs off-threshold"
        ok = keep & ~np.isnan(pet_ref)
        err = np.abs(pet_got[ok] - pet_ref[ok]) / (np.abs(t1[ok]) + np.abs(t2[ok]))
        tsum = float(np.max(np.abs(t1[ok]) + np.abs(t2[ok]))) if ok.any() else 0.0
    return (float(err.max()) if err.size else 0.0), int(edge.sum()), tsum


def check_stats(m, rec, pet_tol, ttc_exact=True, ttc_tol=0.0, jerk_tol=0.0):
    """the record against the statistics of the reference's main()"""
    s = m["stats"]
    assert rec["n_window"] == m["n_window"] and rec["n_sub"] == s["n_sub"]
    for key, name, ext in (("TTC", "ttc", "min"), ("PET", "pet", "min"), ("JERK", "jerk", "max")):
        assert rec[name + "_count"] == s[key]["count"], key
        if not s[key]["count"]:
            assert np.isnan(rec[name + "_mean"]) and np.isnan(rec[f"{name}_{ext}"])
            continue
        tol = {"TTC": ttc_tol, "PET": pet_tol, "JERK": jerk_tol}[key]
        mean, e = s[key]["mean"], s[key]["ext"]
        assert abs(rec[name + "_mean"] - mean) <= 1e-12 * abs(mean) + tol, (key, rec[name + "_mean"], mean)
        if key != "PET" and ttc_exact:
            assert rec[f"{name}_{ext}"] == e, (key, rec[f"{name}_{ext}"], e)
        else:
            assert abs(rec[f"{name}_{ext}"] - e) <= tol + 1e-12 * abs(e), (key, rec[f"{name}_{ext}"], e)


def check_log_case(m, case, rec, cols):
    """section 1: a recorded log's record and window columns against the reference; returns the
    measured PET error"""
    assert rec["status"] == m["status"]
    if m["status"]:
        assert rec["i0"] == -1 and np.isnan(rec["ttc_mean"])
        return 0.0
    assert (rec["i0"], rec["i1"]) == (m["i0"], m["i1"])
    assert bit_equal(cols["TTC"], case["TTC"]) and bit_equal(cols["JERK"], case["JERK"])
    sl = slice(m["i0"], None if m["i1"] < 0 else m["i1"] + 1)
    for k in EGO_COLUMNS:  # the log's own values
        assert bit_equal(cols[k], case["log"][k][sl]), k
    err, excluded, tsum = pet_error(case["log"], m["scene"], m["i0"], m["i1"], case["PET"], np.asarray(cols["PET"]))
    assert excluded <= MAX_EXCLUDED * len(case["PET"])
    assert err <= PET_BOUND, err
    check_stats(m, rec, pet_tol=PET_BOUND * tsum)
    if m["stats"]["TTC"]["count"]:
        assert rec["decel"] == m["stats"]["decel"] and rec["yaw_max"] == m["stats"]["yaw_max"]
    return err


def check_merge(m, case, got):
    """section 2: merged ego columns of a pair; returns the measured maxima (relative v, yaw; a / bound)"""
    assert (got["start"], got["L"]) == (m["start"], m["L"])
    s, L = m["start"], m["L"]
    for k in EGO_COLUMNS:  # before the start row: the log's own values
        assert bit_equal(got[k][:s], case["log"][k][:s]), k
    x, y, vx, vy, ax, ay, yaw = case["merged"]
    g = {k: got[k][s:] for k in EGO_COLUMNS}
    assert bit_equal(g["ego_x"], x) and bit_equal(g["ego_y"], y)
    out = {}
    for k, r in (("ego_vx", vx), ("ego_vy", vy), ("ego_yaw", yaw)):
        v = np.abs(case["track"][:L, 3]) if k != "ego_yaw" else np.abs(r)
        e = np.abs(g[k] - r)
        assert np.all(e <= 4 * U * v), k
        out[k] = float(np.max(e / np.maximum(v, 1e-300)) / U)
    bound = accel_bound(case["log"]["frame"][s:s + L], case["track"][:L, 3])
    for k, r in (("ego_ax", ax), ("ego_ay", ay)):
        e = np.abs(g[k] - r)
        assert np.all(e <= bound), k
        out[k] = float(np.max(e / bound))
    return out


def accel_bound(t, v):
    """64 * 2^-52 * max|v| / min(hd, hs) per row of a merged segment"""
    if len(t) < 2:
        return np.full(len(t), U)
    d = np.abs(np.diff(t))
    h = np.minimum(np.r_[d[0], d], np.r_[d, d[-1]])
    return 64 * U * np.max(np.abs(v)) / h


def check_track_case(m, case, rec, cols):
    """section 3: the record and window columns of a merged pair against the reference's metrics of
    its own merged log; returns (measured PET error, rows with |denom| < 1e-6)"""
    S = so.SCENARIOS[m["scene"]]
    assert rec["status"] == 0 and (rec["start"], rec["L"]) == (m["start"], m["L"])
    assert (rec["i0"], rec["i1"], rec["n_window"]) == (m["i0"], m["i1"], m["n_window"])
    ref = reference_merged(case, m)
    sl = slice(m["i0"], None if m["i1"] < 0 else m["i1"] + 1)
    w = {k: c[sl] for k, c in ref.items()}
    # the window's merged ego columns: copies bit-equal (x, y everywhere; every column before the
    # start row), the rest at the section 2 bounds
    rows = np.arange(m["i0"], m["i0"] + m["n_window"])
    on = rows >= m["start"]
    k_on = rows[on] - m["start"]
    ab, vb = np.zeros(len(rows)), np.zeros(len(rows))
    ab[on] = accel_bound(case["log"]["frame"][m["start"]:m["start"] + m["L"]], case["track"][:m["L"], 3])[k_on]
    vb[on] = 4 * U * np.abs(case["track"][k_on, 3])
    for k, b in (("ego_x", 0.0), ("ego_y", 0.0), ("ego_vx", vb), ("ego_vy", vb), ("ego_ax", ab), ("ego_ay", ab),
                 ("ego_yaw", 4 * U * np.abs(w["ego_yaw"]) * on)):
        g = np.asarray(cols[k])
        assert g.shape == w[k].shape and same_nan(g, w[k]), k
        assert np.all(np.nan_to_num(np.abs(g - w[k])) <= b), k
    sv, axis = S["ttc"]
    denom = w["ego_v" + axis] - w[sv + "_v" + axis]
    near = np.abs(denom) < 1e-6  # the only rows whose TTC sign or NaN status may differ
    assert near.sum() <= MAX_EXCLUDED * len(denom)
    ttc_ref, ttc = case["TTC"], np.asarray(cols["TTC"])
    assert same_nan(ttc_ref[~near], ttc[~near])
    ok = ~near & ~np.isnan(ttc_ref)
    with np.errstate(all="ignore"):
        tb = 8 * U * (np.abs(w["ego_v" + axis]) + np.abs(w[sv + "_v" + axis])) / np.abs(denom) * np.abs(ttc_ref)
    assert np.all(np.abs(ttc - ttc_ref)[ok] <= tb[ok])
    assert np.array_equal(np.sign(ttc[ok]), np.sign(ttc_ref[ok]))
    # JERK: both accelerations within the merge bound, divided by the row's step
    jerk_ref, jerk = case["JERK"], np.asarray(cols["JERK"])
    assert same_nan(jerk_ref, jerk)
    dt = np.r_[1.0, np.abs(np.diff(w["sim_time"]))] if m["has_time"] else S["dt"]
    with np.errstate(all="ignore"):
        jb = (ab + np.r_[0.0, ab[:-1]]) / dt + 4 * U * np.abs(np.nan_to_num(jerk_ref))
    okj = ~np.isnan(jerk_ref)
    assert np.all(np.abs(jerk - jerk_ref)[okj] <= jb[okj])
    err, excluded, tsum = pet_error(ref, m["scene"], m["i0"], m["i1"], case["PET"], np.asarray(cols["PET"]))
    assert excluded <= MAX_EXCLUDED * len(case["PET"])
    assert err <= PET_MERGED_FACTOR * PET_BOUND, err
    with np.errstate(all="ignore"):
        ttc_tol = float(np.nanmax(np.where(ok, tb, 0.0))) if ok.any() else 0.0
    check_stats(m, rec, pet_tol=PET_MERGED_FACTOR * PET_BOUND * tsum, ttc_exact=False,
                ttc_tol=ttc_tol, jerk_tol=float(np.max(jb[okj])) if okj.any() else 0.0)
    st = m["stats"]
    if st["TTC"]["count"]:  # extremes of a merged column over the TTC-valid rows: that column's bound
        assert abs(rec["decel"] - st["decel"]) <= ab.max() and abs(rec["yaw_max"] - st["yaw_max"]) <= 4 * U * abs(st["yaw_max"])
    else:
        assert np.isnan(rec["decel"]) and np.isnan(rec["yaw_max"])
    return err, int(near.sum())


def oracle_case(log, track, scene):
    """(m, case) in the fixtures' form from the numpy oracle (itself bit-equal to the reference on
    the fixtures), so the synthetic shapes go through the same per-column checks; track None =
    the log as recorded.  m["status"] != 0: no columns."""
    if track is None:
        rec, cols = so.record(log, scene, rows=True)
        merged = None
    else:
        rec, cols = so.track_record(log, track, scene, rows=True)
        mg = so.merge(log, track)
        merged = None if mg is None else np.stack([mg[0][k][mg[1]:] for k in EGO_COLUMNS])
    f = lambda v: None if np.isnan(v) else float(v)  # noqa: E731
    m = {"scene": scene, "status": rec["status"], "has_time": "sim_time" in log, "start": rec["start"], "L": rec["L"],
         "i0": rec["i0"], "i1": rec["i1"], "n_window": rec["n_window"], "record": rec,
         "stats": {"TTC": {"count": rec["ttc_count"], "mean": f(rec["ttc_mean"]), "ext": f(rec["ttc_min"])},
                   "PET": {"count": rec["pet_count"], "mean": f(rec["pet_mean"]), "ext": f(rec["pet_min"])},
                   "JERK": {"count": rec["jerk_count"], "mean": f(rec["jerk_mean"]), "ext": f(rec["jerk_max"])},
                   "n_sub": rec["n_sub"], "decel": f(rec["decel"]), "yaw_max": f(rec["yaw_max"])}}
    case = {"log": log, "track": None if track is None else np.asarray(track, np.float64).reshape(-1, 4),
            "merged": merged}
    if cols is not None:
        case.update(TTC=cols["TTC"], PET=cols["PET"], JERK=cols["JERK"])
    return m, case


def check_no_window(m, rec, cols):
    """a track or log without metrics (NO_WINDOW, EMPTY, NO_START): the integer fields, NaN
    elsewhere, no rows"""
    for k, v in m["record"].items():
        assert (np.isnan(v) and np.isnan(rec[k])) if isinstance(v, float) else rec[k] == v, (k, rec[k], v)
    assert cols is None or all(len(c) == 0 for c in cols.values())


def log_columns(log):
    """a fixture log as the column dict SceneLogs takes (absent columns stay absent)"""
    return {k: log[k] for k in COLUMNS if k in log}
