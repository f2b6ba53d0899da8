"""numpy restatement of the reference's SUT_Testing stage (``Defensive_Testing.py`` write-back +
``tools/Metrics_Calculation.py`` metrics), the CPU oracle of ``cvae_amd.safety``.

A log is a dict of float64 columns (``cvae_amd.safety.COLUMNS``; ``sim_time`` may be absent), a track
an [n, 4] array (x, y, theta, v).  No pandas: every step is the numpy operation the reference's
pandas call performs, in its order.  The scenario constants come from ``safety.SCENARIOS``, the
one table the kernel mirrors.
"""
import numpy as np

from cvae_amd.safety import EGO_COLUMNS, EMPTY, EPS_DET, EPS_V, NO_START, NO_WINDOW, OK, RECORD_FIELDS, SCENARIOS


def find_start(log, x0, y0):
    """find_best_start_row (Defensive_Testing.py:156-163); None where np.nanargmin raises"""
    d2 = (log["ego_x"] - x0) ** 2 + (log["ego_y"] - y0) ** 2
    return None if np.isnan(d2).all() else int(np.nanargmin(d2))


def merge(log, track):
    """merge_trajectory_into_csv (:166-205): (merged log, start, L), or None for an empty track / log"""
    track = np.asarray(track, np.float64).reshape(-1, 4)
    n_log = len(log["ego_x"])
    if n_log == 0 or len(track) == 0:
        return None
    start = find_start(log, track[0, 0], track[0, 1])
    if start is None:
        return None
    L = min(len(track), n_log - start)
    x, y, th, v = track[:L].T
    t = log["frame"][start:start + L]
    vx, vy, yaw = v * np.cos(th), v * np.sin(th), np.rad2deg(th)
    with np.errstate(all="ignore"):
        ax, ay = (np.zeros(1), np.zeros(1)) if L == 1 else (np.gradient(vx, t), np.gradient(vy, t))
    out = {k: np.array(c[:start + L], np.float64) for k, c in log.items()}
    for k, c in zip(EGO_COLUMNS, (x, y, vx, vy, ax, ay, yaw)):
        out[k][start:] = c
    return out, start, L


def _first(mask):
    i = np.nonzero(mask)[0]
    return int(i[0]) if len(i) else None


def window(log, scene):
    """filter_* (Metrics_Calculation.py:143-210): (i0, i1) with i1 = -1 for "to the end"; None
    where the reference raises (no start row)"""
    S = SCENARIOS[scene]
    ex, ey = log["ego_x"], log["ego_y"]
    with np.errstate(all="ignore"):
        if scene == 0:
            start = (ey > 0) & (log["sv2_vx"] != 0) & (log["sv2_vy"] != 0)
            end = ey >= S["end_y"]
        elif scene == 1:
            start = log["sv1_yaw"] < S["start_yaw"]
            end = ex < S["end_x"]
        elif scene == 2:
            start = (ey < S["start_y"]) & (ey != 0) & (log["sv1_vx"] != 0) & (log["sv1_vy"] != 0)
            end = ey < S["end_y"]
        else:
            dist = np.sqrt((ex - log["sv1_x"]) ** 2 + (ey - log["sv1_y"]) ** 2)
            ax = log["sv1_ax"]
            start = (dist <= S["dist"]) & (np.abs(ax) >= S["ax"])
            end = (np.abs(ax) < S["ax"]) & (log["sv1_yaw"] < S["end_yaw"]) & (ax != 0) & (log["sv1_x"] > S["end_x"])
    i0 = _first(start)
    if i0 is None:
        return None
    i1 = _first(end[i0:])
    return i0, (-1 if i1 is None else i0 + i1)


def pet_two_rays(px1, py1, vx1, vy1, yaw1, px2, py2, vx2, vy2, yaw2, parts=False):
    """_pet_two_rays (:19-63)"""
    sp1, sp2 = np.hypot(vx1, vy1), np.hypot(vx2, vy2)
    th1, th2 = np.deg2rad(yaw1), np.deg2rad(yaw2)
    V1x, V1y, V2x, V2y = sp1 * np.cos(th1), sp1 * np.sin(th1), sp2 * np.cos(th2), sp2 * np.sin(th2)
    dpx, dpy = px2 - px1, py2 - py1
    det = V1x * (-V2y) - (-V2x) * V1y
    with np.errstate(all="ignore"):
        t1 = (dpx * (-V2y) - dpy * (-V2x)) / det
        t2 = (V1x * dpy - V1y * dpx) / det
        pet = np.abs(t1 - t2)
        invalid = (np.abs(det) < EPS_DET) | (sp1 < EPS_V) | (sp2 < EPS_V) | (t1 < 0) | (t2 < 0) \
            | ~np.isfinite(t1) | ~np.isfinite(t2)
    pet = np.asarray(pet, dtype=float)
    pet[invalid] = np.nan
    return (pet, t1, t2, det) if parts else pet


def columns(log, scene, i0, i1, has_time=None):
    """TTC, PET, JERK of the window rows [i0, i1] (add_ttc_column, add_pet_column, add_jerk_column)"""
    S = SCENARIOS[scene]
    sl = slice(i0, None if i1 < 0 else i1 + 1)
    w = {k: c[sl] for k, c in log.items()}
    sv, axis = S["ttc"]
    with np.errstate(all="ignore"):
        denom = w["ego_v" + axis] - w[sv + "_v" + axis]
        num = w[sv + "_" + axis] - w["ego_" + axis]
        ttc = np.where(np.abs(denom) > EPS_V, num / denom, np.nan)
        o = S["pet"]
        pet = pet_two_rays(w["ego_x"], w["ego_y"], w["ego_vx"], w["ego_vy"], w["ego_yaw"],
                           w[o + "_x"], w[o + "_y"], w[o + "_vx"], w[o + "_vy"], w[o + "_yaw"])
        a = w[S["jerk"]]
        jerk = np.full(len(a), np.nan)
        if has_time is None:
            has_time = "sim_time" in log
        if has_time:
            dt = np.diff(w["sim_time"])
            jerk[1:] = np.where(np.abs(dt) > EPS_V, np.diff(a) / dt, np.nan)
        else:
            jerk[1:] = np.diff(a) / S["dt"]
    return w, ttc, pet, jerk


def sub_window(w, scene):
    """the scenario sub-window of main() (:412-456) as a mask over the window rows"""
    S = SCENARIOS[scene]
    n = len(w["ego_x"])
    with np.errstate(all="ignore"):
        if scene == 0:
            return (w["sv2_x"] >= S["sub"][0]) & (w["sv2_x"] <= S["sub"][1])
        if scene == 1:  # result.loc[:first - 1] on a RangeIndex: the rows before the first hit (none for first = 0)
            f = _first(w["ego_ax"] >= S["sub"])
            return np.arange(n) < (n if f is None else f)
        if scene == 2:
            return w["sv1_x"] <= S["sub"]
        x1, y1, x2, y2 = S["sub"]
        f = _first((w["sv1_x"] - x1) * (y2 - y1) - (w["sv1_y"] - y1) * (x2 - x1) > 0)
        return np.arange(n) >= (n if f is None else f)


def _stat(v, fn):
    v = v[~np.isnan(v)]
    return float(fn(v)) if len(v) else float("nan")


def record(log, scene, start=0, L=0, has_time=None, rows=False):
    """the per-track record (``RECORD_FIELDS``) of a (merged) log, and the window columns"""
    rec = dict.fromkeys(RECORD_FIELDS, float("nan"))
    rec.update(status=OK, start=start, L=L, i0=-1, i1=-1, n_window=0, n_sub=0, ttc_count=0, pet_count=0, jerk_count=0)
    win = window(log, scene)
    if win is None:
        rec["status"] = NO_WINDOW
        return (rec, None) if rows else rec
    i0, i1 = win
    w, ttc, pet, jerk = columns(log, scene, i0, i1, has_time)
    sub = sub_window(w, scene)
    with np.errstate(all="ignore"):
        vt = sub & (ttc > 0)
        vp = sub & np.isfinite(pet) & (pet >= 0)
        vj = sub & np.isfinite(jerk)
    col, how = SCENARIOS[scene]["decel"]
    rec.update(i0=i0, i1=i1, n_window=len(ttc), n_sub=int(sub.sum()),
               ttc_count=int(vt.sum()), pet_count=int(vp.sum()), jerk_count=int(vj.sum()))
    if vt.any():
        rec.update(ttc_mean=float(np.mean(ttc[vt])), ttc_min=float(np.min(ttc[vt])),
                   decel=_stat(w[col][vt], np.min if how == "min" else np.max), yaw_max=_stat(w["ego_yaw"][vt], np.max))
    if vp.any():
        rec.update(pet_mean=float(np.mean(pet[vp])), pet_min=float(np.min(pet[vp])))
    if vj.any():
        rec.update(jerk_mean=float(np.mean(np.abs(jerk[vj]))), jerk_max=float(np.max(np.abs(jerk[vj]))))
    if rows:
        cols = {"TTC": ttc, "PET": pet, "JERK": jerk}
        cols.update({k: w[k] for k in EGO_COLUMNS})
        return rec, cols
    return rec


def track_record(log, track, scene, rows=False):
    """merge + record; EMPTY / NO_START where the reference raises before the metrics"""
    track = np.asarray(track, np.float64).reshape(-1, 4)
    m = merge(log, track)
    if m is None:
        rec = dict.fromkeys(RECORD_FIELDS, float("nan"))
        empty = len(log["ego_x"]) == 0 or len(track) == 0
        rec.update(status=EMPTY if empty else NO_START, start=-1, L=0, i0=-1, i1=-1, n_window=0, n_sub=0,
                   ttc_count=0, pet_count=0, jerk_count=0)
        return (rec, None) if rows else rec
    merged, start, L = m
    return record(merged, scene, start, L, has_time="sim_time" in log, rows=rows)
