"""Safety metrics (TTC, PET, jerk) of tracked trajectories on the GPU: the reference's
``SUT_Testing/`` stage for a whole population.

Replaces, per track, ``Defensive_Testing.py`` (``find_best_start_row`` :156-163,
``compute_ego_kinematics`` :130-153, ``merge_trajectory_into_csv`` :166-205 — the write-back of a
tracked trajectory [x, y, theta, v] into the human log it started from) and
``tools/Metrics_Calculation.py`` (the four scenario filters :143-210, ``add_ttc_column`` :264-274,
``_pet_two_rays`` :19-63, ``add_jerk_column`` :300-328 and the sub-window statistics of ``main()``
:412-456) with one launch of ``csrc/cvae_safety.h`` (C-ABI ``cvae_safety_metrics``).  The merged
log is never materialised; only an 18-word record per track leaves the device, plus the per-row
columns when asked for.  DESIGN.md §4.10.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import CvaeError, CvaeSafetyConfig, check, lib

COLUMNS = ("frame", "sim_time", "ego_x", "ego_y", "ego_vx", "ego_vy", "ego_ax", "ego_ay", "ego_yaw",
           "sv1_x", "sv1_y", "sv1_vx", "sv1_vy", "sv1_ax", "sv1_yaw",
           "sv2_x", "sv2_y", "sv2_vx", "sv2_vy", "sv2_yaw")
EGO_COLUMNS = ("ego_x", "ego_y", "ego_vx", "ego_vy", "ego_ax", "ego_ay", "ego_yaw")
ROW_COLUMNS = ("TTC", "PET", "JERK") + EGO_COLUMNS
RECORD_FIELDS = ("status", "start", "L", "i0", "i1", "n_window", "n_sub",
                 "ttc_count", "ttc_mean", "ttc_min", "pet_count", "pet_mean", "pet_min",
                 "jerk_count", "jerk_mean", "jerk_max", "decel", "yaw_max")
_INT_FIELDS = ("status", "start", "L", "i0", "i1", "n_window", "n_sub", "ttc_count", "pet_count", "jerk_count")
OK, NO_WINDOW, EMPTY, NO_START = 0, 1, 2, 3
EPS_V, EPS_DET = 1e-9, 1e-12  # Metrics_Calculation.py:15-16

# The scenario table (Metrics_Calculation.py), one entry per cvae_scene id.  csrc/cvae_safety.h
# mirrors it (its SF_* constants; tests/test_safety_oracle.py compares the two) and the numpy
# oracle of the tests reads it from here.  These are NOT the extractor's predicates
# (cvae_amd.preprocess): Static here also needs both sv2 velocities non-zero and ends at
# ego_y >= 80 inclusive, and so on.
SCENARIOS = (
    {"name": "StaticBlindTown05", "key": "sce1", "dt": 0.02, "ttc": ("sv2", "y"), "pet": "sv2", "jerk": "ego_ay",
     "end_y": 80.0, "sub": (-196.81, -193.31), "decel": ("ego_ay", "min")},
    {"name": "DynamicBlindTown05", "key": "sce2", "dt": 0.025, "ttc": ("sv2", "x"), "pet": "sv2", "jerk": "ego_ax",
     "start_yaw": -150.0, "end_x": -186.8897, "sub": 100.0, "decel": ("ego_ax", "max")},
    {"name": "PredictableMovementTown05", "key": "sce3", "dt": 0.015, "ttc": ("sv1", "y"), "pet": "sv1",
     "jerk": "ego_ay", "start_y": 40.0, "end_y": -78.0, "sub": 156.76, "decel": ("ego_ay", "max")},
    {"name": "UnpredictableMovementTown04", "key": "sce4", "dt": 0.02, "ttc": ("sv1", "y"), "pet": "sv1",
     "jerk": "ego_ay", "dist": 30.0, "ax": 0.1, "end_yaw": -90.0, "end_x": 15.0,
     "sub": (13.06, -160.0, 14.77, 220.0), "decel": ("ego_ay", "max")},
)


def scene_id(scene) -> int:
    """cvae_scene id of 'sce1'..'sce4', a scenario name (or a string containing either), or an id."""
    if isinstance(scene, (int, np.integer)):
        if 0 <= int(scene) < len(SCENARIOS):
            return int(scene)
        raise ValueError(f"unknown scene {scene!r}")
    for i, s in enumerate(SCENARIOS):
        if s["name"] in str(scene) or s["key"] in str(scene):
            return i
    raise ValueError(f"unknown scene {scene!r}")


def read_columns(csv_path):
    """The columns of ``COLUMNS`` a log has, as a DataFrame (``pd.read_csv`` with ``usecols``, the
    reference's parser on fewer columns)."""
    import pandas as pd
    return pd.read_csv(csv_path, usecols=lambda c: c in COLUMNS)


def pack_logs(frames):
    """(cols [20, n_rows] float64, offsets int64 [n+1], flags int32 [n]) of DataFrames / column
    dicts: a missing column is NaN; flag bit 0 = ``sim_time`` exists, bit 1 = the log has a row with
    finite ego_x and ego_y."""
    arrs, flags = [], []
    for f in frames:
        n = len(f[next(iter(f.keys()))]) if len(f.keys()) else 0
        a = np.full((len(COLUMNS), n), np.nan)
        for k, name in enumerate(COLUMNS):
            if name in f:
                a[k] = np.asarray(f[name], dtype=np.float64)
        arrs.append(a)
        fin = np.isfinite(a[2]) & np.isfinite(a[3])
        flags.append((1 if "sim_time" in f else 0) | (2 if fin.any() else 0))
    off = np.zeros(len(arrs) + 1, np.int64)
    off[1:] = np.cumsum([a.shape[1] for a in arrs])
    cols = np.ascontiguousarray(np.concatenate(arrs, axis=1)) if arrs else np.zeros((len(COLUMNS), 0))
    return cols, off, np.asarray(flags, np.int32).reshape(-1)


def _torch():
    import torch
    return torch


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _hp(a):
    return a.ctypes.data_as(C.c_void_p)


class SceneLogs:
    """The logs of one scene on the device, uploaded once.  ``frames_or_csv_paths``: DataFrames (or
    dicts of columns) and / or CSV paths; ``scene``: 'sce1'..'sce4', a scenario name or a
    ``cvae_scene`` id."""

    def __init__(self, frames_or_csv_paths, scene, device="cuda"):
        torch = _torch()
        self.scene = scene_id(scene)
        frames = [read_columns(f) if isinstance(f, (str, bytes)) or hasattr(f, "__fspath__") else f
                  for f in frames_or_csv_paths]
        self.cols_host, self.offsets_host, self.flags_host = pack_logs(frames)
        self.device = torch.device(device)
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)  # noqa: E731
        self.cols, self.offsets, self.flags = to(self.cols_host), to(self.offsets_host), to(self.flags_host)

    def __len__(self):
        return len(self.offsets_host) - 1

    @property
    def n_rows(self):
        return int(self.offsets_host[-1])

    def rows_of(self, f):
        return int(self.offsets_host[f + 1] - self.offsets_host[f])


def _tracks(tracks, dev):
    """(states device tensor or None, offsets device tensor, offsets host) of DeviceTracks, a
    (states, offsets) pair or a list of [n, 4] arrays — as ``validate.metrics`` takes them."""
    torch = _torch()
    if hasattr(tracks, "states") and hasattr(tracks, "offsets_host"):  # mpc.DeviceTracks
        return tracks.states, tracks.offsets, np.ascontiguousarray(tracks.offsets_host, dtype=np.int64)
    if isinstance(tracks, tuple) and len(tracks) == 2 and hasattr(tracks[0], "data_ptr"):
        states, off = tracks
        off_h = off.cpu().numpy() if hasattr(off, "cpu") else np.asarray(off)
        off_h = np.ascontiguousarray(off_h, dtype=np.int64)
        d_off = off if hasattr(off, "cpu") else torch.from_numpy(off_h).to(states.device)
        return states, d_off, off_h
    trajs = [np.asarray(t, dtype=np.float64).reshape(-1, 4) for t in tracks]
    off = np.zeros(len(trajs) + 1, np.int64)
    off[1:] = np.cumsum([len(t) for t in trajs])
    flat = np.ascontiguousarray(np.concatenate(trajs)) if trajs else np.zeros((0, 4))
    return torch.from_numpy(flat).to(dev), torch.from_numpy(off).to(dev), off


def _records(rec):
    out = {k: rec[:, i].copy() for i, k in enumerate(RECORD_FIELDS)}
    for k in _INT_FIELDS:
        out[k] = out[k].astype(np.int64)
    return out


def _run(logs, tracks, log_of_track, want_rows, merge, block_waves):
    torch = _torch()
    dev = logs.device
    lot = np.ascontiguousarray(np.asarray(log_of_track, dtype=np.int32).reshape(-1))
    P = len(lot)
    states = d_off = None
    off_h = np.zeros(P + 1, np.int64)
    if merge:
        states, d_off, off_h = _tracks(tracks, dev)
        if len(off_h) - 1 != P:
            raise CvaeError(f"log_of_track has {P} entries for {len(off_h) - 1} tracks")
        if states.dtype != torch.float64 or not states.is_contiguous():
            raise CvaeError("track states must be a contiguous float64 [rows, 4] tensor")
    cfg = CvaeSafetyConfig()
    cfg.scene, cfg.want_rows, cfg.block_waves, cfg.merge = logs.scene, int(want_rows), int(block_waves), int(merge)
    n_logs = len(logs)
    ok = (lot >= 0) & (lot < n_logs)
    row_off = np.zeros(P + 1, np.int64)
    if want_rows and ok.all():
        row_off[1:] = np.cumsum(logs.offsets_host[lot + 1] - logs.offsets_host[lot])
    n_out = int(row_off[-1])
    d_lot = torch.from_numpy(lot).to(dev)
    d_rec = torch.empty((P, len(RECORD_FIELDS)), dtype=torch.float64, device=dev)
    d_rows = d_ro = None
    if want_rows:
        d_rows = torch.full((len(ROW_COLUMNS), max(n_out, 1)), float("nan"), dtype=torch.float64, device=dev)
        d_ro = torch.from_numpy(row_off).to(dev)
    check(lib().cvae_safety_metrics(
        C.byref(cfg), _p(logs.cols), logs.n_rows, _p(logs.offsets), _hp(logs.offsets_host), n_logs, _p(logs.flags),
        _hp(logs.flags_host), _p(states), 0 if states is None else int(states.shape[0]), _p(d_off), _hp(off_h), P,
        _p(d_lot), _hp(lot), _p(d_rec), _p(d_rows), _p(d_ro), max(n_out, 1) if want_rows else 0,
        C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "cvae_safety_metrics")
    out = _records(d_rec.cpu().numpy().reshape(P, len(RECORD_FIELDS)))
    if want_rows:
        out["row_offsets"] = row_off
        out["rows_device"] = d_rows
    return out


def _window_rows(out, names):
    """ragged host columns of the window rows [i0, i0 + n_window) per track"""
    rows = out.pop("rows_device").cpu().numpy()
    ro = out["row_offsets"]
    lo = ro[:-1] + np.maximum(out["i0"], 0)
    n = np.where(out["status"] == OK, out["n_window"], 0)
    for k, name in enumerate(ROW_COLUMNS):
        if name in names:
            out[name] = [rows[k, a:a + m].copy() for a, m in zip(lo, n)]
    return out


def track_safety(tracks, logs: SceneLogs, log_of_track, rows=False, block_waves=0):
    """Merge every track into its log and score it.  ``tracks``: the ``DeviceTracks`` of
    ``mpc.track_batch_device`` (nothing but the records leaves the device), a (states, offsets)
    pair of device tensors, or a list of [n, 4] (x, y, theta, v) arrays; ``log_of_track``: the
    index in ``logs`` of each track's log.  Returns a dict of numpy arrays, one per
    ``RECORD_FIELDS`` entry; ``rows=True`` adds ``TTC`` / ``PET`` / ``JERK`` and the seven merged
    ego columns as lists of per-track arrays over the scenario window.  Where the reference raises
    (no start row: status ``NO_WINDOW``; an empty track: ``EMPTY``) the metrics are NaN."""
    out = _run(logs, tracks, log_of_track, 3 if rows else 0, True, block_waves)
    return _window_rows(out, ROW_COLUMNS) if rows else out


def log_safety(logs: SceneLogs, rows=False, block_waves=0):
    """The same metrics of the logs as recorded, no track merged (``compute_metric_from_csv`` +
    ``main()`` for a system under test): one record per log."""
    out = _run(logs, None, np.arange(len(logs), dtype=np.int32), 3 if rows else 0, False, block_waves)
    return _window_rows(out, ROW_COLUMNS) if rows else out


def merge_tracks(tracks, logs: SceneLogs, log_of_track, block_waves=0):
    """The batch form of ``merge_trajectory_into_csv``: per track a dict with ``start``, ``L`` and
    the seven merged ego columns (length start + L; the log's own values before ``start``), for
    users who still want the ``*_def.csv`` files.  ``None`` for a track without a merge (EMPTY)."""
    out = _run(logs, tracks, log_of_track, 2, True, block_waves)
    rows = out.pop("rows_device").cpu().numpy()
    ro, res = out["row_offsets"], []
    for p in range(len(ro) - 1):
        if out["start"][p] < 0:
            res.append(None)
            continue
        m = int(out["start"][p] + out["L"][p])
        d = {"start": int(out["start"][p]), "L": int(out["L"][p])}
        for k, name in enumerate(EGO_COLUMNS):
            d[name] = rows[3 + k, ro[p]:ro[p] + m].copy()
        res.append(d)
    return res


def summary(records):
    """The population view: the share of tracks with a scenario window, and min / 5th percentile /
    median of the per-track min-TTC and min-PET over the tracks that have one."""
    st = np.asarray(records["status"])
    out = {"n_tracks": int(len(st)), "window_share": float(np.mean(st == OK)) if len(st) else float("nan")}
    for k in ("ttc_min", "pet_min"):
        v = np.asarray(records[k], dtype=np.float64)
        v = v[np.isfinite(v)]
        out[k + "_count"] = int(len(v))
        for name, q in (("min", 0.0), ("p05", 5.0), ("median", 50.0)):
            out[f"{k}_{name}"] = float(np.percentile(v, q)) if len(v) else float("nan")
    return out


def checkpoint_safety(model_path, start_states, logs: SceneLogs, log_of_track, seq_len=10, dim=3, latent_dim=8,
                      z=None, rows=False, timings=None):
    """Generate, track and score a checkpoint without the states leaving the device: the safety
    counterpart of ``validate.validate_checkpoint`` (same generation and tracking: N=30, control
    horizon 20, the scene's dt, total time = the last waypoint's), then ``track_safety``.
    ``start_states``: [P, 5] (x, y, theta, vx, vy); ``timings``: a dict that receives seconds per
    stage."""
    from .validate import _generate_and_track
    tracks, lap, t0 = _generate_and_track(model_path, start_states, logs.device, SCENARIOS[logs.scene]["dt"], seq_len,
                                          dim, latent_dim, z, timings)
    out = track_safety(tracks, logs, log_of_track, rows=rows)
    lap("safety", t0)
    return out
