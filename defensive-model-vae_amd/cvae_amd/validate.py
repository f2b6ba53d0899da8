"""Model-vs-human validation on the GPU: the last stage of the reference pipeline.

Replaces the per-point Python loops of ``Distribution.py`` / ``Spatial_Distribution.py`` — velocity
Jensen-Shannon divergence (M1, ``Distribution.py:195-331``), ``RMSE_frequency`` by points (M2,
``Spatial_Distribution.py:18-161``) and by trajectories (M3, ``:387-492``), the space-time-velocity
surface RMSE (M4, ``:708-931, :1540-1583``) and the spatiotemporal plane RMSE (M5, ``:1357-1429``)
— with the HIP kernels of ``csrc/cvae_metrics.h`` (C-ABI ``cvae_val_ranges / cvae_val_accumulate``).

Two launches per population: a ranges pass (min/max, exact), then — after the HOST has built every
bin edge with numpy exactly as the reference does — one accumulate pass that binary-searches those
edges and fills small integer tables.  Only the tables leave the device; the final scalars
(JS, RMSEs, the 40x40 Gaussian smoothing) are float64 numpy on them.  DESIGN.md §4.9.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import CvaeError, CvaeValConfig, CvaeValTables, check, lib

N_VEDGES, N_SURF, SUBSAMPLE = 50, 40, 150
FIX = 2.0 ** -24  # quantum of the fixed-point sums
SCENE_DT = (("sce1", 0.02), ("sce2", 0.025), ("sce3", 0.015))  # Spatial_Distribution.py:686-705


def scene_dt(scene: str) -> float:
    for k, v in SCENE_DT:
        if k in scene:
            return v
    return 0.02


def grid_edges(scene: str, grid_size: float = 0.5):
    """``_get_grid_edges`` (Spatial_Distribution.py:360-384)."""
    if "sce1" in scene:
        return np.arange(-198, -188 + 1, grid_size), np.arange(40, 80 + 1, grid_size)
    if "sce2" in scene:
        return np.arange(-200, -120, grid_size), np.arange(-8, 6, grid_size)
    if "sce3" in scene:
        return np.arange(148, 158, grid_size), np.arange(-80, 22, grid_size)
    return np.arange(0, 20, grid_size), np.arange(-20, 100, grid_size)


# ---- human velocities (sequential: host, once per HumanReference) -------------------------------
def human_velocities_global(human_trajectories):
    """``calculate_human_velocities`` (Distribution.py:248-296), operation for operation: a step with
    dt <= 1e-6 repeats the last value of the whole list (across trajectory boundaries)."""
    vel = []
    for traj in human_trajectories:
        t, x, y = traj[:, 2], traj[:, 0], traj[:, 1]
        n = len(traj)
        for i in list(range(n - 1)) + ([n - 2] if n > 1 else []):  # the last point repeats the last step
            dt = t[i + 1] - t[i]
            if dt > 1e-6:
                dx, dy = x[i + 1] - x[i], y[i + 1] - y[i]
                vel.append(np.sqrt(dx ** 2 + dy ** 2) / dt)
            else:
                vel.append(vel[-1] if vel else 0.0)
    return np.array(vel, dtype=np.float64)


def human_velocities_per_track(human_trajectories):
    """``_prepare_human_stv_data`` (Spatial_Distribution.py:765-795): per trajectory with >= 2 rows,
    the carry restarting in each; the last point repeats the value before it."""
    out = []
    for traj in human_trajectories:
        if traj.shape[0] < 2:
            continue
        t, x, y = traj[:, 2], traj[:, 0], traj[:, 1]
        vel = []
        for i in range(len(traj) - 1):
            dt = t[i + 1] - t[i]
            if dt > 1e-6:
                dx, dy = x[i + 1] - x[i], y[i + 1] - y[i]
                vel.append(np.sqrt(dx ** 2 + dy ** 2) / dt)
            else:
                vel.append(vel[-1] if vel else 0.0)
        vel.append(vel[-1] if vel else 0.0)
        out.append(np.array(vel, dtype=np.float64))
    return out


# ---- host finalisation from the tables -----------------------------------------------------------
def js_from_counts(hist_model, hist_human) -> float:
    """Distribution.py:319-331 with scipy ``entropy``'s renormalisation of both arguments, base 2."""
    p = hist_model / (hist_model.sum() + 1e-10)
    q = hist_human / (hist_human.sum() + 1e-10)
    m = 0.5 * (p + q)

    def entropy(pk, qk):
        pk, qk = pk / np.sum(pk), qk / np.sum(qk)
        return float(np.sum(pk * np.log(pk / qk)) / np.log(2))

    return 0.5 * (entropy(p + 1e-10, m + 1e-10) + entropy(q + 1e-10, m + 1e-10))


def rmse_frequency(H_model, H_human) -> float:
    """Spatial_Distribution.py:136-156 / :468-487: over the cells where either count is positive."""
    a, b = np.asarray(H_model, np.float64).ravel(), np.asarray(H_human, np.float64).ravel()
    mask = (a > 0) | (b > 0)
    if not mask.any():
        return 0.0
    return float(np.sqrt(np.mean((a[mask] - b[mask]) ** 2)))


def gaussian_filter_nearest(a, sigma=2.0, truncate=4.0):
    """``scipy.ndimage.gaussian_filter(a, sigma, mode='nearest')`` restated in numpy: radius
    int(truncate * sigma + 0.5), normalised weights, separable, axis 0 then axis 1."""
    a = np.asarray(a, np.float64)
    r = int(truncate * float(sigma) + 0.5)
    x = np.arange(-r, r + 1)
    w = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    w = w / w.sum()
    for axis in range(a.ndim):
        b = np.moveaxis(np.pad(np.moveaxis(a, axis, 0), [(r, r)] + [(0, 0)] * (a.ndim - 1), mode="edge"), 0, 0)
        n = a.shape[axis]
        acc = np.zeros_like(np.moveaxis(a, axis, 0))
        for j in range(2 * r + 1):
            acc += w[j] * b[j:j + n]
        a = np.moveaxis(acc, 0, axis)
    return a


def surface_rmse(surf_model, surf_human):
    """``calculate_surface_rmse`` (:1540-1583) for both masks: (rmse over all cells, rmse over the
    cells where either surface is non-zero, the number of those cells)."""
    d = surf_model - surf_human
    nz = (surf_model != 0.0) | (surf_human != 0.0)
    r_nz = float(np.sqrt(np.mean(d[nz] ** 2))) if nz.any() else 0.0
    return float(np.sqrt(np.mean(d ** 2))), r_nz, int(nz.sum())


def plane_rmse(cnt_m, sx_m, sy_m, cnt_h, sx_h, sy_h):
    """``compute_spatiotemporal_plane_rmse`` (:1408-1429) from the per-slice sums."""
    both = (cnt_m > 0) & (cnt_h > 0)
    if not both.any():
        return float("nan"), []
    dx = sx_m[both] / cnt_m[both] - sx_h[both] / cnt_h[both]
    dy = sy_m[both] / cnt_m[both] - sy_h[both] / cnt_h[both]
    err = np.sqrt(dx ** 2 + dy ** 2)
    return float(np.sqrt(np.mean(err ** 2))), err.tolist()


def surface_from_tables(cnt, total):
    """v_surface (:916-925): the mean where the count is positive, 0 elsewhere, then smoothed."""
    mean = np.where(cnt > 0, total / np.maximum(cnt, 1), 0.0)
    return gaussian_filter_nearest(mean, 2.0)


# ---- device side ---------------------------------------------------------------------------------
def _torch():
    import torch
    return torch


def _unkey(k):
    k = np.asarray(k, np.uint64)
    neg = (k >> np.uint64(63)) == 0
    bits = np.where(neg, ~k, k & np.uint64(0x7FFFFFFFFFFFFFFF))
    return bits.astype(np.uint64).view(np.float64)


class _Population:
    """A ragged population on the device plus its ranges (one tiny D2H copy)."""

    def __init__(self, rows, offsets, offsets_host, stride, dt, v_hist=None, v_surf=None, surf_min_rows=0,
                 block_waves=0):
        torch = _torch()
        self.rows, self.offsets, self.stride, self.dt = rows, offsets, stride, float(dt)
        self.offsets_host = np.ascontiguousarray(offsets_host, dtype=np.int64)
        self.P = len(self.offsets_host) - 1
        self.n_rows = int(rows.shape[0])
        self.v_hist, self.v_surf, self.surf_min_rows, self.block_waves = v_hist, v_surf, surf_min_rows, block_waves
        self.dev = rows.device
        d_out = torch.empty(16, dtype=torch.int64, device=self.dev)
        c = self.config()
        check(lib().cvae_val_ranges(C.byref(c), self.P, self._p(rows), self.n_rows, self._p(offsets),
                                    self.offsets_host.ctypes.data_as(C.c_void_p), self._p(v_hist), self._p(d_out),
                                    self._stream()), "cvae_val_ranges")
        self.ranges_raw = np.ascontiguousarray(d_out.cpu().numpy().view(np.uint64))
        r = _unkey(self.ranges_raw[:14])
        self.count, self.longest = int(self.ranges_raw[14]), int(self.ranges_raw[15])
        names = ("v", "x", "y", "t", "sx", "sy", "st")
        # (min, max) per quantity, None where no point contributed
        self.range = {n: ((float(r[2 * i]), float(r[2 * i + 1]))
                          if self.ranges_raw[2 * i] <= self.ranges_raw[2 * i + 1] else None)
                      for i, n in enumerate(names)}

    @staticmethod
    def _p(t):
        return None if t is None else C.c_void_p(t.data_ptr())

    def _stream(self):
        return C.c_void_p(_torch().cuda.current_stream(self.dev).cuda_stream)

    def config(self, axis="x", n_v=0, n_x=0, n_y=0, n_c=0, n_t=0, n_s=0):
        c = CvaeValConfig()
        c.dt, c.stride, c.x_col, c.y_col = self.dt, self.stride, 0, 1
        c.t_col = 2 if self.stride == 3 else -1
        c.v_col = 3 if self.stride == 4 else -1
        c.coord_col = 0 if axis == "x" else 1
        c.subsample, c.surf_min_rows = SUBSAMPLE, self.surf_min_rows
        c.n_v_edges, c.n_x_edges, c.n_y_edges = n_v, n_x, n_y
        c.n_coord_edges, c.n_time_edges, c.n_slice_edges, c.block_waves = n_c, n_t, n_s, self.block_waves
        return c

    def accumulate(self, axis, ve, xe, ye, ce, te, se):
        """One launch: every table whose edge array is non-empty.  Returns host numpy tables."""
        torch = _torch()
        arrs = [np.ascontiguousarray(e, dtype=np.float64) for e in (ve, xe, ye, ce, te, se)]
        n_v, n_x, n_y, n_c, n_t, n_s = (len(a) for a in arrs)
        if n_s < 2:
            n_s, arrs[5] = 0, np.zeros(0)
        c = self.config(axis, n_v, n_x, n_y, n_c, n_t, n_s)
        nb, cells, surf, ns = max(n_v - 1, 0), max(n_x - 1, 0) * max(n_y - 1, 0), max(n_c - 1, 0) * max(n_t - 1, 0), \
            max(n_s - 1, 0)
        # one buffer: the three int64 tables first (8-byte aligned), then the uint32 ones
        n64, n32 = surf + 2 * ns, nb + 2 * cells + surf + ns
        buf = torch.zeros(2 * n64 + n32 + 2, dtype=torch.int32, device=self.dev)
        base = buf.data_ptr()
        o64 = np.cumsum([0, surf, ns, ns]) * 8
        o32 = 8 * n64 + np.cumsum([0, nb, cells, cells, surf, ns]) * 4
        t = CvaeValTables()
        t.surf_sum, t.slice_sx, t.slice_sy = (base + int(o) for o in o64[:3])
        t.hist_v, t.h_points, t.h_traj, t.surf_cnt, t.slice_cnt = (base + int(o) for o in o32[:5])
        edges = np.concatenate(arrs) if sum(len(a) for a in arrs) else np.zeros(1)
        d_edges = torch.from_numpy(edges).to(self.dev)
        check(lib().cvae_val_accumulate(C.byref(c), self.P, self._p(self.rows), self.n_rows, self._p(self.offsets),
                                        self.offsets_host.ctypes.data_as(C.c_void_p), self._p(self.v_hist),
                                        self._p(self.v_surf), self._p(d_edges),
                                        self.ranges_raw.ctypes.data_as(C.c_void_p), C.byref(t), self._stream()),
              "cvae_val_accumulate")
        h = buf.cpu().numpy()
        i64 = h[:2 * n64].view(np.int64)
        u32 = h[2 * n64:2 * n64 + n32].view(np.uint32).astype(np.int64)
        q = np.cumsum([0, nb, cells, cells, surf, ns])
        gs, ss = (max(n_y - 1, 0), max(n_x - 1, 0)), (max(n_t - 1, 0), max(n_c - 1, 0))
        return {"hist_v": u32[q[0]:q[1]], "H_points": u32[q[1]:q[2]].reshape(gs), "H_traj": u32[q[2]:q[3]].reshape(gs),
                "surf_cnt": u32[q[3]:q[4]].reshape(ss), "surf_sum": i64[:surf].reshape(ss).copy(),
                "slice_cnt": u32[q[4]:q[5]], "slice_sx": i64[surf:surf + ns].copy(),
                "slice_sy": i64[surf + ns:surf + 2 * ns].copy()}


def _ragged(trajs, width):
    trajs = [np.asarray(t, dtype=np.float64).reshape(-1, width) for t in trajs]
    off = np.zeros(len(trajs) + 1, np.int64)
    off[1:] = np.cumsum([len(t) for t in trajs])
    flat = np.ascontiguousarray(np.concatenate(trajs)) if trajs else np.zeros((0, width))
    return trajs, flat, off


def _check_values(*arrays):
    for a in arrays:
        if a.size and not np.all(np.abs(a[~np.isnan(a)]) < 1024.0):
            raise CvaeError("values must be finite and |value| < 1024")


class HumanReference:
    """The human side of every metric: ``human_trajectories`` is the list of [n, 3] (x, y, t) arrays
    ``Distribution.load_human_trajectories`` returns.  Velocities are computed once on the host
    (both of the reference's rules), everything is uploaded once, and the human tables are cached
    per set of edges, so one instance serves many checkpoints."""

    def __init__(self, human_trajectories, scene, grid_size=0.5, device="cuda", block_waves=0):
        torch = _torch()
        self.scene, self.grid_size, self.dt = scene, float(grid_size), scene_dt(scene)
        self.device = torch.device(device)
        self.block_waves = block_waves
        self.x_edges, self.y_edges = grid_edges(scene, grid_size)
        trajs, flat, off = _ragged(human_trajectories, 3)
        self.v_global = human_velocities_global(trajs)
        self.v_per_track = human_velocities_per_track(trajs)
        # per-row velocity arrays: NaN = no value (one-point trajectories have none, Distribution.py:267-282)
        vh, vs = np.full(len(flat), np.nan), np.zeros(len(flat))
        g = k = 0
        for p, t in enumerate(trajs):
            n = len(t)
            if n > 1:
                vh[off[p]:off[p + 1]] = self.v_global[g:g + n]
                vs[off[p]:off[p + 1]] = self.v_per_track[k]
                g, k = g + n, k + 1
        _check_values(flat[:, :2], vh, vs)
        self.n_traj, self.n_points = len(trajs), len(flat)
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)  # noqa: E731
        self.pop = _Population(to(flat), to(off), off, 3, self.dt, to(vh), to(vs), surf_min_rows=2,
                               block_waves=block_waves)
        self._cache = {}

    def tables(self, axis, ve, ce, te, se):
        key = (axis,) + tuple(np.ascontiguousarray(e, dtype=np.float64).tobytes() for e in (ve, ce, te, se))
        if key not in self._cache:
            if len(self._cache) > 64:
                self._cache.clear()
            self._cache[key] = self.pop.accumulate(axis, ve, self.x_edges, self.y_edges, ce, te, se)
        return self._cache[key]


def _model_population(tracks, ref):
    torch = _torch()
    if hasattr(tracks, "states") and hasattr(tracks, "offsets_host"):  # mpc.DeviceTracks
        return _Population(tracks.states, tracks.offsets, tracks.offsets_host, 4, ref.dt, block_waves=ref.block_waves)
    if isinstance(tracks, tuple) and len(tracks) == 2:  # (states [rows, 4] device tensor, offsets)
        states, off = tracks
        off_h = off.cpu().numpy() if hasattr(off, "cpu") else np.asarray(off, np.int64)
        d_off = off if hasattr(off, "cpu") else torch.from_numpy(np.ascontiguousarray(off_h)).to(states.device)
        return _Population(states, d_off, off_h, 4, ref.dt, block_waves=ref.block_waves)
    _, flat, off = _ragged(tracks, 4)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(ref.device)  # noqa: E731
    return _Population(to(flat), to(off), off, 4, ref.dt, block_waves=ref.block_waves)


def _span(a, b):
    """(min, max) over the ranges that exist, or None"""
    r = [x for x in (a, b) if x is not None]
    return (min(x[0] for x in r), max(x[1] for x in r)) if r else None


def metrics(tracks, ref: HumanReference, axis="x", time_interval=5.0):
    """M1..M5 of the model tracks against ``ref``.  ``tracks``: the ``DeviceTracks`` of
    ``mpc.track_batch_device`` (nothing but the tables leaves the device), or a list of [n, 4]
    (x, y, theta, v) arrays.  Where the reference's own functions would raise — a population
    without points — the metric is NaN and its tables are zero."""
    if axis not in ("x", "y"):
        raise ValueError("axis must be 'x' or 'y'")
    m, h = _model_population(tracks, ref), ref.pop
    none = np.zeros(0)
    have = m.count > 0 and h.count > 0
    # M1 edges: Distribution.py:310-312
    ve = none
    if have and m.range["v"] is not None and h.range["v"] is not None:
        ve = np.linspace(min(m.range["v"][0], h.range["v"][0]), max(m.range["v"][1], h.range["v"][1]), N_VEDGES)
    # M4 edges: unified ranges (:800-832), np.linspace(.., 41) (:900-901)
    ce = te = none
    sk = "sx" if axis == "x" else "sy"
    if m.range[sk] is not None and h.range[sk] is not None:
        cr, tr = _span(m.range[sk], h.range[sk]), _span(m.range["st"], h.range["st"])
        ce, te = np.linspace(cr[0], cr[1], N_SURF + 1), np.linspace(tr[0], tr[1], N_SURF + 1)
    # M5 edges (:1401-1403)
    se = none
    if have:
        tr = _span(m.range["t"], h.range["t"])
        se = np.arange(tr[0], tr[1] + 1e-9, time_interval)
        if len(se) - 1 > 4096:
            raise CvaeError("cvae_val_accumulate failed: at most 4096 time slices")
        if len(se) < 2:
            se = none
    tm = m.accumulate(axis, ve, ref.x_edges, ref.y_edges, ce, te, se)
    th = ref.tables(axis, ve, ce, te, se)

    out = {"v_edges": ve, "x_edges": ref.x_edges, "y_edges": ref.y_edges, "coord_edges": ce, "time_edges": te,
           "slice_edges": se}
    zeros_v = np.zeros(N_VEDGES - 1, np.int64)
    out["hist_v_model"] = tm["hist_v"] if len(ve) else zeros_v
    out["hist_v_human"] = th["hist_v"] if len(ve) else zeros_v
    out["js_velocity"] = js_from_counts(out["hist_v_model"], out["hist_v_human"]) if len(ve) else float("nan")
    for k in ("H_points", "H_traj"):
        out[k + "_model"], out[k + "_human"] = tm[k], th[k]
    out["rmse_frequency_points"] = rmse_frequency(tm["H_points"], th["H_points"])
    out["rmse_frequency_trajectories"] = rmse_frequency(tm["H_traj"], th["H_traj"])
    if len(ce):
        sm = surface_from_tables(tm["surf_cnt"], tm["surf_sum"] * FIX)
        sh = surface_from_tables(th["surf_cnt"], th["surf_sum"] * FIX)
        out["surf_cnt_model"], out["surf_cnt_human"] = tm["surf_cnt"], th["surf_cnt"]
        r_all, r_nz, n_nz = surface_rmse(sm, sh)
    else:
        sm = sh = np.zeros((N_SURF, N_SURF))
        out["surf_cnt_model"] = out["surf_cnt_human"] = np.zeros((N_SURF, N_SURF), np.int64)
        r_all, r_nz, n_nz = float("nan"), float("nan"), 0
    out.update(surface_model=sm, surface_human=sh, surface_rmse=r_all, surface_rmse_nonzero=r_nz,
               surface_points_nonzero=n_nz)
    if len(se):
        out["plane_rmse"], out["plane_slice_errors"] = plane_rmse(
            tm["slice_cnt"], tm["slice_sx"] * FIX, tm["slice_sy"] * FIX,
            th["slice_cnt"], th["slice_sx"] * FIX, th["slice_sy"] * FIX)
    else:
        out["plane_rmse"], out["plane_slice_errors"] = float("nan"), []
    out["slice_cnt_model"], out["slice_cnt_human"] = tm["slice_cnt"], th["slice_cnt"]
    out["slice_sum_model"] = np.stack([tm["slice_sx"], tm["slice_sy"]])
    out["surf_sum_model"] = tm["surf_sum"]
    return out


def _generate_and_track(model_path, start_states, device, dt, seq_len, dim, latent_dim, z, timings):
    """The stages ``validate_checkpoint`` and ``safety.checkpoint_safety`` share: ``generate_trajectories``
    from each start position, then every generated path tracked as ``Distribution.py:83-105`` does
    (N=30, control horizon 20, the scene's dt, total time = the last waypoint's).  Returns the
    ``DeviceTracks`` and ``lap(name, t0)``, which records a stage's seconds in ``timings``."""
    import time

    from . import mpc
    from .tools import generate_trajectories
    torch = _torch()
    start = np.asarray(start_states, dtype=np.float64).reshape(-1, 5)

    def lap(name, t0):
        if timings is not None:
            torch.cuda.synchronize(device)
            timings[name] = time.perf_counter() - t0
        return time.perf_counter()

    t0 = time.perf_counter()
    wps = generate_trajectories(model_path, start[:, :2], seq_len, dim, latent_dim, z=z, device=device)
    wps = [np.asarray(w, np.float64)[:, [1, 2, 0]].copy() for w in wps]  # [t, x, y] -> [x, y, t] (:77-78)
    for w in wps:
        w[0, 2] = 0.0
    t0 = lap("generate", t0)
    tracks = mpc.track_batch_device(wps, start, device=device, prediction_horizon=30, control_horizon=20, dt=dt)
    return tracks, lap, lap("track", t0)


def validate_checkpoint(model_path, start_states, ref: HumanReference, seq_len=10, dim=3, latent_dim=8, axis="x",
                        time_interval=5.0, z=None, timings=None):
    """Generate, track and score a checkpoint without the states leaving the device.

    ``start_states``: [P, 5] (x, y, theta, vx, vy), the start rows ``get_start_conditions_from_csv``
    reads.  Runs ``generate_trajectories`` from each start position, tracks every generated path
    as ``Distribution.py:83-105`` does (N=30, control horizon 20, the scene's dt, total time = the
    last waypoint's), then ``metrics``.  ``timings``: a dict that receives seconds per stage."""
    tracks, lap, t0 = _generate_and_track(model_path, start_states, ref.device, ref.dt, seq_len, dim, latent_dim, z,
                                          timings)
    out = metrics(tracks, ref, axis=axis, time_interval=time_interval)
    lap("metrics", t0)
    return out
