"""A numpy restatement of the model-vs-human validation metrics (M1..M5 of DESIGN §4.9), written
from the definitions and used as the checker where the reference cannot run: whole-array numpy,
no per-point Python loops, no scipy.

    metrics(model, human, scene, grid_size, axis, time_interval) -> dict

``model``: list of [n, 4] (x, y, theta, v); ``human``: list of [n, 3] (x, y, t).  The dict has the
keys of ``cvae_amd.validate.metrics``.  Where the reference's own functions would raise (a
population without points) the metric is NaN and its tables are zero.
"""
import numpy as np

SCENE_DT = {"sce1": 0.02, "sce2": 0.025, "sce3": 0.015}
N_VBINS, N_SURF, SUBSAMPLE = 49, 40, 150


def scene_dt(scene):
    for k, v in SCENE_DT.items():
        if k in scene:
            return v
    return 0.02


def grid_edges(scene, g):
    if "sce1" in scene:
        return np.arange(-198, -188 + 1, g), np.arange(40, 80 + 1, g)
    if "sce2" in scene:
        return np.arange(-200, -120, g), np.arange(-8, 6, g)
    if "sce3" in scene:
        return np.arange(148, 158, g), np.arange(-80, 22, g)
    return np.arange(0, 20, g), np.arange(-20, 100, g)


def _cat(parts, width=None):
    parts = [np.asarray(p, np.float64) for p in parts]
    if parts:
        return np.concatenate(parts)
    return np.zeros((0,) if width is None else (0, width))


# ---- human velocities -------------------------------------------------------------------------
def _segment_speed(tr):
    """speed of each step of one track and whether its time step is usable (> 1e-6)"""
    d = np.diff(tr, axis=0)
    ok = d[:, 2] > 1e-6
    # squares as the scalar ``dx ** 2`` forms them (libm pow): x * x is 1 ulp away now and then
    sq = np.array([[a ** 2, b ** 2] for a, b in zip(d[:, 0], d[:, 1])], dtype=np.float64).reshape(-1, 2)
    with np.errstate(divide="ignore", invalid="ignore"):
        v = np.sqrt(sq[:, 0] + sq[:, 1]) / d[:, 2]
    return v, ok


def _carry(v, ok, first):
    """replace unusable entries by the latest usable one before them (``first`` when there is none)"""
    idx = np.where(ok, np.arange(len(v)), -1)
    idx = np.maximum.accumulate(idx)
    return np.where(idx >= 0, v[np.maximum(idx, 0)], first)


def human_velocities_global(human):
    """M1 rule: one value per point of every track with >= 2 points; a step with dt <= 1e-6 repeats
    the previous value of the WHOLE list (so it crosses track boundaries; 0 at the very start); the
    last point evaluates the last step once more."""
    out, last = [], None
    for tr in human:
        tr = np.asarray(tr, np.float64)
        if len(tr) < 2:
            continue
        v, ok = _segment_speed(tr)
        v = _carry(v, ok, 0.0 if last is None else last)
        v = np.append(v, v[-1])  # the last step again: the same value, or the same carry
        out.append(v)
        last = v[-1]
    return _cat(out)


def human_velocities_per_track(human):
    """M4 rule: per track with >= 2 points, carry restarts at 0 in every track; the last point
    repeats the value before it.  Returns a list aligned with the tracks kept."""
    out = []
    for tr in human:
        tr = np.asarray(tr, np.float64)
        if len(tr) < 2:
            continue
        v, ok = _segment_speed(tr)
        v = _carry(v, ok, 0.0)
        out.append(np.append(v, v[-1]))
    return out


# ---- finalisation from tables -----------------------------------------------------------------
def js_from_counts(hm, hh):
    p = hm / (hm.sum() + 1e-10)
    q = hh / (hh.sum() + 1e-10)
    m = 0.5 * (p + q)

    def kl(a, b):
        a, b = a / a.sum(), b / b.sum()
        return float(np.sum(a * np.log(a / b)) / np.log(2.0))

    return 0.5 * (kl(p + 1e-10, m + 1e-10) + kl(q + 1e-10, m + 1e-10))


def rmse_frequency(hm, hh):
    a, b = hm.ravel().astype(np.float64), hh.ravel().astype(np.float64)
    keep = (a > 0) | (b > 0)
    if not keep.any():
        return 0.0
    return float(np.sqrt(np.mean((a[keep] - b[keep]) ** 2)))


def gaussian_smooth(a, sigma=2.0, truncate=4.0):
    r = int(truncate * sigma + 0.5)
    x = np.arange(-r, r + 1)
    w = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    w /= w.sum()
    for ax in (0, 1):
        pad = [(r, r) if k == ax else (0, 0) for k in (0, 1)]
        b = np.pad(a, pad, mode="edge")
        n = a.shape[ax]
        a = sum(w[j] * np.take(b, np.arange(j, j + n), axis=ax) for j in range(2 * r + 1))
    return a


def surface_rmse(sm, sh):
    d = sm - sh
    nz = (sm != 0.0) | (sh != 0.0)
    r_all = float(np.sqrt(np.mean(d ** 2)))
    r_nz = float(np.sqrt(np.mean(d[nz] ** 2))) if nz.any() else 0.0
    return r_all, r_nz, int(nz.sum())


# ---- the metrics ------------------------------------------------------------------------------
def _subsample(tr):
    n = len(tr)
    return tr if n <= SUBSAMPLE else tr[np.linspace(0, n - 1, SUBSAMPLE, dtype=int)]


def _clip_bins(x, e):
    return np.clip(np.searchsorted(e, x, side="right") - 1, 0, len(e) - 2)


def _surface(c, t, v, ce, te):
    cnt = np.zeros((N_SURF, N_SURF), np.int64)
    s = np.zeros((N_SURF, N_SURF))
    ci, ti = _clip_bins(c, ce), _clip_bins(t, te)
    np.add.at(cnt, (ti, ci), 1)
    np.add.at(s, (ti, ci), v)
    mean = np.where(cnt > 0, s / np.maximum(cnt, 1), 0.0)
    return cnt, gaussian_smooth(mean)


def metrics(model, human, scene, grid_size=0.5, axis="x", time_interval=5.0):
    model = [np.asarray(m, np.float64).reshape(-1, 4) for m in model]
    human = [np.asarray(h, np.float64).reshape(-1, 3) for h in human]
    dt = scene_dt(scene)
    out = {}

    # M1
    vm, vh = _cat([m[:, 3] for m in model]), human_velocities_global(human)
    if len(vm) and len(vh):
        e = np.linspace(min(vm.min(), vh.min()), max(vm.max(), vh.max()), N_VBINS + 1)
        hm, hh = np.histogram(vm, bins=e)[0], np.histogram(vh, bins=e)[0]
        out["js_velocity"] = js_from_counts(hm, hh)
    else:
        e, hm, hh = np.zeros(0), np.zeros(N_VBINS, np.int64), np.zeros(N_VBINS, np.int64)
        out["js_velocity"] = float("nan")
    out["v_edges"], out["hist_v_model"], out["hist_v_human"] = e, hm.astype(np.int64), hh.astype(np.int64)

    # M2, M3
    xe, ye = grid_edges(scene, grid_size)
    shape = (len(ye) - 1, len(xe) - 1)
    for who, pop in (("model", model), ("human", human)):
        pts = _cat([_subsample(t)[:, :2] for t in pop], 2)
        out["H_points_" + who] = np.histogram2d(pts[:, 0], pts[:, 1], bins=[xe, ye])[0].T.astype(np.int64)
        H = np.zeros(shape, np.int64)
        for t in pop:
            if len(t):
                cell = np.unique(_clip_bins(t[:, 1], ye) * shape[1] + _clip_bins(t[:, 0], xe))
                H.ravel()[cell] += 1
        out["H_traj_" + who] = H
    out["rmse_frequency_points"] = rmse_frequency(out["H_points_model"], out["H_points_human"])
    out["rmse_frequency_trajectories"] = rmse_frequency(out["H_traj_model"], out["H_traj_human"])

    # M4
    k = 0 if axis == "x" else 1
    hs = [h for h in human if len(h) >= 2]
    mc, mt, mv = (_cat([m[:, k] for m in model]), _cat([np.arange(len(m)) * dt for m in model]),
                  _cat([m[:, 3] for m in model]))
    hc, ht, hv = _cat([h[:, k] for h in hs]), _cat([h[:, 2] for h in hs]), _cat(human_velocities_per_track(human))
    zero = np.zeros((N_SURF, N_SURF))
    if len(mc) and len(hc):
        c_all, t_all = np.concatenate([mc, hc]), np.concatenate([mt, ht])
        ce = np.linspace(c_all.min(), c_all.max(), N_SURF + 1)
        te = np.linspace(t_all.min(), t_all.max(), N_SURF + 1)
        cm, sm = _surface(mc, mt, mv, ce, te)
        ch, sh = _surface(hc, ht, hv, ce, te)
        r_all, r_nz, n_nz = surface_rmse(sm, sh)
    else:
        ce = te = np.zeros(0)
        cm = ch = zero.astype(np.int64)
        sm = sh = zero
        r_all, r_nz, n_nz = float("nan"), float("nan"), 0
    out.update(coord_edges=ce, time_edges=te, surf_cnt_model=cm, surf_cnt_human=ch, surface_model=sm,
               surface_human=sh, surface_rmse=r_all, surface_rmse_nonzero=r_nz, surface_points_nonzero=n_nz)

    # M5
    pm = _cat([np.column_stack([m[:, 0], m[:, 1], np.arange(len(m)) * dt]) for m in model], 3)
    ph = _cat(human, 3)
    se = np.zeros(0)
    if len(pm) and len(ph):
        se = np.arange(min(ph[:, 2].min(), pm[:, 2].min()), max(ph[:, 2].max(), pm[:, 2].max()) + 1e-9, time_interval)
    ns = max(len(se) - 1, 0)
    cnt, cen = {}, {}
    for who, p in (("model", pm), ("human", ph)):
        c, sx, sy = np.zeros(ns, np.int64), np.zeros(ns), np.zeros(ns)
        if ns:
            i = np.searchsorted(se, p[:, 2], side="right") - 1
            ok = (i >= 0) & (i < ns)
            np.add.at(c, i[ok], 1)
            np.add.at(sx, i[ok], p[ok, 0])
            np.add.at(sy, i[ok], p[ok, 1])
        cnt[who], cen[who] = c, np.column_stack([sx, sy]) / np.maximum(c, 1)[:, None]
    both = (cnt["model"] > 0) & (cnt["human"] > 0)
    errs = np.sqrt(((cen["model"] - cen["human"]) ** 2).sum(axis=1))[both]
    out["plane_rmse"] = float(np.sqrt(np.mean(errs ** 2))) if len(errs) else float("nan")
    out["plane_slice_errors"] = errs.tolist()
    out["slice_edges"], out["slice_cnt_model"], out["slice_cnt_human"] = se, cnt["model"], cnt["human"]
    return out
