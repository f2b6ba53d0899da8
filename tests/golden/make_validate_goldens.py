"""Fixtures for the validation-metric tests (run here, where /root/reference exists):

the reference's own model-vs-human validation (``Distribution.py`` / ``Spatial_Distribution.py``)
run on

* ``sce1`` — its 38 recorded tracks ``results/GeneratedData/tracked_trajectory_sce1_*.npy`` against
  ``load_human_trajectories`` of 12 sce1 logs (grid 11x41 m, dt 0.02);
* ``sce3`` — 4 recorded sce3 tracks against the first sce3 logs of one folder (grid 10x102 m, dt 0.015).

Recorded per scene: the inputs (ragged, flat + offsets), both human-velocity rules
(``calculate_human_velocities`` and ``_prepare_human_stv_data``), and the reference functions' own
outputs — M1 velocity JS (``plot_velocity_distribution``: its ``entropy`` calls are observed, the
function returns nothing), M2 ``calculate_rmse_frequency``, M3 ``calculate_rmse_frequency_new`` /
``_count_trajectories_per_grid`` at grid 0.5 and 1.0, M4 ``_build_surface_from_stv`` +
``calculate_surface_rmse`` for both axes, M5 ``compute_spatiotemporal_plane_rmse`` at 5 s and 1 s.
Count tables the reference forms but does not return (np.histogram / np.histogram2d / digitize
counts) are taken with the same numpy call on the same edges.  Wall time per metric is metadata.

    python tests/golden/make_validate_goldens.py
"""
import contextlib
import io
import json
import os
import sys
import time

import numpy as np

os.environ.setdefault("MPLBACKEND", "Agg")
HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path[:0] = [REF]
_cwd = os.getcwd()
os.chdir(REF)
with contextlib.redirect_stdout(io.StringIO()):
    import Distribution as D  # noqa: E402  (the reference, imported read-only)
    import Spatial_Distribution as S  # noqa: E402
import matplotlib.pyplot as plt  # noqa: E402
os.chdir(_cwd)

SCENES = {  # name: (model file name, scene folder, sub-folder, n_model, n_human)
    "sce1": ("vae_offset_sce1_cond_ld8_epoch3000.pth", "StaticBlindTown05", "减速", None, 12),
    "sce3": ("vae_offset_sce3_cond_ld8_epoch3000.pth", "PredictableMovementTown05", "减速+转向", 4, 6),
}
GRIDS = (0.5, 1.0)
INTERVALS = (5.0, 1.0)

_entropy_out = []
_orig_entropy = D.entropy


def _recording_entropy(*a, **k):
    r = _orig_entropy(*a, **k)
    _entropy_out.append(float(r))
    return r


D.entropy = _recording_entropy


def ragged(trajs, width):
    off = np.zeros(len(trajs) + 1, np.int64)
    off[1:] = np.cumsum([len(t) for t in trajs])
    flat = np.concatenate([np.asarray(t, np.float64)[:, :width] for t in trajs]) if trajs else np.zeros((0, width))
    return np.ascontiguousarray(flat), off


def timed(meta, key, fn, *a, **k):
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        r = fn(*a, **k)
    meta[key] = round(time.perf_counter() - t0, 4)
    return r


def scene(name, out, meta):
    model_name, folder, sub, n_model, n_human = SCENES[name]
    files = sorted(f for f in os.listdir(os.path.join(REF, "results/GeneratedData"))
                   if f.startswith(f"tracked_trajectory_{name}_") and f.endswith(".npy"))[:n_model]
    model = [np.load(os.path.join(REF, "results/GeneratedData", f)) for f in files]
    d = os.path.join(REF, "DefensiveData", folder, sub)
    csvs = [os.path.join(d, f) for f in sorted(os.listdir(d)) if f.lower().endswith(".csv")][:n_human]
    os.chdir(REF)
    with contextlib.redirect_stdout(io.StringIO()):
        human = [np.asarray(h, np.float64) for h in D.load_human_trajectories(csvs, model_name)]
    os.chdir(_cwd)
    p = name + "/"
    m = meta[name] = {"model_files": files, "human_files": [os.path.basename(c) for c in csvs], "seconds": {}}
    sec = m["seconds"]
    out[p + "model_flat"], out[p + "model_offsets"] = ragged(model, 4)
    out[p + "human_flat"], out[p + "human_offsets"] = ragged(human, 3)
    out[p + "dt"] = np.float64(S._get_model_time_step(model_name))

    # M1
    t0 = time.perf_counter()
    gv = D.extract_velocities_from_trajectories(model)
    hv = D.calculate_human_velocities(human)
    _entropy_out.clear()
    with contextlib.redirect_stdout(io.StringIO()):
        try:
            D.plot_velocity_distribution(gv, hv, None)
        except Exception:  # the plotting half may not run headless; the JS half has run by then
            pass
    plt.close("all")
    sec["m1"] = round(time.perf_counter() - t0, 4)
    assert len(_entropy_out) == 2
    out[p + "human_v_global"] = hv
    out[p + "m1_js"] = np.float64(0.5 * (_entropy_out[0] + _entropy_out[1]))
    edges = np.linspace(min(np.min(gv), np.min(hv)), max(np.max(gv), np.max(hv)), 50)  # Distribution.py:310-312
    out[p + "m1_edges"] = edges
    out[p + "m1_hist_model"] = np.histogram(gv, bins=edges)[0].astype(np.int64)
    out[p + "m1_hist_human"] = np.histogram(hv, bins=edges)[0].astype(np.int64)

    for g in GRIDS:
        q = f"{p}g{g}/"
        xe, ye = S._get_grid_edges(model_name, g)
        out[q + "x_edges"], out[q + "y_edges"] = xe, ye
        gc = S.extract_coordinates_from_trajectories(model)
        hc = S.extract_human_coordinates(human)
        out[q + "m2_rmse"] = np.float64(timed(sec, f"m2_g{g}", S.calculate_rmse_frequency, gc, hc, model_name, g))
        out[q + "m2_H_model"] = np.histogram2d(gc[:, 0], gc[:, 1], bins=[xe, ye])[0].T.astype(np.int64)
        out[q + "m2_H_human"] = np.histogram2d(hc[:, 0], hc[:, 1], bins=[xe, ye])[0].T.astype(np.int64)
        out[q + "m3_rmse"] = np.float64(timed(sec, f"m3_g{g}", S.calculate_rmse_frequency_new, model, human,
                                              model_name, g))
        out[q + "m3_H_model"] = S._count_trajectories_per_grid(model, model_name, g)[0].astype(np.int64)
        out[q + "m3_H_human"] = S._count_trajectories_per_grid(human, model_name, g)[0].astype(np.int64)

    for axis in ("x", "y"):
        q = f"{p}m4_{axis}/"
        t0 = time.perf_counter()
        mc, mt, mv = S._prepare_model_stv_data(model, model_name, axis=axis)
        hc, ht, hvl = S._prepare_human_stv_data(human, axis=axis)
        cr, tr = S._calculate_unified_axes_ranges(mc, mt, hc, ht)
        _, _, sm = S._build_surface_from_stv(mc, mt, mv, 40, 40, cr, tr)
        _, _, sh = S._build_surface_from_stv(hc, ht, hvl, 40, 40, cr, tr)
        with contextlib.redirect_stdout(io.StringIO()):
            r_all, _ = S.calculate_surface_rmse(sm, sh, include_zero_velocity=True)
            r_nz, n_nz = S.calculate_surface_rmse(sm, sh, include_zero_velocity=False)
        sec[f"m4_{axis}"] = round(time.perf_counter() - t0, 4)
        ce, te = np.linspace(cr[0], cr[1], 41), np.linspace(tr[0], tr[1], 41)  # :900-901
        out[q + "coord_edges"], out[q + "time_edges"] = ce, te
        for who, cl, tl in (("model", mc, mt), ("human", hc, ht)):
            ci = np.clip(np.digitize(np.concatenate(cl), ce) - 1, 0, 39)  # :906-910
            ti = np.clip(np.digitize(np.concatenate(tl), te) - 1, 0, 39)
            cnt = np.zeros((40, 40), np.int64)
            np.add.at(cnt, (ti, ci), 1)
            out[q + "cnt_" + who] = cnt
        out[q + "surf_model"], out[q + "surf_human"] = sm, sh
        out[q + "rmse_all"], out[q + "rmse_nz"], out[q + "n_nz"] = np.float64(r_all), np.float64(r_nz), np.int64(n_nz)
        if axis == "x":
            out[p + "human_v_pertrack"] = np.concatenate(hvl)

    dt = float(out[p + "dt"])
    for iv in INTERVALS:
        q = f"{p}m5_{iv}/"
        rmse, errs = timed(sec, f"m5_{iv}", S.compute_spatiotemporal_plane_rmse, human, model, model_name, iv)
        out[q + "rmse"], out[q + "errors"] = np.float64(rmse), np.asarray(errs, np.float64)
        th = np.concatenate([h[:, 2] for h in human])
        tm = np.concatenate([np.array([i * dt for i in range(len(t))]) for t in model])  # :1393
        e = np.arange(min(th.min(), tm.min()), max(th.max(), tm.max()) + 1e-9, iv)  # :1401-1403
        out[q + "edges"] = e
        for who, t in (("model", tm), ("human", th)):
            out[q + "cnt_" + who] = np.array([int(((t >= e[i]) & (t < e[i + 1])).sum()) for i in range(len(e) - 1)],
                                             np.int64)
    print(name, json.dumps(sec), flush=True)


def main():
    out, meta = {}, {}
    for name in SCENES:
        scene(name, out, meta)
    out["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
    np.savez_compressed(os.path.join(HERE, "validate.npz"), **out)
    print(os.path.getsize(os.path.join(HERE, "validate.npz")), "bytes")


if __name__ == "__main__":
    main()
