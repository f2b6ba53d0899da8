"""GPU checks of cvae_amd.validate (csrc/cvae_metrics.h through cvae_val_ranges / cvae_val_accumulate).

Tolerances: integer tables are bit-equal; js_velocity and both rmse_frequency_* depend
on integers only -> 1e-12; the sums are 64-bit fixed point with quantum q = 2^-24, every mean is
within q/2 ~ 3e-8 of the exact mean, carried through convex weights (the Gaussian) and a centroid
distance -> 1e-7 for the smoothed surfaces, both surface RMSEs and the plane RMSE.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.join(os.path.dirname(HERE), "defensive-model-vae_amd")]
import validate_oracle as VO  # noqa: E402

pytestmark = pytest.mark.gpu
INT_TOL, FIX_TOL = 1e-12, 1e-7
INT_TABLES = ("hist_v", "H_points", "H_traj", "surf_cnt", "slice_cnt")


@pytest.fixture(scope="module")
def V():
    from cvae_amd import validate
    return validate


@pytest.fixture(scope="module")
def G():
    return np.load(os.path.join(HERE, "golden", "validate.npz"))


def split(flat, off):
    return [flat[off[i]:off[i + 1]] for i in range(len(off) - 1)]


def close(a, b, tol):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape
    both_nan = np.isnan(a) & np.isnan(b)
    d = np.abs(np.where(both_nan, 0.0, a - b))
    print("max |diff|", float(d.max(initial=0.0)), "tol", tol)
    assert not np.isnan(d).any() and d.max(initial=0.0) <= tol


def same_int(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and np.array_equal(a.astype(np.int64), b.astype(np.int64))


# ---- golden parity ---------------------------------------------------------------------------------
@pytest.mark.parametrize("s", ["sce1", "sce3"])
@pytest.mark.parametrize("g", [0.5, 1.0])
def test_golden_parity(V, G, s, g):
    model = split(G[s + "/model_flat"], G[s + "/model_offsets"])
    human = split(G[s + "/human_flat"], G[s + "/human_offsets"])
    ref = V.HumanReference(human, s, grid_size=g)
    q = f"{s}/g{g}/"
    for axis, iv in (("x", 5.0), ("y", 1.0)):
        r = V.metrics(model, ref, axis=axis, time_interval=iv)
        same_int(r["hist_v_model"], G[s + "/m1_hist_model"])
        same_int(r["hist_v_human"], G[s + "/m1_hist_human"])
        for k, gk in (("H_points", "m2_H"), ("H_traj", "m3_H")):
            same_int(r[k + "_model"], G[q + gk + "_model"])
            same_int(r[k + "_human"], G[q + gk + "_human"])
        a, p = f"{s}/m4_{axis}/", f"{s}/m5_{iv}/"
        same_int(r["surf_cnt_model"], G[a + "cnt_model"])
        same_int(r["surf_cnt_human"], G[a + "cnt_human"])
        same_int(r["slice_cnt_model"], G[p + "cnt_model"])
        same_int(r["slice_cnt_human"], G[p + "cnt_human"])
        close(r["js_velocity"], G[s + "/m1_js"], INT_TOL)
        close(r["rmse_frequency_points"], G[q + "m2_rmse"], INT_TOL)
        close(r["rmse_frequency_trajectories"], G[q + "m3_rmse"], INT_TOL)
        close(r["surface_model"], G[a + "surf_model"], FIX_TOL)
        close(r["surface_human"], G[a + "surf_human"], FIX_TOL)
        close(r["surface_rmse"], G[a + "rmse_all"], FIX_TOL)
        close(r["surface_rmse_nonzero"], G[a + "rmse_nz"], FIX_TOL)
        assert r["surface_points_nonzero"] == int(G[a + "n_nz"])
        close(r["plane_rmse"], G[p + "rmse"], FIX_TOL)
        close(r["plane_slice_errors"], G[p + "errors"], FIX_TOL)


# ---- synthetic adversarial populations against the oracle ------------------------------------------
LENGTHS = (0, 1, 2, 63, 64, 65, 150, 151, 152, 777)
SCENE = "sce1"  # x in [-198, -187], y in [40, 80]


def edge_values(e):
    """values on the first / an interior / the last edge, one ulp either side of each, and outside"""
    pts = []
    for v in (e[0], e[len(e) // 2], e[-1]):
        pts += [v, np.nextafter(v, -np.inf), np.nextafter(v, np.inf)]
    return np.array(pts + [e[0] - 3.0, e[-1] + 3.0])


def synthetic_model(P, rng, dt=0.02):
    xe, ye = VO.grid_edges(SCENE, 0.5)
    ex, ey = edge_values(xe), edge_values(ye)
    out = []
    for p in range(P):
        n = LENGTHS[p % len(LENGTHS)] if P > 1 else 777
        t = np.arange(n) * dt
        tr = np.column_stack([-193.0 + 4.0 * np.sin(0.9 * t + p), 45.0 + 2.5 * t + 0.1 * p, 0.1 * t,
                              np.abs(8.0 - 0.5 * t + 0.3 * np.cos(p + t))]).reshape(n, 4)
        k = min(n, len(ex))
        tr[:k, 0] = rng.permutation(ex)[:k]  # on edges, one ulp off, outside on both sides
        if n > len(ex):
            tr[-k:, 1] = rng.permutation(ey)[:k]
        out.append(tr)
    if P >= 3:
        out[1] = np.tile([[-192.3, 50.2, 0.0, 5.0]], (len(out[1]) or 1, 1))[:max(len(out[1]), 1)]  # one cell
        out[2] = out[1].copy()  # two trajectories visiting identical cells
    return out


def synthetic_human(P, rng):
    out = []
    for p in range(P):
        n = LENGTHS[(p + 3) % len(LENGTHS)] if P > 1 else 152
        t = np.cumsum(np.full(n, 0.1)) + 0.05 * p
        tr = np.column_stack([-194.0 + 3.0 * np.cos(0.2 * t + p), 42.0 + 1.1 * t, t]).reshape(n, 3)
        out.append(tr)
    if P >= 1 and len(out[0]) >= 3:
        out[0][1, 2] = out[0][0, 2]  # dt <= 1e-6 at the first step of the first track
    if P >= 3:
        j = next(i for i in range(1, P) if len(out[i]) >= 3)
        out[j][1, 2] = out[j][0, 2] + 5e-7  # ... and at a track boundary (carries across it)
    return out


def compare(r, o):
    for k in INT_TABLES:
        same_int(r[k + "_model"], o[k + "_model"])
        same_int(r[k + "_human"], o[k + "_human"])
    for k in ("v_edges", "coord_edges", "time_edges"):
        assert np.array_equal(r[k], o[k])
    if len(o["slice_edges"]) >= 2:
        assert np.array_equal(r["slice_edges"], o["slice_edges"])
    for k in ("js_velocity", "rmse_frequency_points", "rmse_frequency_trajectories"):
        close(r[k], o[k], INT_TOL)
    for k in ("surface_model", "surface_human", "surface_rmse", "surface_rmse_nonzero", "plane_rmse",
              "plane_slice_errors"):
        close(r[k], o[k], FIX_TOL)
    assert r["surface_points_nonzero"] == o["surface_points_nonzero"]


@pytest.mark.parametrize("P,PH", [(0, 0), (0, 3), (3, 0), (1, 1), (3, 3), (70, 70), (70, 1), (1, 70)])
def test_synthetic_against_oracle(V, P, PH):
    rng = np.random.default_rng(100 * P + PH)
    model, human = synthetic_model(P, rng), synthetic_human(PH, rng)
    ref = V.HumanReference(human, SCENE, grid_size=0.5)
    for axis, iv in (("x", 5.0), ("y", 0.7)):
        compare(V.metrics(model, ref, axis=axis, time_interval=iv), VO.metrics(model, human, SCENE, 0.5, axis, iv))


def test_degenerate_velocity_range_and_long_interval(V):
    """vmin == vmax (np.linspace of equal ends: everything lands in the closed last bin) and a
    time_interval longer than the time span (NaN and an empty list)."""
    model = [np.column_stack([np.linspace(-195, -190, n), np.linspace(45, 60, n), np.zeros(n), np.full(n, 4.0)])
             for n in (65, 151)]
    human = [np.array([[-193.0, 45.0, 0.0], [-193.0, 49.0, 1.0]])]  # speed exactly 4.0 at both points
    ref = V.HumanReference(human, SCENE)
    assert np.all(ref.v_global == 4.0)
    r = V.metrics(model, ref, time_interval=1000.0)
    o = VO.metrics(model, human, SCENE, 0.5, "x", 1000.0)
    assert r["v_edges"][0] == r["v_edges"][-1]
    assert r["hist_v_model"][-1] == sum(len(m) for m in model) and r["hist_v_model"][:-1].sum() == 0
    assert np.isnan(r["plane_rmse"]) and r["plane_slice_errors"] == []
    compare(r, o)


# ---- determinism -----------------------------------------------------------------------------------
def test_bit_identical_across_order_and_geometry(V, G):
    s = "sce1"
    model = split(G[s + "/model_flat"], G[s + "/model_offsets"])
    human = split(G[s + "/human_flat"], G[s + "/human_offsets"])
    runs = []
    for waves, order in ((0, 1), (1, -1), (8, 1), (0, 1)):
        ref = V.HumanReference(human, s, block_waves=waves)  # (the M1 velocity carry is order-dependent by definition)
        runs.append(V.metrics(model[::order], ref, axis="y", time_interval=1.0))
    keys = [k + w for k in INT_TABLES for w in ("_model", "_human")] + ["surf_sum_model", "slice_sum_model"]
    for r in runs[1:]:
        for k in keys:
            assert np.array_equal(r[k], runs[0][k]), k
        for k in ("surface_model", "surface_human"):
            assert np.array_equal(r[k], runs[0][k]), k
        for k in ("js_velocity", "rmse_frequency_points", "rmse_frequency_trajectories", "surface_rmse", "plane_rmse"):
            assert r[k] == runs[0][k], k


# ---- device path -----------------------------------------------------------------------------------
def test_device_tracks_equal_host_lists(V, G):
    from cvae_amd import mpc
    M = np.load(os.path.join(HERE, "golden", "mpc.npz"))
    wp, init = M["c1/waypoints"], M["c1/init"]  # test0: N=30, control horizon 20, dt=0.05
    wps, inits = [], []
    for k in range(3):
        w = wp.copy()
        w[:, 0] += 1.5 * k - 195.0
        w[:, 1] += 0.5 * k + 50.0
        i0 = init.copy()
        i0[0] += 1.5 * k - 195.0
        i0[1] += 0.5 * k + 50.0
        wps.append(w)
        inits.append(i0)
    cfg = dict(prediction_horizon=30, control_horizon=20, dt=0.05)
    dev = mpc.track_batch_device(wps, np.array(inits), **cfg)
    host = mpc.track_batch(wps, np.array(inits), **cfg)
    assert np.array_equal(dev.offsets.cpu().numpy(), dev.offsets_host)
    for p, (_, st, _) in enumerate(host):
        a, b = dev.offsets_host[p], dev.offsets_host[p + 1]
        assert np.array_equal(dev.states[a:b].cpu().numpy(), st)
    human = split(G["sce1/human_flat"], G["sce1/human_offsets"])
    ref = V.HumanReference(human, "sce1")
    rd = V.metrics(dev, ref, time_interval=1.0)
    rh = V.metrics([st for _, st, _ in host], ref, time_interval=1.0)
    for k, v in rd.items():
        if isinstance(v, np.ndarray):
            assert np.array_equal(v, rh[k], equal_nan=True), k
        elif isinstance(v, list):
            assert v == rh[k], k
        else:
            assert v == rh[k] or (np.isnan(v) and np.isnan(rh[k])), k


# ---- caps and input checks -------------------------------------------------------------------------
def test_caps_raise_before_any_launch(V):
    import ctypes as C

    import torch
    from cvae_amd._lib import CvaeError, CvaeValConfig, CvaeValTables, lib
    human = [np.array([[-193.0, 45.0, 0.0], [-193.0, 49.0, 1.0]])]
    with pytest.raises(CvaeError, match="65536 cells"):
        ref = V.HumanReference(human, "sce4", grid_size=0.125)  # 160 x 960 cells
        V.metrics([np.array([[1.0, 1.0, 0.0, 2.0]])], ref)
    # non-monotone offsets: straight at the C-ABI, with device buffers nothing may touch
    rows = torch.zeros((4, 4), dtype=torch.float64, device="cuda")
    off_h = np.array([0, 3, 2, 4], np.int64)
    off = torch.from_numpy(off_h).cuda()
    out = torch.full((16,), 7, dtype=torch.int64, device="cuda")
    c = CvaeValConfig()
    c.dt, c.stride, c.x_col, c.y_col, c.t_col, c.v_col, c.coord_col = 0.02, 4, 0, 1, -1, 3, 0
    rc = lib().cvae_val_ranges(C.byref(c), 3, C.c_void_p(rows.data_ptr()), 4, C.c_void_p(off.data_ptr()),
                               off_h.ctypes.data_as(C.c_void_p), None, C.c_void_p(out.data_ptr()), None)
    assert rc < 0 and b"monotone" in lib().cvae_last_error()
    t = CvaeValTables()
    rc = lib().cvae_val_accumulate(C.byref(c), 3, C.c_void_p(rows.data_ptr()), 4, C.c_void_p(off.data_ptr()),
                                   off_h.ctypes.data_as(C.c_void_p), None, None, None,
                                   np.zeros(16, np.uint64).ctypes.data_as(C.c_void_p), C.byref(t), None)
    assert rc < 0 and b"monotone" in lib().cvae_last_error()
    off_h[:] = [0, 1, 2, 3]  # does not end at n_rows
    rc = lib().cvae_val_ranges(C.byref(c), 3, C.c_void_p(rows.data_ptr()), 4, C.c_void_p(off.data_ptr()),
                               off_h.ctypes.data_as(C.c_void_p), None, C.c_void_p(out.data_ptr()), None)
    assert rc < 0 and b"end at n_rows" in lib().cvae_last_error()
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 7).all()  # no launch happened
    with pytest.raises(CvaeError, match="1024"):
        V.metrics([np.array([[2000.0, 1.0, 0.0, 2.0]])], V.HumanReference(human, "sce1"))


# ---- checkpoint to metrics -------------------------------------------------------------------------
def test_validate_checkpoint_equals_staged_host_run(V, G, monkeypatch):
    """generate -> track on the device -> metrics, against the same stages run through host lists.
    Generation itself is covered by test_hip_parity; the fixed test weights do not produce increasing
    times, so the generator is replaced by one returning the sce1 log tracks of mpc.npz as [t, x, y]."""
    from cvae_amd import mpc, tools
    M = np.load(os.path.join(HERE, "golden", "mpc.npz"))
    wps = [M[f"c{k}/waypoints"] for k in (2, 3)]  # StaticBlindTown05 logs, (x, y, t)
    start_states = np.array([M[f"c{k}/init"] for k in (2, 3)])
    seen = {}

    def fake_generate(model_path, start_points, seq_len, dim, latent_dim, z=None, device=None):
        seen["args"] = (model_path, np.asarray(start_points).copy(), seq_len, dim, latent_dim)
        out = np.stack([w[:, [2, 0, 1]] for w in wps])
        out[:, 0, 0] = -0.01  # the first time is overwritten with 0 downstream (Distribution.py:78)
        return out

    monkeypatch.setattr(tools, "generate_trajectories", fake_generate)
    human = split(G["sce1/human_flat"], G["sce1/human_offsets"])
    ref = V.HumanReference(human, "sce1")
    tm = {}
    r = V.validate_checkpoint("ckpt.pth", start_states, ref, seq_len=10, dim=3, latent_dim=8, timings=tm)
    assert set(tm) == {"generate", "track", "metrics"}
    assert seen["args"][0] == "ckpt.pth" and np.array_equal(seen["args"][1], start_states[:, :2])
    host = mpc.track_batch([w.copy() for w in wps], start_states, prediction_horizon=30, control_horizon=20, dt=0.02)
    rh = V.metrics([st for _, st, _ in host], ref)
    for k, v in r.items():
        if isinstance(v, np.ndarray):
            assert np.array_equal(v, rh[k], equal_nan=True), k
    assert r["hist_v_model"].sum() == sum(len(st) for _, st, _ in host) > 2
