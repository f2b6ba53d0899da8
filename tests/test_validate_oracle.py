"""CPU checks of the validation metrics against the reference's recorded outputs
(tests/golden/validate.npz, made by tests/golden/make_validate_goldens.py):

* the numpy restatement tests/validate_oracle.py reproduces every golden — integer tables and edges
  bit-equal, scalars and surfaces within 1e-12 (float64 sums of at most 1,600 terms of order 1 in
  another order);
* the package's host finalisation (JS from counts, the Gaussian restatement, both RMSE masks, the
  plane RMSE) reproduces the goldens from the goldens' own tables within 1e-12;
* both human-velocity rules reproduce the goldens bit-equally.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.join(os.path.dirname(HERE), "defensive-model-vae_amd")]
import validate_oracle as VO  # noqa: E402

from cvae_amd import validate as V  # noqa: E402

TOL = 1e-12
SCENES, GRIDS, AXES, INTERVALS = ("sce1", "sce3"), (0.5, 1.0), ("x", "y"), (5.0, 1.0)


@pytest.fixture(scope="module")
def G():
    return np.load(os.path.join(HERE, "golden", "validate.npz"))


def split(flat, off):
    return [flat[off[i]:off[i + 1]] for i in range(len(off) - 1)]


def population(G, s):
    return (split(G[s + "/model_flat"], G[s + "/model_offsets"]), split(G[s + "/human_flat"], G[s + "/human_offsets"]))


_cache = {}


def oracle(G, s, g, axis, iv):
    k = (s, g, axis, iv)
    if k not in _cache:
        m, h = population(G, s)
        _cache[k] = VO.metrics(m, h, s, g, axis, iv)
    return _cache[k]


def same_int(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and np.array_equal(a.astype(np.int64), b.astype(np.int64))


def same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("s", SCENES)
def test_scene_constants(G, s):
    assert VO.scene_dt(s) == V.scene_dt(s) == float(G[s + "/dt"])
    for g in GRIDS:
        for got in (VO.grid_edges(s, g), V.grid_edges(s, g)):
            same_bits(got[0], G[f"{s}/g{g}/x_edges"])
            same_bits(got[1], G[f"{s}/g{g}/y_edges"])


@pytest.mark.parametrize("s", SCENES)
@pytest.mark.parametrize("mod", [VO, V], ids=["oracle", "package"])
def test_human_velocity_rules_bit_equal(G, s, mod):
    _, h = population(G, s)
    same_bits(mod.human_velocities_global(h), G[s + "/human_v_global"])
    same_bits(np.concatenate(mod.human_velocities_per_track(h)), G[s + "/human_v_pertrack"])


@pytest.mark.parametrize("s", SCENES)
def test_oracle_velocity_js(G, s):
    o = oracle(G, s, 0.5, "x", 5.0)
    same_bits(o["v_edges"], G[s + "/m1_edges"])
    same_int(o["hist_v_model"], G[s + "/m1_hist_model"])
    same_int(o["hist_v_human"], G[s + "/m1_hist_human"])
    assert abs(o["js_velocity"] - float(G[s + "/m1_js"])) <= TOL


@pytest.mark.parametrize("s", SCENES)
@pytest.mark.parametrize("g", GRIDS)
def test_oracle_rmse_frequency(G, s, g):
    o, q = oracle(G, s, g, "x", 5.0), f"{s}/g{g}/"
    for k, gk in (("H_points", "m2_H"), ("H_traj", "m3_H")):
        same_int(o[k + "_model"], G[q + gk + "_model"])
        same_int(o[k + "_human"], G[q + gk + "_human"])
    assert abs(o["rmse_frequency_points"] - float(G[q + "m2_rmse"])) <= TOL
    assert abs(o["rmse_frequency_trajectories"] - float(G[q + "m3_rmse"])) <= TOL


@pytest.mark.parametrize("s", SCENES)
@pytest.mark.parametrize("axis", AXES)
def test_oracle_surface(G, s, axis):
    o, q = oracle(G, s, 0.5, axis, 5.0), f"{s}/m4_{axis}/"
    same_bits(o["coord_edges"], G[q + "coord_edges"])
    same_bits(o["time_edges"], G[q + "time_edges"])
    same_int(o["surf_cnt_model"], G[q + "cnt_model"])
    same_int(o["surf_cnt_human"], G[q + "cnt_human"])
    assert np.max(np.abs(o["surface_model"] - G[q + "surf_model"])) <= TOL
    assert np.max(np.abs(o["surface_human"] - G[q + "surf_human"])) <= TOL
    assert abs(o["surface_rmse"] - float(G[q + "rmse_all"])) <= TOL
    assert abs(o["surface_rmse_nonzero"] - float(G[q + "rmse_nz"])) <= TOL
    assert o["surface_points_nonzero"] == int(G[q + "n_nz"])


@pytest.mark.parametrize("s", SCENES)
@pytest.mark.parametrize("iv", INTERVALS)
def test_oracle_planes(G, s, iv):
    o, q = oracle(G, s, 0.5, "x", iv), f"{s}/m5_{iv}/"
    same_bits(o["slice_edges"], G[q + "edges"])
    same_int(o["slice_cnt_model"], G[q + "cnt_model"])
    same_int(o["slice_cnt_human"], G[q + "cnt_human"])
    assert len(o["plane_slice_errors"]) == len(G[q + "errors"])
    assert np.max(np.abs(np.array(o["plane_slice_errors"]) - G[q + "errors"]), initial=0.0) <= TOL
    assert abs(o["plane_rmse"] - float(G[q + "rmse"])) <= TOL


def test_sanity_anchor(G):
    """sce1, 12 human logs, grid 0.5: the order of magnitude the reference prints."""
    assert 6.0 < float(G["sce1/g0.5/m3_rmse"]) < 7.5
    assert len(G["sce1/m5_1.0/errors"]) == 16


# ---- the package's host finalisation, from the goldens' own tables --------------------------------
@pytest.mark.parametrize("s", SCENES)
def test_package_js_from_counts(G, s):
    js = V.js_from_counts(G[s + "/m1_hist_model"], G[s + "/m1_hist_human"])
    assert abs(js - float(G[s + "/m1_js"])) <= TOL


@pytest.mark.parametrize("s", SCENES)
@pytest.mark.parametrize("g", GRIDS)
def test_package_rmse_frequency(G, s, g):
    q = f"{s}/g{g}/"
    assert abs(V.rmse_frequency(G[q + "m2_H_model"], G[q + "m2_H_human"]) - float(G[q + "m2_rmse"])) <= TOL
    assert abs(V.rmse_frequency(G[q + "m3_H_model"], G[q + "m3_H_human"]) - float(G[q + "m3_rmse"])) <= TOL


@pytest.mark.parametrize("s", SCENES)
@pytest.mark.parametrize("axis", AXES)
def test_package_surface_finalisation(G, s, axis):
    """exact float64 sums (from the oracle's binning, whose counts are the goldens') -> the package's
    mean + Gaussian restatement + both RMSE masks"""
    q = f"{s}/m4_{axis}/"
    m, h = population(G, s)
    k, dt = (0 if axis == "x" else 1), float(G[s + "/dt"])
    ce, te = G[q + "coord_edges"], G[q + "time_edges"]
    hs = [t for t in h if len(t) >= 2]
    pops = {"model": (np.concatenate([t[:, k] for t in m]), np.concatenate([np.arange(len(t)) * dt for t in m]),
                      np.concatenate([t[:, 3] for t in m])),
            "human": (np.concatenate([t[:, k] for t in hs]), np.concatenate([t[:, 2] for t in hs]),
                      G[s + "/human_v_pertrack"])}
    surf = {}
    for who, (c, t, v) in pops.items():
        ci = np.clip(np.digitize(c, ce) - 1, 0, 39)
        ti = np.clip(np.digitize(t, te) - 1, 0, 39)
        total = np.zeros((40, 40))
        np.add.at(total, (ti, ci), v)
        surf[who] = V.surface_from_tables(G[q + "cnt_" + who], total)
        assert np.max(np.abs(surf[who] - G[q + "surf_" + who])) <= TOL
    r_all, r_nz, n_nz = V.surface_rmse(G[q + "surf_model"], G[q + "surf_human"])
    assert abs(r_all - float(G[q + "rmse_all"])) <= TOL and abs(r_nz - float(G[q + "rmse_nz"])) <= TOL
    assert n_nz == int(G[q + "n_nz"])


@pytest.mark.parametrize("s", SCENES)
@pytest.mark.parametrize("iv", INTERVALS)
def test_package_plane_finalisation(G, s, iv):
    q = f"{s}/m5_{iv}/"
    m, h = population(G, s)
    dt, e = float(G[s + "/dt"]), G[q + "edges"]
    pm = np.concatenate([np.column_stack([t[:, 0], t[:, 1], np.arange(len(t)) * dt]) for t in m])
    ph = np.concatenate(h)
    sums = []
    for p in (pm, ph):
        i = np.searchsorted(e, p[:, 2], side="right") - 1
        ok = (i >= 0) & (i < len(e) - 1)
        c, sx, sy = np.zeros(len(e) - 1, np.int64), np.zeros(len(e) - 1), np.zeros(len(e) - 1)
        np.add.at(c, i[ok], 1)
        np.add.at(sx, i[ok], p[ok, 0])
        np.add.at(sy, i[ok], p[ok, 1])
        sums += [c, sx, sy]
    same_int(sums[0], G[q + "cnt_model"])
    rmse, errs = V.plane_rmse(*sums)
    assert abs(rmse - float(G[q + "rmse"])) <= TOL
    assert np.max(np.abs(np.array(errs) - G[q + "errors"])) <= TOL


def test_gaussian_restatement_edges():
    """mode='nearest' on a small odd-shaped array whose border matters: weights sum to 1 along both
    axes, so a constant stays constant and a one-hot corner keeps its mass inside."""
    a = np.full((5, 7), 3.25)
    assert np.max(np.abs(V.gaussian_filter_nearest(a) - 3.25)) <= 1e-14
    b = np.zeros((5, 7))
    b[0, 0] = 1.0
    s = V.gaussian_filter_nearest(b)
    assert s[0, 0] == s.max() and np.all(s > 0) and np.max(np.abs(s - VO.gaussian_smooth(b))) <= 1e-15


def test_plane_rmse_nothing_qualifies():
    z = np.zeros(3)
    r, e = V.plane_rmse(np.array([1, 0, 0]), z, z, np.array([0, 2, 0]), z, z)
    assert np.isnan(r) and e == []
