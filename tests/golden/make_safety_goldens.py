"""Fixtures for the safety-metric tests (run where the reference checkout exists):

    python tests/golden/make_safety_goldens.py /path/to/reference

The reference's own ``SUT_Testing/Defensive_Testing.py`` and ``SUT_Testing/tools/Metrics_Calculation.py``
are imported read-only and run on

(a) recorded logs of ``SUT_Testing/collected_data`` (``LOGS``): at least one per scenario, with and
    without ``sim_time``, and ``BEHAVIOR_UnpredictableMovementTown04`` for which the reference raises
    "no start row";
(b) the track / log pairs the reference ships a ``*_def.csv`` for (``PAIRS``):
    ``results/GeneratedData/tracked_trajectory_sce*_exp*_*.npy`` merged into their ``DefensiveData``
    log with ``find_best_start_row`` + ``merge_trajectory_into_csv``, then scored.

Recorded per case: the 20 needed columns of the log as ``pd.read_csv`` parses them (a missing column
is absent), the window bounds (the two ``_first_index`` calls of the scenario's filter are
observed), the ``TTC`` / ``PET`` / ``JERK`` columns of ``compute_metric_from_csv`` and the statistics
of ``main()`` — its body is run as written with only the four selection lines (model, scenario,
test_run, metric) replaced, ``pd.read_csv`` answering with the frame under test, and the frames it
hands to ``_sub_valid_for_metric`` observed; for (b) also the track, the start row and the seven
merged ego columns from the start row on (before it the merged log is the source log).  Data only,
one compressed .npz.
"""
import contextlib
import inspect
import io
import json
import os
import re
import sys

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("CVAE_REFERENCE", ""))
sys.path[:0] = [os.path.join(REF, "SUT_Testing"), os.path.join(REF, "SUT_Testing", "tools")]
sys.path.insert(0, os.path.join(HERE, "..", "..", "defensive-model-vae_amd"))
import Defensive_Testing as DT  # noqa: E402  (the reference, imported read-only)
import Metrics_Calculation as M  # noqa: E402
from cvae_amd.safety import COLUMNS, EGO_COLUMNS, SCENARIOS  # noqa: E402

LOGS = ("DEF_StaticBlindTown05_1", "IDM_DynamicBlindTown05_1",
        "DEF_PredictableMovementTown05_1", "IDM_UnpredictableMovementTown04_1",
        "BEHAVIOR_UnpredictableMovementTown04")
PAIRS = ("sce1_exp1_2", "sce1_exp26_2", "sce2_exp12_2", "sce3_exp8_2", "sce4_exp13_2")

_calls = []
_orig_first = M._first_index
M._first_index = lambda mask: (_calls.append(_orig_first(mask)), _calls[-1])[1]
_subs = []
_orig_sub_valid = M._sub_valid_for_metric


def _sub_valid(sub, metric):
    out = _orig_sub_valid(sub, metric)
    _subs.append((len(sub), out))
    return out


class _Pandas:
    """pandas, with read_csv answering with the frame under test"""
    frame = None

    def __getattr__(self, k):
        return getattr(pd, k)

    def read_csv(self, *a, **k):
        return self.frame.copy()


M.pd = _Pandas()
M.resolve_csv_path = lambda *a, **k: "frame-under-test"


def run_main(df, scenario, metric):
    """main() as written, on df: returns (n_sub, sub_valid) or None when it raises "no start row" """
    src = inspect.getsource(M.main)
    for name, value in (("model", "'X'"), ("scenario", repr(scenario)), ("test_run", "None"),
                        ("metric", repr(metric))):
        src, n = re.subn(rf"^(\s*){name}(: [^=]+)? = .*$", rf"\g<1>{name} = {value}", src, count=1, flags=re.M)
        assert n == 1, name
    ns = dict(M.__dict__)
    ns["_sub_valid_for_metric"] = _sub_valid
    exec(src, ns)
    M.pd.frame = df
    del _subs[:]
    with contextlib.redirect_stdout(io.StringIO()):
        ns["main"]()
    assert len(_subs) == 1
    return _subs[0]


def score(df, scenario, out, key):
    """everything the reference computes for df, into out under key/…; returns the meta entry"""
    meta = {"scenario": scenario, "scene": [s["name"] for s in SCENARIOS].index(scenario),
            "has_time": "sim_time" in df.columns, "n_rows": len(df), "columns": [c for c in COLUMNS if c in df.columns]}
    out[key + "/cols"] = np.stack([df[c].to_numpy(dtype=np.float64) for c in meta["columns"]])
    M.pd.frame = df
    del _calls[:]
    try:
        cols = {m: M.compute_metric_from_csv("X", scenario, None, metric=m) for m in ("TTC", "PET", "JERK")}
    except ValueError as e:
        meta.update(status=1, error=str(e))
        return meta
    i0, i1 = _calls[0], _calls[1]
    meta.update(status=0, i0=int(i0), i1=-1 if i1 is None else int(i0 + i1), n_window=len(cols["TTC"]))
    for m in ("TTC", "PET", "JERK"):
        out[f"{key}/{m}"] = cols[m][m].to_numpy(dtype=np.float64)
    stats = {}
    for m in ("TTC", "PET", "JERK"):
        n_sub, sv = run_main(df, scenario, m)
        v = sv[m].abs() if m == "JERK" else sv[m]
        stats[m] = {"count": len(sv), "mean": float(v.mean()) if len(sv) else None,
                    "ext": float(v.max() if m == "JERK" else v.min()) if len(sv) else None}
        if m == "TTC":
            col, how = SCENARIOS[meta["scene"]]["decel"]
            stats["n_sub"] = n_sub
            stats["decel"] = float(getattr(sv[col], how)()) if len(sv) else None
            stats["yaw_max"] = float(sv["ego_yaw"].max()) if len(sv) else None
    meta["stats"] = stats
    return meta


def main():
    out, meta = {}, {"logs": {}, "pairs": {}}
    for name in LOGS:
        df = pd.read_csv(os.path.join(REF, "SUT_Testing", "collected_data", name + ".csv"))
        _, scenario, _ = M.parse_filename(name)
        meta["logs"][name] = score(df, scenario, out, "a/" + name)
    for name in PAIRS:
        npy = os.path.join(REF, "results", "GeneratedData", f"tracked_trajectory_{name}.npy")
        sce, exp, suffix = DT.parse_tracked_npy_name(npy)
        csv = DT.find_csv_under_defensive_data(__import__("pathlib").Path(REF) / "DefensiveData",
                                               DT.expected_csv_name(sce, exp, suffix))
        df = pd.read_csv(csv)
        traj = DT.parse_tracked_npy_state(np.asarray(np.load(npy)))
        start = DT.find_best_start_row(df, float(traj[0, 0]), float(traj[0, 1]))
        merged = DT.merge_trajectory_into_csv(df, traj, start)
        key = "b/" + name
        m = score(merged, DT.SCE_TO_TOWN[sce], out, key)
        # the source log replaces the merged one as the recorded input; the merged ego columns are the expectation
        m["n_rows"] = len(df)
        out[key + "/cols"] = np.stack([df[c].to_numpy(dtype=np.float64) for c in m["columns"]])
        out[key + "/track"] = traj
        out[key + "/merged"] = np.stack([merged[c].to_numpy(dtype=np.float64)[start:] for c in EGO_COLUMNS])
        m.update(start=int(start), L=int(len(merged) - start), source=os.path.basename(str(csv)))
        meta["pairs"][name] = m
    out["meta"] = np.array(json.dumps(meta))
    path = os.path.join(HERE, "safety.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    for k, v in {**meta["logs"], **meta["pairs"]}.items():
        print(k, {a: b for a, b in v.items() if a not in ("columns",)})


if __name__ == "__main__":
    main()
