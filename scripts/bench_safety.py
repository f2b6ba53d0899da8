#!/usr/bin/env python
"""Time the safety metrics (cvae_amd.safety) on the golden sce1 population.

    python scripts/bench_safety.py [--tiles 1 108] [--reference DIR] [--no-gpu] [--host LABEL] >> profiles/safety/bench.jsonl

Inputs: the 38 recorded sce1 tracks of tests/golden/validate.npz against the sce1 source log of
tests/golden/safety.npz, tiled (P = 38 and P = 4,104).  Per size: ``track_safety`` end to end
(records only) — median of 20 calls after 3 warm-ups, timed with stream events and with the wall
clock, a synchronize on both sides — and the numpy restatement tests/safety_oracle.py on the same
box (all tracks at P = 38; 38 tracks scaled at larger P).  With --reference DIR (a checkout of the
reference; it is not part of this repository) the reference's own pandas path —
``find_best_start_row`` + ``merge_trajectory_into_csv`` + the scenario filter and the three metric
columns — is timed per track on the same inputs.  One JSON line per measurement; every line carries the
``host`` label, so rows taken on different machines stay distinguishable in one file.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "defensive-model-vae_amd"), os.path.join(ROOT, "tests")]


def inputs():
    import safety_checks as sc
    G = np.load(os.path.join(ROOT, "tests", "golden", "validate.npz"))
    f, o = G["sce1/model_flat"], G["sce1/model_offsets"]
    tracks = [np.ascontiguousarray(f[o[i]:o[i + 1]]) for i in range(len(o) - 1)]
    _, _, pairs = sc.load()
    return tracks, sc.log_columns(pairs["sce1_exp1_2"]["log"])


def reference_seconds(ref_dir, tracks, log):
    import pandas as pd
    sys.path[:0] = [os.path.join(ref_dir, "SUT_Testing"), os.path.join(ref_dir, "SUT_Testing", "tools")]
    import Defensive_Testing as DT
    import Metrics_Calculation as M
    df = pd.DataFrame(log)
    name = "StaticBlindTown05"
    t0 = time.perf_counter()
    for t in tracks:
        merged = DT.merge_trajectory_into_csv(df, t, DT.find_best_start_row(df, float(t[0, 0]), float(t[0, 1])))
        try:
            w = M.filter_dataframe_by_scenario(merged, name)
        except ValueError:
            continue
        M.add_jerk_column(M.add_pet_column(M.add_ttc_column(w, name), name), name)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, nargs="+", default=[1, 108])
    ap.add_argument("--reference", default=None)
    ap.add_argument("--no-gpu", action="store_true")
    ap.add_argument("--host", default="unlabelled", help="label of the machine, written into every row")
    a = ap.parse_args()

    def emit(row):
        print(json.dumps(dict(row, host=a.host)), flush=True)

    import safety_oracle as so
    tracks, log = inputs()
    t0 = time.perf_counter()
    for t in tracks:
        so.track_record(log, t, 0)
    t_or = time.perf_counter() - t0
    emit({"what": "oracle_numpy", "P": len(tracks), "seconds": round(t_or, 4),
          "ms_per_track": round(t_or / len(tracks) * 1e3, 3)})
    if a.reference:
        t_ref = reference_seconds(a.reference, tracks, log)
        emit({"what": "reference_pandas", "P": len(tracks), "seconds": round(t_ref, 4),
              "ms_per_track": round(t_ref / len(tracks) * 1e3, 3)})
    if a.no_gpu:
        return
    import torch
    from cvae_amd import safety as S
    L = S.SceneLogs([log], "sce1")
    sync = torch.cuda.synchronize
    for tiles in a.tiles:
        pop = tracks * tiles
        off = np.zeros(len(pop) + 1, np.int64)
        off[1:] = np.cumsum([len(t) for t in pop])
        dev = (torch.from_numpy(np.concatenate(pop)).cuda(), torch.from_numpy(off).cuda())
        lot = np.zeros(len(pop), np.int32)
        for _ in range(3):
            r = S.track_safety(dev, L, lot)
        wall, ev = [], []
        for _ in range(20):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            sync()
            t0 = time.perf_counter()
            e0.record()
            S.track_safety(dev, L, lot)
            e1.record()
            sync()
            wall.append(time.perf_counter() - t0)
            ev.append(e0.elapsed_time(e1))
        emit({"what": "track_safety", "P": len(pop), "track_rows": int(off[-1]), "log_rows": L.n_rows,
              "events_ms_median": round(statistics.median(ev), 3), "events_ms_min": round(min(ev), 3),
              "wall_ms_median": round(statistics.median(wall) * 1e3, 3),
              "oracle_numpy_ms_scaled": round(t_or / len(tracks) * len(pop) * 1e3, 1),
              "window_share": S.summary(r)["window_share"]})


if __name__ == "__main__":
    main()
