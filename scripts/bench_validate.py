#!/usr/bin/env python
"""Time the validation metrics (cvae_amd.validate) on the golden sce1 population.

    python scripts/bench_validate.py [--tiles 1 108] [--checkpoint MODEL.pth] > profiles/validate/bench.jsonl

Per population size (the 38 golden tracks tiled: P = 38 and P = 4,104 >= 4,096): the device time of
``metrics`` (median of 20 calls after 3 warm-ups, a synchronize on both sides; the human side is
cached after the first call, as in a sweep over checkpoints), the time of its two passes alone, and
the numpy restatement tests/validate_oracle.py on the same box.  The reference's own per-metric CPU
time comes from the golden's metadata (38 tracks).  With --checkpoint, ``validate_checkpoint`` split
by stage.  One JSON line per measurement.
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


def timed(fn, sync, n=20, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(n):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, nargs="+", default=[1, 108])
    ap.add_argument("--checkpoint", default=None)
    a = ap.parse_args()
    import torch
    import validate_oracle as VO
    from cvae_amd import validate as V
    G = np.load(os.path.join(ROOT, "tests", "golden", "validate.npz"))
    meta = json.loads(bytes(G["meta"]).decode())
    split = lambda f, o: [f[o[i]:o[i + 1]] for i in range(len(o) - 1)]  # noqa: E731
    model = split(G["sce1/model_flat"], G["sce1/model_offsets"])
    human = split(G["sce1/human_flat"], G["sce1/human_offsets"])
    sec = meta["sce1"]["seconds"]
    print(json.dumps({"what": "reference_cpu_seconds_38_tracks", "per_metric": sec,
                      "one_pass": round(sec["m1"] + sec["m2_g0.5"] + sec["m3_g0.5"] + sec["m4_x"] + sec["m5_5.0"], 4)}))
    sync = torch.cuda.synchronize
    ref = V.HumanReference(human, "sce1")
    for tiles in a.tiles:
        pop = model * tiles
        _, flat, off = V._ragged(pop, 4)
        states = torch.from_numpy(flat).cuda()
        tracks = (states, torch.from_numpy(off).cuda())
        med, best = timed(lambda: V.metrics(tracks, ref), sync)
        m = V._model_population(tracks, ref)
        r = V.metrics(tracks, ref)
        e = [r[k] for k in ("v_edges", "x_edges", "y_edges", "coord_edges", "time_edges", "slice_edges")]
        t_rng, _ = timed(lambda: V._model_population(tracks, ref), sync)
        t_acc, _ = timed(lambda: m.accumulate("x", *e), sync)
        t0 = time.perf_counter()
        VO.metrics(pop, human, "sce1", 0.5, "x", 5.0)
        t_or = time.perf_counter() - t0
        print(json.dumps({"what": "metrics", "P": len(pop), "points": int(off[-1]), "metrics_ms_median": round(med * 1e3, 3),
                          "metrics_ms_min": round(best * 1e3, 3), "ranges_pass_ms": round(t_rng * 1e3, 3),
                          "accumulate_pass_ms": round(t_acc * 1e3, 3), "oracle_numpy_ms": round(t_or * 1e3, 1),
                          "threads": torch.get_num_threads()}), flush=True)
    if a.checkpoint:
        start = np.column_stack([np.array([m[0, 0] for m in model]), np.array([m[0, 1] for m in model]),
                                 np.array([m[0, 2] for m in model]), np.zeros(len(model)),
                                 np.array([m[0, 3] for m in model])])
        tm = {}
        V.validate_checkpoint(a.checkpoint, start, ref, timings=tm)
        print(json.dumps({"what": "validate_checkpoint", "P": len(start), "seconds": tm}))


if __name__ == "__main__":
    main()
