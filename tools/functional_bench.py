#!/usr/bin/env python3
"""Cost of the column functionals on the headline ensemble (1 048 576 columns x 80 layers, SHEBA day-200 fixture tiled as bench.py
tiles it, 500 warm-up steps).  Nothing here is a bar; the record says what the calls cost, host wall clock around the blocking call
(the launch, the copy back and the synchronisation included), medians of --repeats calls:

  evaluate_permeable   samsim_set_functionals (which marks the rows stale) is outside the clock; inside it samsim_get_functionals of
                       a one-column window, so the evaluation of the whole handle and eight bytes of copy: one functional,
                       THICKNESS_WHERE psi_l >= 0.05 over the whole column (reads thick and psi_l)
  evaluate_eight       the same with eight functionals over four arrays (psi_l, T, S_abs and m for S_bu, ray: a thick-only pre-pass and two walks)
  read_clean           samsim_get_functionals of the one-column window with the rows current: the fixed cost of the call
  histogram_stale      samsim_get_histogram of the permeable thickness with the rows stale: evaluation + histogram
  histogram_clean      the same with the rows current
  get_state            the whole handle, beside them

Beside each evaluation the bytes its walks must read and the bandwidth that makes.

    python tools/functional_bench.py > profiles/rN_functionals.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def spread(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "runs_ms": ms}


def timed(f, repeats, before=None):
    ms, out = [], None
    for _ in range(repeats):
        if before:
            before()
        t0 = time.perf_counter()
        out = f()
        ms.append((time.perf_counter() - t0) * 1e3)
    return spread(ms), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncol", type=int, default=1 << 20)
    ap.add_argument("--warmup-steps", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=9)
    a = ap.parse_args()

    import samsim_amd
    from samsim_amd import testcases as tcs
    from samsim_amd.capi import FunctionalSpec, func_slot
    mk = FunctionalSpec.make
    z, st, clock, pert = bench.load_ensemble("sheba_ensemble_80.npz")
    cfg, _ = tcs.testcase4(1, nlayer=int(z["nlayer"]), n_top=int(z["n_top"]), n_bottom=int(z["n_bottom"]))
    g = samsim_amd.hip_solver(cfg, a.ncol)
    g.set_forcing(*bench.sheba_forcing(), bench.tile(pert[0], a.ncol), bench.tile(pert[1], a.ncol))
    bench.upload_tiled(g, st, a.ncol, 0)
    g.set_clock(**clock)
    g.set_output_window(0, 0)
    g.step(a.warmup_steps)
    g.synchronize()
    N = int(cfg.nlayer)
    status = g.get_status()[0]
    out = {"what": "cost of the column functionals on one handle; host wall clock around the blocking calls",
           "ncol": a.ncol, "nlayer": N, "warmup_steps": a.warmup_steps, "repeats": a.repeats, "device": g.get_device()[1],
           "lib_md5": bench.lib_md5(), "failed_columns": int((status != 0).sum())}
    na = g.ensemble_stats(["N_active"])["N_active"]
    out["n_active"] = {"mean": na.mean, "min": na.min, "max": na.max}
    # a wave reads whole 512-byte rows up to its largest n_active; the mean over the columns is the lower bound quoted here
    row_bytes = 8.0 * a.ncol * na.mean

    permeable = [mk("thickness_where", "psi_l", sense=1, threshold=0.05)]
    eight = [mk("thickness_where", "psi_l", sense=1, threshold=0.05),
             mk("crossing_depth", "psi_l", sense=1, threshold=0.05, missing=-1.0),
             mk("crossing_depth", "T", sense=1, threshold=-5.0, missing=-1.0),
             mk("min", "T", missing=0.0),
             mk("mean", "S_bu", z_hi=0.5, missing=-1.0),
             mk("integral", "psi_l"),
             mk("max", "ray", missing=-1.0),
             mk("depth_of_max", "ray", "bottom", missing=-1.0)]
    for label, specs, rows in (("evaluate_permeable", permeable, 2), ("evaluate_eight", eight, 1 + 5 + 2)):
        # rows per layer: thick + psi_l; and the pre-pass over thick, a walk over thick, psi_l, T, S_abs and m, a walk over thick and ray
        t, v = timed(lambda: g.functionals(0, 0, 1), a.repeats, before=lambda: g.set_functionals(specs))
        t.update(functionals=len(specs), layer_rows_read=rows, bytes_read=rows * row_bytes,
                 TBps=rows * row_bytes / (t["median_ms"] * 1e-3) / 1e12, value_of_column_0=float(v[0]))
        out[label] = t
        print(label, t["median_ms"], "ms", file=sys.stderr, flush=True)
    g.set_functionals(permeable)
    g.functionals(0, 0, 1)
    out["read_clean"], _ = timed(lambda: g.functionals(0, 0, 1), a.repeats)
    q = g.ensemble_stats([func_slot(0)])[func_slot(0)]
    out["permeable_thickness"] = {"count": q.count, "mean": q.mean, "min": q.min, "max": q.max, "std": q.std}
    nv, v0, dv = 50, 0.0, max(q.max, 1e-3) / 49.0
    out["histogram_stale"], h = timed(lambda: g.histogram(func_slot(0), nv, v0, dv), a.repeats, before=lambda: g.set_functionals(permeable))
    out["histogram_clean"], h2 = timed(lambda: g.histogram(func_slot(0), nv, v0, dv), a.repeats)
    assert (h == h2).all() and int(h.sum()) == q.count
    out["histogram_counts"] = [int(x) for x in h]
    full, whole = timed(lambda: g.get_state(), 2)
    full.update(columns=a.ncol, bytes_returned=whole.lay.nbytes + whole.scal.nbytes + whole.n_active.nbytes)
    del whole
    out["get_state_whole_handle"] = full
    out["get_state_over_evaluate_permeable"] = full["median_ms"] / out["evaluate_permeable"]["median_ms"]
    g.close()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
