#!/usr/bin/env python3
"""Cost of samsim_select_columns and samsim_get_columns on the headline ensemble (1 048 576 columns x 80 layers, SHEBA day-200
fixture tiled as bench.py tiles it, 500 warm-up steps).  Nothing here is a bar; the record says what the calls cost, host wall clock
around the blocking call (launches, the copy back and the synchronisation included), medians of --repeats calls:

  select        one term and four terms, matching a narrow bracket round the median of m_snow (aimed at 0.1 % of the running columns;
                on an ensemble of 256 tiled members it holds the copies of one, 0.39 %) and matching all of them, with max_out =
                SAMSIM_SELECT_MAX_OUT and counting only (max_out = 0); beside it the bytes the predicate must read (8 per term, 4 of
                status) and the bandwidth that makes
  get_columns   100, 10 000 and 262 144 scattered columns (a random permutation's head), all fifteen arrays; the bytes returned, the
                bytes the device reads for them (every 8-byte element is its own 64-byte request in the blocked layout: the
                overfetch is eight) and the time per column
  get_state     the whole handle, beside them, and a quarter of it (the first 262 144 columns, one window)
  ensemble_stats  samsim_get_ensemble_stats of one slot, beside them
  step          with --parent-lib: `bench.py --gpus 1` for the parent commit's library and this one, alternating in one job (the
                step kernel and its headers are the parent's, so the two must agree within the parent's own spread); written to
                --bench-out

    python tools/select_bench.py --parent-lib samsim_amd/csrc/variants/libsamsim_hip_parent.so --bench-out profiles/rN_bench.json \\
        > profiles/rN_select.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

HBM_ACHIEVABLE_TBS = 6.3    # measured copy bandwidth of the MI355X (8.0 TB/s spec)


def spread(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "runs_ms": ms}


def timed(f, repeats):
    ms, out = [], None
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = f()
        ms.append((time.perf_counter() - t0) * 1e3)
    return spread(ms), out


def bench_line(lib, steps, warmup):
    """the JSON line of one bench.py run in a process of its own, with the library `lib` (None: the product)"""
    env = dict(os.environ)
    env.pop("SAMSIM_HIP_LIB", None)
    if lib:
        env["SAMSIM_HIP_LIB"] = os.path.abspath(lib)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
           "--no-cpu-baseline", "--no-extra"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=1100)
    if r.returncode != 0:
        sys.exit(f"bench.py failed with {lib or 'the product library'}:\n{r.stdout[-2000:]}{r.stderr[-2000:]}")
    return json.loads([line for line in r.stdout.splitlines() if line.startswith("{")][-1])


def step_ab(a):
    parent, new, lines = [], [], {}
    for _ in range(a.rounds):
        for name, lib, into in (("parent", a.parent_lib, parent), ("new", None, new)):
            lines[name] = bench_line(lib, a.bench_steps, a.bench_warmup)
            into.append(lines[name]["roofline"]["mean_launch_ms"])
            print(name, into[-1], "ms", file=sys.stderr, flush=True)
    pm, nm = statistics.median(parent), statistics.median(new)
    return {"what": f"roofline.mean_launch_ms of `bench.py --gpus 1 --steps {a.bench_steps} --warmup {a.bench_warmup} --no-cpu-baseline "
                    "--no-extra`, parent and new library alternating within one job (parent, new, ...)",
            "parent_ms": parent, "new_ms": new, "parent_lib_md5": lines["parent"]["roofline"]["lib_md5"],
            "new_lib_md5": lines["new"]["roofline"]["lib_md5"], "parent_median": pm, "new_median": nm, "ratio_of_medians": nm / pm,
            "parent_relative_spread": (max(parent) - min(parent)) / pm, "new_relative_spread": (max(new) - min(new)) / nm,
            "failed_columns": [lines["parent"]["failed_columns"], lines["new"]["failed_columns"]],
            "within_the_parents_spread": bool(min(new) <= max(parent) and min(parent) <= max(new)),
            "new_line": lines["new"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncol", type=int, default=1 << 20)
    ap.add_argument("--warmup-steps", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--parent-lib", default=None, help="library of the parent commit for the comparison of the step")
    ap.add_argument("--bench-out", default=None, help="where the comparison of the step is written")
    ap.add_argument("--bench-steps", type=int, default=10)
    ap.add_argument("--bench-warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3, help="parent / new alternations of the comparison of the step")
    a = ap.parse_args()

    # ---- the step against the parent: first, each run in a process of its own, before this process opens the GPU
    if a.parent_lib:
        ab = step_ab(a)
        if a.bench_out:
            with open(a.bench_out, "w") as f:
                json.dump(ab, f, indent=1)
                f.write("\n")

    import samsim_amd
    from samsim_amd import testcases as tcs
    from samsim_amd.capi import NARR, NSCAL, SELECT_MAX_OUT
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
    out = {"what": "cost of samsim_select_columns and samsim_get_columns on one handle; host wall clock around the blocking calls",
           "ncol": a.ncol, "nlayer": N, "warmup_steps": a.warmup_steps, "repeats": a.repeats, "device": g.get_device()[1],
           "lib_md5": bench.lib_md5(), "hbm_achievable_TBps": HBM_ACHIEVABLE_TBS}

    # ---- select: brackets from the values themselves
    names = ["m_snow", "T_top", "thick_snow", "T_snow"]
    scal = g.get_state(narr=4).scal
    status = g.get_status()[0]
    ok = status == 0
    out["failed_columns"] = int((~ok).sum())
    inf = float("inf")
    everything = [(n, -inf, inf) for n in names]
    x = scal[samsim_amd.capi.S["m_snow"]][ok]
    lo, hi = (float(q) for q in np.quantile(x, [0.4995, 0.5005]))
    rare = [("m_snow", lo, hi)] + everything[1:]
    out["select"] = {"how": "Solver.select; `rare` brackets m_snow between its 49.95 % and 50.05 % quantiles, `all` is [-inf, +inf) on "
                            "every term; count_only is max_out = 0", "terms": names}
    for label, terms in (("one_term_rare", rare[:1]), ("four_terms_rare", rare), ("one_term_all", everything[:1]),
                         ("four_terms_all", everything)):
        t, (idx, n) = timed(lambda: g.select(terms), a.repeats)
        c, _ = timed(lambda: g.select(terms, max_out=0), a.repeats)
        need = a.ncol * (4.0 + 8.0 * len(terms))
        t.update(n_match=int(n), indices_returned=int(idx.size), count_only=c, bytes_read=need,
                 TBps_count_only=need / (c["median_ms"] * 1e-3) / 1e12)
        out["select"][label] = t
        print(label, t["median_ms"], "ms", file=sys.stderr, flush=True)
    t, stats = timed(lambda: g.ensemble_stats(["m_snow"]), a.repeats)
    t["count"] = int(stats["m_snow"].count)
    out["ensemble_stats_one_slot"] = t

    # ---- get_columns against get_state
    rng = np.random.default_rng(14)
    perm = rng.permutation(a.ncol).astype(np.int64)
    out["get_columns"] = {"how": "Solver.get_columns of the head of a random permutation of the columns, all fifteen arrays; "
                                 "device_bytes_read counts a 64-byte request per 8-byte element of the layer block (the blocked layout "
                                 "[block][layer][array][64 lanes] puts the neighbours of an element in other columns)",
                          "overfetch_of_the_blocked_layout": 8.0}
    for n in (100, 10000, SELECT_MAX_OUT):
        cols = perm[:n]
        t, got = timed(lambda: g.get_columns(cols), a.repeats if n < SELECT_MAX_OUT else max(3, a.repeats // 2))
        ret = got.lay.nbytes + got.scal.nbytes + got.n_active.nbytes
        t.update(columns=n, bytes_returned=ret, device_bytes_read=8.0 * got.lay.nbytes + 64.0 * NSCAL * n,
                 us_per_column=t["median_ms"] * 1e3 / n, GBps_returned=ret / (t["median_ms"] * 1e-3) / 1e9)
        out["get_columns"][f"{n}_columns"] = t
        print("get_columns", n, t["median_ms"], "ms", file=sys.stderr, flush=True)
        del got
    full, whole = timed(lambda: g.get_state(), 2)
    full.update(columns=a.ncol, bytes_returned=whole.lay.nbytes + whole.scal.nbytes + whole.n_active.nbytes)
    full["GBps_returned"] = full["bytes_returned"] / (full["median_ms"] * 1e-3) / 1e9
    del whole
    quarter, part = timed(lambda: g.get_state(0, SELECT_MAX_OUT), 3)
    quarter.update(columns=SELECT_MAX_OUT, bytes_returned=part.lay.nbytes + part.scal.nbytes + part.n_active.nbytes)
    del part
    out["get_state_whole_handle"] = full
    out["get_state_window_of_262144"] = quarter
    big = out["get_columns"][f"{SELECT_MAX_OUT}_columns"]["median_ms"]
    out["get_columns_262144_over_a_quarter_of_get_state"] = big / (full["median_ms"] * SELECT_MAX_OUT / a.ncol)
    out["get_columns_262144_over_get_state_of_a_262144_window"] = big / quarter["median_ms"]
    out["narr"] = NARR
    g.close()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
