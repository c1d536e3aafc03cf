#!/usr/bin/env python3
"""Cost of the time-domain diagnostics (samsim_set_tracks) on the headline ensemble (1 048 576 columns x 80 layers, SHEBA day-200
fixture tiled as bench.py tiles it, 500 warm-up steps).  Three things are recorded, none is a bar:

  sample       the device time of one sample for four SCALAR tracks, four tracks that need the walk, and all eight: K launches of
               ONE step enqueued back to back (samsim_steps_timed, HIP events) with the tracks sampled after every step, minus the
               same K launches without tracks, / K.  Both sequences end every launch the same way, so the difference is the K
               sampling kernels as they run in place, behind their step launches on the two streams.  Beside it the bytes the
               kernel must move (computed from shapes: rows needed x sum(N_active) x 8 for the walk, 8 bytes per scalar, the track
               fields read and written) and the bandwidth that makes.
  tracking_off the 500-step time of `bench.py --gpus 1` without tracks for this library and for the parent commit's
               (--parent-lib), alternating within one job: the step kernel is the parent's, so they must agree within the job's own
               run-to-run spread.
  tracking_on  the 500-step time with the eight tracks at every = 500, 100 and 10: the samples and the extra launch ends (each cut
               makes one more "last step stores everything").

    python tools/track_bench.py --parent-lib samsim_amd/csrc/variants/libsamsim_hip_parent.so > profiles/rN_tracks.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

HBM_ACHIEVABLE_TBS = 6.3    # measured copy bandwidth of the MI355X (8.0 TB/s spec)


def spread(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "runs_ms": ms}


def bench_step_ms(lib, steps, warmup):
    """roofline.mean_launch_ms of one bench.py run in a process of its own, with the library `lib` (None: the product)"""
    env = dict(os.environ)
    env.pop("SAMSIM_HIP_LIB", None)
    if lib:
        env["SAMSIM_HIP_LIB"] = os.path.abspath(lib)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
           "--no-cpu-baseline", "--no-extra"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        sys.exit(f"bench.py failed with {lib or 'the product library'}:\n{r.stdout[-2000:]}{r.stderr[-2000:]}")
    res = json.loads([line for line in r.stdout.splitlines() if line.startswith("{")][-1])
    return res["roofline"]["mean_launch_ms"], res["roofline"]["lib_md5"], res["failed_columns"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncol", type=int, default=1 << 20)
    ap.add_argument("--warmup-steps", type=int, default=500)
    ap.add_argument("--launch", type=int, default=500, help="steps of the launch the overhead is quoted for")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--one-step-launches", type=int, default=50, help="K of the sample-time measurement")
    ap.add_argument("--parent-lib", default=None, help="library of the parent commit for the tracking-off comparison")
    ap.add_argument("--bench-steps", type=int, default=5)
    ap.add_argument("--bench-warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3, help="parent / new alternations of the tracking-off comparison")
    a = ap.parse_args()

    out = {"what": "cost of samsim_set_tracks on one handle; HIP events of samsim_steps_timed", "ncol": a.ncol}
    # ---- tracking off, against the parent: first, each run in a process of its own, before this process opens the GPU
    if a.parent_lib:
        parent, new, md5, failed = [], [], {}, []
        for _ in range(a.rounds):
            for name, lib, into in (("parent", a.parent_lib, parent), ("new", None, new)):
                ms, md5[name], nf = bench_step_ms(lib, a.bench_steps, a.bench_warmup)
                into.append(ms)
                failed.append(nf)
        pm, nm = statistics.median(parent), statistics.median(new)
        out["tracking_off"] = {
            "what": f"roofline.mean_launch_ms of `bench.py --gpus 1 --steps {a.bench_steps} --warmup {a.bench_warmup} --no-cpu-baseline "
                    "--no-extra`, parent and new library alternating within one job (parent, new, ...), no tracks set",
            "parent_ms": parent, "new_ms": new, "parent_lib_md5": md5["parent"], "new_lib_md5": md5["new"], "parent_median": pm,
            "new_median": nm, "ratio_of_medians": nm / pm, "parent_relative_spread": (max(parent) - min(parent)) / pm,
            "new_relative_spread": (max(new) - min(new)) / nm, "failed_columns": failed,
            "within_the_jobs_spread": bool(min(new) <= max(parent) and min(parent) <= max(new))}

    import samsim_amd
    from samsim_amd import testcases as tcs
    from samsim_amd.capi import NTF, TrackSpec
    z, st, clock, pert = bench.load_ensemble("sheba_ensemble_80.npz")
    cfg, _ = tcs.testcase4(1, nlayer=int(z["nlayer"]), n_top=int(z["n_top"]), n_bottom=int(z["n_bottom"]))
    g = samsim_amd.hip_solver(cfg, a.ncol)
    g.set_forcing(*bench.sheba_forcing(), bench.tile(pert[0], a.ncol), bench.tile(pert[1], a.ncol))
    bench.upload_tiled(g, st, a.ncol, 0)
    g.set_clock(**clock)
    g.set_output_window(0, 0)
    g.step(a.warmup_steps)
    g.synchronize()
    na = g.ensemble_stats(["N_active"])["N_active"]
    columns, layer_cells = int(na.count), float(na.mean) * int(na.count)
    out.update(nlayer=int(cfg.nlayer), warmup_steps=a.warmup_steps, failed_columns=a.ncol - columns, sum_n_active=layer_cells,
               device=g.get_device()[1], lib_md5=bench.lib_md5(), hbm_achievable_TBps=HBM_ACHIEVABLE_TBS)

    scalars = [TrackSpec.make("scalar", "T_top", sense=+1, threshold=0.0), TrackSpec.make("scalar", "T_snow", sense=-1, threshold=-0.5),
               TrackSpec.make("scalar", "thick_snow"), TrackSpec.make("n_active")]
    walkers = [TrackSpec.make("ice_thickness"), TrackSpec.make("bulk_salinity"), TrackSpec.make("layer", "T", layer=1),
               TrackSpec.make("layer", "S_bu", layer=-1)]
    # bytes one sample must move: status, n_active and flags (12 per column); per track ten fields read (LAST is only written) and
    # at most eleven written -- the extremes and the condition's fields only where they change, counted here as if always --;
    # 8 per SCALAR value; thick, S_abs and m over the active layers; one value (S_bu: three) per LAYER track
    fixed, per_track = 12.0 * a.ncol, (10 + NTF) * 8.0 * columns
    need = {"four_scalar_tracks": fixed + 4 * per_track + 3 * 8.0 * columns,
            "four_walking_tracks": fixed + 4 * per_track + 3 * 8.0 * layer_cells + 4 * 8.0 * columns}
    need["all_eight"] = need["four_scalar_tracks"] + need["four_walking_tracks"] - fixed
    K = a.one_step_launches
    none = ("without_tracks", None)

    def rounds(configs, every_of, nsteps, nlaunches):
        """{name: [ms, ...]}: a.repeats rounds, each taking the configurations in turn -- the step time drifts with the season as the
        clock moves on, and in turn every configuration sees the same drift"""
        ms = {name: [] for name, _ in configs}
        for _ in range(a.repeats):
            for name, specs in configs:
                g.set_tracks(specs, every_of(name)) if specs else g.set_tracks(None)
                ms[name].append(g.steps_timed(nsteps, nlaunches))
        return ms
    g.steps_timed(1, K)                                        # warm-up of the sequence itself
    configs = [none, ("four_scalar_tracks", scalars), ("four_walking_tracks", walkers), ("all_eight", scalars + walkers)]
    ms = rounds(configs, lambda name: 1, 1, K)
    base = statistics.median(ms["without_tracks"])
    out["sample"] = {"how": f"{K} launches of one step back to back, with the tracks sampled after every step minus without tracks, / {K}; "
                            f"{a.repeats} rounds over the four configurations in turn, medians", "one_step_launches": K,
                     "without_tracks": spread(ms["without_tracks"])}
    for name, specs in configs[1:]:
        t = spread(ms[name])
        one = (t["median_ms"] - base) / K
        t.update(sample_ms=one, bytes_needed=need[name], TBps_needed_bytes=(need[name] / (one * 1e-3) / 1e12) if one > 0 else None)
        out["sample"][name] = t
    slot = samsim_amd.capi.track_slot(0, "N")
    out["sample"]["sampled_columns"] = int(g.ensemble_stats([slot])[slot].count)
    # ---- tracking on: the launch of 500 with the eight tracks at three cadences, against the same handle without tracks
    g.set_tracks(None)
    g.step((-g.get_clock().step) % a.launch)                   # every launch starts at a multiple of its length
    g.steps_timed(a.launch, 1)
    cadences = {f"every_{e}": e for e in (500, 100, 10)}
    ms = rounds([none] + [(name, scalars + walkers) for name in cadences], lambda name: cadences[name], a.launch, 1)
    off = spread(ms["without_tracks"])
    out["tracking_on"] = {"how": f"samsim_steps_timed({a.launch}, 1), {a.repeats} rounds over the four configurations in turn, medians; the "
                                 f"clock is a multiple of {a.launch} at every launch, so every = 500, 100, 10 cut it into 1, 5 and 50 "
                                 "launches, each followed by a sample",
                          "launch_steps": a.launch, "without_tracks": off}
    for name, every in cadences.items():
        t = spread(ms[name])
        t.update(samples_per_launch=a.launch // every, overhead_ms=t["median_ms"] - off["median_ms"],
                 overhead_relative=t["median_ms"] / off["median_ms"] - 1.0)
        out["tracking_on"][name] = t
    out["clock_step_at_the_end"] = int(g.get_clock().step)
    out["failed_columns_at_the_end"] = int((g.get_status()[0] != 0).sum())
    g.close()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
