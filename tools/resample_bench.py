#!/usr/bin/env python3
"""Cost of the posterior draw on the headline ensemble (1 048 576 columns x 80 layers, SHEBA day-200 fixture tiled as bench.py tiles
it, 500 warm-up steps, the twin-experiment GAUSS row of tools/weights_bench.py).  Nothing here is a bar; the record says what the
call costs beside the calls it resembles, host wall clock around the blocking call (the launches and the synchronisation
included), medians of --repeats calls with min and max:

  resample_<kind>_<m>      samsim_resample, m = 4 096, 262 144 and 1 048 576, both kinds
  resample_degenerate_<m>  ... on a GAUSS row whose scale leaves one member at 1.0 and every other at 0.0: one column takes every draw
  get_ancestors            the whole ancestor list of the largest draw to the host; get_offspring the whole offspring row
  weighted_histogram_64    samsim_get_weighted_histogram of the thickness: the same 64-step lane order per block, once
  select_262144            samsim_select_columns returning 262 144 indices: the same three-launch pattern
  get_weights, get_state   what finding the ancestors cost before: the row to the host, and the survivors' state

    python tools/resample_bench.py > profiles/rN_resample.json
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from tools.functional_bench import timed  # noqa: E402

DRAWS = (4096, 262144, 1048576)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncol", type=int, default=1 << 20)
    ap.add_argument("--warmup-steps", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--no-get-state", action="store_true", help="leave out the download of the whole handle")
    a = ap.parse_args()

    import samsim_amd
    from samsim_amd import capi, testcases as tcs
    from samsim_amd.capi import SensorSpec, score_slot
    mk = SensorSpec.make
    z, st, clock, pert = bench.load_ensemble("sheba_ensemble_80.npz")
    cfg, _ = tcs.testcase4(1, nlayer=int(z["nlayer"]), n_top=int(z["n_top"]), n_bottom=int(z["n_bottom"]))
    g = samsim_amd.hip_solver(cfg, a.ncol)
    g.set_forcing(*bench.sheba_forcing(), bench.tile(pert[0], a.ncol), bench.tile(pert[1], a.ncol))
    bench.upload_tiled(g, st, a.ncol, 0)
    g.set_clock(**clock)
    g.set_output_window(0, 0)
    g.step(a.warmup_steps)
    g.synchronize()
    status = g.get_status()[0]
    out = {"what": "cost of samsim_resample beside the calls it resembles on one handle; host wall clock around the blocking calls",
           "ncol": a.ncol, "nlayer": int(cfg.nlayer), "warmup_steps": a.warmup_steps, "repeats": a.repeats, "device": g.get_device()[1],
           "lib_md5": bench.lib_md5(), "failed_columns": int((status != 0).sum())}

    # the twin experiment of tools/weights_bench.py: the observations are one member's values
    buoy = [mk("profile", "T", 0.1 * i, interp="linear") for i in range(16)] + [mk("ice_thickness"), mk("scalar", "thick_snow")]
    member = int(np.flatnonzero(status == 0)[a.ncol // 3 % max(1, int((status == 0).sum()))])
    g.set_sensors(buoy)
    g.score(g.sensor_values([member])[:, 0])
    J = score_slot("J_SUM")
    q = g.ensemble_stats([J])[J]
    scale = max(q.mean, 1e-3) / 2.0                         # tempered: the mean member keeps exp(-1) of the best member's weight

    def note(label, t, **more):
        t.update(more)
        out[label] = t
        print(label, t["median_ms"], "ms", file=sys.stderr, flush=True)

    winfo = g.set_weights(J, "gauss", scale)
    out["weights"] = dict(winfo, scale=scale)
    assert winfo["n_pos"] >= 2
    for m in DRAWS:
        for kind, kw in (("systematic", dict(u0=0.37)), ("stratified", dict(seed=2026))):
            t, info = timed(lambda: g.resample(m, kind, **kw), a.repeats)
            assert info["m_drawn"] == m
            note(f"resample_{kind}_{m}", t, info=info)
    t, anc = timed(lambda: g.ancestors(), 3)
    assert anc.size == DRAWS[-1] and (np.diff(anc) >= 0).all()
    note("get_ancestors", t, bytes_returned=int(anc.nbytes))
    t, N = timed(lambda: g.offspring(), 3)
    assert N.sum() == DRAWS[-1] and np.array_equal(np.bincount(anc, minlength=a.ncol), N.astype(np.int64))
    note("get_offspring", t, bytes_returned=int(N.nbytes))
    del anc, N

    th = g.ensemble_stats(["thickness"])["thickness"]
    v0, dv = th.min, (th.max - th.min) * 1.001 / 64
    t, wh = timed(lambda: g.weighted_histogram("thickness", 64, v0, dv), a.repeats)
    note("weighted_histogram_64", t, sum=float(wh.sum()))
    # the thickness bound that 262 144 running columns pass
    n_sel = min(262144, th.count)
    t, (idx, n_match) = timed(lambda: g.select([("thickness", -1e300, 1e300)], max_out=n_sel), a.repeats)
    assert idx.size == n_sel
    note("select_262144", t, returned=int(idx.size), n_match=int(n_match))
    t, w = timed(lambda: g.weights(), 3)
    note("get_weights", t, bytes_returned=int(w.nbytes))
    del w

    # the degenerate posterior: the best member at 1.0, every other beyond the cut-off of the exponential.  The members are tiled,
    # so the best misfit is shared by every copy of a member: one column's melt_err diagnostic is put far below the others'
    # instead, and the GAUSS row is formed from that scalar
    one = g.get_state(member, 1)
    one.scal[capi.S["melt_err"]] = -1.0e30
    g.set_state(one, member)
    dinfo = g.set_weights("melt_err", "gauss", 1.0)
    assert dinfo["n_pos"] == 1 and dinfo["sum_w"] == 1.0
    out["weights_degenerate"] = dinfo
    for m in DRAWS:
        t, info = timed(lambda: g.resample(m, "systematic", u0=0.37), a.repeats)
        note(f"resample_degenerate_{m}", t, info=info)
        out[f"degenerate_over_spread_{m}"] = t["median_ms"] / out[f"resample_systematic_{m}"]["median_ms"]

    if not a.no_get_state:
        whole_t, whole = timed(lambda: g.get_state(), 2)
        whole_t.update(columns=a.ncol, bytes_returned=whole.lay.nbytes + whole.scal.nbytes + whole.n_active.nbytes)
        del whole
        out["get_state_whole_handle"] = whole_t
    both = out["weighted_histogram_64"]["median_ms"] + out["select_262144"]["median_ms"]
    out["histogram_plus_select_ms"] = both
    for m in DRAWS:
        out[f"resample_systematic_{m}_over_histogram_plus_select"] = out[f"resample_systematic_{m}"]["median_ms"] / both
    g.close()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
