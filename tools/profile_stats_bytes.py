#!/usr/bin/env python3
"""Do two builds of the library return the same bytes from the four reductions of the layer profiles?  Writes, for eight requests
-- both axes, both origins, one and two passes, two of them grouped -- on the day-345 melt ensemble tiled over 70 001 columns (200
steps, three stopped columns, labels = column mod 9): the profile statistics, the regressions on dT2m and the weighted statistics
(Gauss weight on the ice thickness) of T, S_bu, psi_l and thick, and the joint histograms of T at 40 and at 254 value bins (one
and two passes at 64 depth bins or fewer, two and three at 100) for the library selected by SAMSIM_HIP_LIB; run it once per
build, a process each, and compare the files with --compare.

    SAMSIM_HIP_LIB=.../libsamsim_hip_parent.so python tools/profile_stats_bytes.py --out out/parent.npz
    python tools/profile_stats_bytes.py --out out/new.npz
    python tools/profile_stats_bytes.py --compare out/parent.npz out/new.npz > profiles/rN_profile_stats_bytes.json
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

REQUESTS = [dict(axis="layer", origin="top"), dict(axis="layer", origin="bottom"),
            dict(axis="depth", origin="top", nbins=32, dz=0.07), dict(axis="depth", origin="bottom", nbins=32, z0=0.035, dz=0.07),
            dict(axis="depth", origin="top", nbins=100, dz=0.02), dict(axis="depth", origin="bottom", nbins=100, dz=0.02),
            dict(axis="depth", origin="top", nbins=100, dz=0.02, group=4), dict(axis="layer", origin="bottom", group=7)]
NAMES = ["T", "S_bu", "psi_l", "thick"]
# family -> what it calls; every family serves every request on the same handle
FAMILIES = {"profile_stats": "samsim_get_profile_stats / samsim_get_group_profile_stats",
            "profile_regression": "samsim_get_profile_regression, predictor dT2m",
            "weighted_profile_stats": "samsim_get_weighted_profile_stats after samsim_set_weights(GAUSS on thickness, scale 0.1)",
            "profile_histogram_40": "samsim_get_profile_histogram of T, 40 value bins of 0.5 from -20",
            "profile_histogram_254": "samsim_get_profile_histogram of T, 254 value bins of 0.08 from -20"}


def results(g, family, rq):
    """the bytes one family returns for one request"""
    if family == "profile_stats":
        q = g.profile_stats(NAMES, **rq)
    elif family == "profile_regression":
        q = g.profile_regression(NAMES, "dT2m", **rq)
    elif family == "weighted_profile_stats":
        q = g.weighted_profile_stats(NAMES, **rq)
    else:
        nv, dv = (40, 0.5) if family == "profile_histogram_40" else (254, 0.08)
        h = g.profile_histogram("T", nv, -20.0, dv, **rq)
        assert int(h.sum()) > 0
        return h.tobytes()
    assert max(int(q[n]["count"].max()) for n in NAMES) > 0
    return b"".join(q[n].tobytes() for n in NAMES)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--compare", nargs=2, default=None)
    a = ap.parse_args()
    if a.compare:
        x, y = np.load(a.compare[0]), np.load(a.compare[1])
        out = {"what": "the four reductions of the layer profiles (T, S_bu, psi_l, thick; the histograms T) of two builds of the library, "
                       "a process per library, every request on the same handle; day-345 melt ensemble tiled over 70 001 columns, 200 "
                       "steps, three stopped columns, labels = column mod 9 for the grouped requests; sha256 over the bytes of a "
                       "family's results per request",
               "families": FAMILIES, "parent_lib_md5": str(x["lib_md5"]), "new_lib_md5": str(y["lib_md5"]), "requests": []}
        total, same_all = 0, True
        for i, rq in enumerate(REQUESTS):
            for fam in FAMILIES:
                u, v = x[f"{fam}{i}"].tobytes(), y[f"{fam}{i}"].tobytes()
                total += len(u)
                same_all = same_all and u == v
                out["requests"].append({"family": fam, "request": rq, "parent_sha256": hashlib.sha256(u).hexdigest(),
                                        "new_sha256": hashlib.sha256(v).hexdigest(), "same_bytes": u == v})
        out["bytes_compared"], out["all_bytes_identical"] = total, bool(same_all)
        print(json.dumps(out, indent=1))
        sys.exit(0 if same_all else 1)
    import samsim_amd
    from samsim_amd import testcases as tcs
    from samsim_amd.capi import State
    ncol = 70001
    z, st, clock, pert = bench.load_ensemble("sheba_ensemble_80_day345.npz")
    cfg, _ = tcs.testcase4(1, nlayer=int(z["nlayer"]), n_top=int(z["n_top"]), n_bottom=int(z["n_bottom"]))
    full = State(bench.tile(st.lay, ncol), bench.tile(st.scal, ncol), bench.tile(st.n_active, ncol).astype(np.int32))
    for c in (5, 40000, 70000):
        full.arr("H_abs")[0, c] = -1.0e15            # getT cannot converge -> STOP 99
    g = samsim_amd.hip_solver(cfg, ncol)
    g.set_forcing(*bench.sheba_forcing(), bench.tile(pert[0], ncol), bench.tile(pert[1], ncol))
    g.set_state(full)
    g.set_clock(**clock)
    g.set_output_window(0, 0)
    g.step(200)
    assert (g.get_status()[0] != 0).sum() == 3
    g.set_groups((np.arange(ncol) % 9).astype(np.int32), ngroups=9)
    assert g.set_weights("thickness", "gauss", 0.1)["n_pos"] > 0
    res = {"lib_md5": bench.lib_md5()}
    for i, rq in enumerate(REQUESTS):
        for fam in FAMILIES:
            res[f"{fam}{i}"] = np.frombuffer(results(g, fam, rq), dtype=np.uint8)
    np.savez(a.out, **res)
    print(json.dumps({"lib_md5": res["lib_md5"], "out": a.out, "bytes": int(sum(v.size for k, v in res.items() if k != "lib_md5"))}))


if __name__ == "__main__":
    main()
