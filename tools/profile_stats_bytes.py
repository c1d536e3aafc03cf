#!/usr/bin/env python3
"""Do two builds of the library return the same bytes from the profile statistics?  Writes profile_stats_raw (T, S_bu, psi_l, thick)
of eight requests -- both axes, both origins, one and two passes, two of them grouped -- on the day-345 melt ensemble tiled over
70 001 columns (200 steps, three stopped columns, labels = column mod 9) for the library selected by SAMSIM_HIP_LIB; run it once
per build, a process each, and compare the files with --compare.

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--compare", nargs=2, default=None)
    a = ap.parse_args()
    if a.compare:
        x, y = np.load(a.compare[0]), np.load(a.compare[1])
        out = {"what": "samsim_get_profile_stats / samsim_get_group_profile_stats (profile_stats_raw: T, S_bu, psi_l, thick) of two builds "
                       "of the library, a process per library; day-345 melt ensemble tiled over 70 001 columns, 200 steps, three stopped "
                       "columns, labels = column mod 9 for the grouped requests; sha256 over the bytes of the four arrays' results per request",
               "parent_lib_md5": str(x["lib_md5"]), "new_lib_md5": str(y["lib_md5"]), "requests": []}
        total, same_all = 0, True
        for i, rq in enumerate(REQUESTS):
            u, v = x[f"r{i}"].tobytes(), y[f"r{i}"].tobytes()
            total += len(u)
            same_all = same_all and u == v
            out["requests"].append({"request": rq, "parent_sha256": hashlib.sha256(u).hexdigest(), "new_sha256": hashlib.sha256(v).hexdigest(),
                                    "same_bytes": u == v})
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
    res = {"lib_md5": bench.lib_md5()}
    for i, rq in enumerate(REQUESTS):
        q = g.profile_stats(NAMES, **rq)
        assert max(int(q[n]["count"].max()) for n in NAMES) > 0
        res[f"r{i}"] = np.frombuffer(b"".join(q[n].tobytes() for n in NAMES), dtype=np.uint8)
    np.savez(a.out, **res)
    print(json.dumps({"lib_md5": res["lib_md5"], "out": a.out, "bytes": int(sum(res[f"r{i}"].size for i in range(len(REQUESTS))))}))


if __name__ == "__main__":
    main()
