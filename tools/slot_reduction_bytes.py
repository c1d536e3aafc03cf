#!/usr/bin/env python3
"""Do two builds of the library return the same bytes from the reductions of the per-column scalars?  On the day-345 melt ensemble
tiled over 70 001 and over 4 197 columns (200 steps, three stopped columns, labels = column mod 9), for the library selected by
SAMSIM_HIP_LIB: the group statistics of eight slots; the histograms of the thickness at 40 and at 254 value bins, ungrouped and by
group, and of T_top by 1 024 groups at 254 bins (the path that does not count in LDS); the covariances of the first k slots, k = 1
to 8; the weight row and its info, Gauss on the thickness and direct on precip_scale; the weighted statistics and covariances of
the first k slots and the weighted histograms at 40 and 254 bins -- everything that takes a group over all columns and over group
4.  Run it once per build, a process each, and compare the files with --compare.

    SAMSIM_HIP_LIB=.../libsamsim_hip_parent.so python tools/slot_reduction_bytes.py --out out/parent.npz
    python tools/slot_reduction_bytes.py --out out/new.npz
    python tools/slot_reduction_bytes.py --compare out/parent.npz out/new.npz > profiles/rN_same_bytes.json
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

SLOTS = ["thickness", "T_top", "m_snow", "thick_snow", "bulk_salin", "N_active", "dT2m", "precip_scale"]
NCOLS = (70001, 4197)
GROUPS = (None, 4)
HISTS = ((40, 0.0, 0.1), (254, 0.0, 0.016))     # nvbins, v0, dv of the thickness


def handle(ncol):
    import samsim_amd
    from samsim_amd import testcases as tcs
    from samsim_amd.capi import State
    z, st, clock, pert = bench.load_ensemble("sheba_ensemble_80_day345.npz")
    cfg, _ = tcs.testcase4(1, nlayer=int(z["nlayer"]), n_top=int(z["n_top"]), n_bottom=int(z["n_bottom"]))
    full = State(bench.tile(st.lay, ncol), bench.tile(st.scal, ncol), bench.tile(st.n_active, ncol).astype(np.int32))
    stopped = (5, ncol // 2, ncol - 1)
    for c in stopped:
        full.arr("H_abs")[0, c] = -1.0e15            # getT cannot converge -> STOP 99
    g = samsim_amd.hip_solver(cfg, ncol)
    g.set_forcing(*bench.sheba_forcing(), bench.tile(pert[0], ncol), bench.tile(pert[1], ncol))
    g.set_state(full)
    g.set_clock(**clock)
    g.set_output_window(0, 0)
    g.step(200)
    assert (g.get_status()[0] != 0).sum() == 3
    return g


def requests(g):
    """(family, request, bytes) of every request on one handle, in a fixed order"""
    def by9():
        g.set_groups((np.arange(g.ncol) % 9).astype(np.int32), ngroups=9)
    by9()
    q = g.group_stats(SLOTS)
    assert min(int(q[n]["count"].min()) for n in SLOTS) > 0
    yield "group_stats", {}, b"".join(q[n].tobytes() for n in SLOTS)
    for nv, v0, dv in HISTS:
        for by_group in (False, True):
            h = g.histogram("thickness", nv, v0, dv, by_group=by_group)
            assert int(h.sum()) == g.ncol - 3
            yield "histogram", dict(nvbins=nv, by_group=by_group, path="lds"), h.tobytes()
    g.set_groups((np.arange(g.ncol) % 1024).astype(np.int32), ngroups=1024)      # 1 024 x 256 counts: not in LDS
    h = g.histogram("T_top", 254, -3.0, 0.0125, by_group=True)
    assert int(h.sum()) == g.ncol - 3
    yield "histogram", dict(nvbins=254, by_group=True, ngroups=1024, path="global"), h.tobytes()
    by9()
    for group in GROUPS:
        for k in range(1, 9):
            n, mean, cov = g.covariance(SLOTS[:k], group=group)
            assert n > 0
            yield "covariance", dict(k=k, group=group), np.int64(n).tobytes() + mean.tobytes() + cov.tobytes()
    for group in GROUPS:
        for slot, kind, scale in (("precip_scale", "direct", 0.0), ("thickness", "gauss", 0.1)):      # the Gauss row stays for what follows
            info = g.set_weights(slot, kind, scale, group) if kind == "gauss" else g.set_weights(slot, kind, group=group)
            assert info["n_pos"] > 0
            fields = np.array([info[f] for f in ("n_in", "n_pos", "x_min", "sum_w", "sum_w2")], dtype=np.float64)
            yield "set_weights", dict(slot=slot, kind=kind, group=group), g.weights().tobytes() + fields.tobytes()
        for k in range(1, 9):
            q = g.weighted_stats(SLOTS[:k], group=group)
            yield "weighted_stats", dict(k=k, group=group), b"".join(np.asarray(q[n]).tobytes() for n in SLOTS[:k])
            n, sw, sw2, mean, cov = g.weighted_covariance(SLOTS[:k], group=group)
            assert n > 0
            yield ("weighted_covariance", dict(k=k, group=group),
                   np.int64(n).tobytes() + np.array([sw, sw2]).tobytes() + mean.tobytes() + cov.tobytes())
        for nv, v0, dv in HISTS:
            h = g.weighted_histogram("thickness", nv, v0, dv, group=group)
            assert float(h.sum()) > 0.0
            yield "weighted_histogram", dict(nvbins=nv, group=group), h.tobytes()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--compare", nargs=2, default=None)
    a = ap.parse_args()
    if a.compare:
        x, y = np.load(a.compare[0]), np.load(a.compare[1])
        keys = json.loads(str(x["keys"]))
        assert keys == json.loads(str(y["keys"]))
        out = {"what": "the reductions of the per-column scalars of two builds of the library, a process per library, every request on "
                       "the same handle; day-345 melt ensemble tiled over ncol columns, 200 steps, three stopped columns, labels = "
                       "column mod 9 (mod 1 024 for the histogram that does not count in LDS); sha256 over the bytes of a request's results",
               "slots": SLOTS, "parent_lib_md5": str(x["lib_md5"]), "new_lib_md5": str(y["lib_md5"]), "requests": []}
        total, same_all = 0, True
        for i, (ncol, fam, rq) in enumerate(keys):
            u, v = x[f"r{i}"].tobytes(), y[f"r{i}"].tobytes()
            total += len(u)
            same_all = same_all and u == v
            out["requests"].append({"ncol": ncol, "family": fam, "request": rq, "parent_sha256": hashlib.sha256(u).hexdigest(),
                                    "new_sha256": hashlib.sha256(v).hexdigest(), "same_bytes": u == v})
        out["bytes_compared"], out["all_bytes_identical"] = total, bool(same_all)
        print(json.dumps(out, indent=1))
        sys.exit(0 if same_all else 1)
    res, keys = {"lib_md5": bench.lib_md5()}, []
    for ncol in NCOLS:
        for fam, rq, b in requests(handle(ncol)):
            res[f"r{len(keys)}"] = np.frombuffer(b, dtype=np.uint8)
            keys.append([ncol, fam, rq])
    res["keys"] = json.dumps(keys)
    np.savez(a.out, **res)
    print(json.dumps({"lib_md5": res["lib_md5"], "out": a.out, "requests": len(keys),
                      "bytes": int(sum(v.size for k, v in res.items() if k.startswith("r")))}))


if __name__ == "__main__":
    main()
