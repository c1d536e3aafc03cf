"""bench.py --dump-outputs on the GPU: the files hold the state the timed steps left (warm-up and timed launches together), on a
sample of 64-column windows, in float64 and within the size limit, and --steps sets the number of timed steps."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import samsim_amd
from samsim_amd.capi import A, S
from tests.helpers import DEAD_BETWEEN_OUTPUTS, ROOT

pytestmark = pytest.mark.gpu


def test_dump_outputs_hold_the_state_the_timed_steps_left(tmp_path):
    ncol, substeps, steps, warmup = 8192, 20, 2, 1
    d = tmp_path / "dump"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--ncol", str(ncol), "--substeps", str(substeps),
                          "--steps", str(steps), "--warmup", str(warmup), "--dump-outputs", str(d)],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    r = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert r["steps"] == steps and r["config"]["timed_timesteps"] == steps * substeps and r["ms_per_step"] > 0
    assert "cpu_baseline" not in r and "extra" not in r          # a plain run: those legs are behind --full
    files = sorted(os.listdir(d))
    assert sum(os.path.getsize(d / f) for f in files) < 64 << 20
    got = {f[:-4]: np.load(d / f) for f in files}
    assert all(a.dtype == np.float64 for a in got.values())
    assert "S_br" not in got and "ray" not in got and not DEAD_BETWEEN_OUTPUTS & set(got)

    # the same run through the Python mirror: the tiled ensemble repeats every 256 columns, so each dumped 64-column window must
    # be one of the four 64-member windows of the first 256 columns
    import bench
    cfg, st, pert, clock, forcing, _, _ = bench.workload(argparse.Namespace(workload="sheba", nlayer=80))
    g = samsim_amd.hip_solver(cfg, ncol)
    g.set_forcing(*forcing, bench.tile(pert[0], ncol), bench.tile(pert[1], ncol))
    bench.upload_tiled(g, st, ncol, 0)
    g.set_clock(**clock)
    g.set_output_window(0, 0)
    g.step((steps + warmup) * substeps)
    want = g.get_state(0, 256)
    g.close()
    na = want.n_active
    k = np.arange(cfg.nlayer)[:, None] < na[None, :]
    nwin = got["n_active"].size // 64
    assert nwin >= 1 and got["n_active"].size == 64 * nwin
    for w in range(nwin):
        cols = slice(64 * w, 64 * w + 64)
        matches = []
        for m in range(4):
            mem = slice(64 * m, 64 * m + 64)
            ok = np.array_equal(got["n_active"][cols], na[mem].astype(np.float64))
            for name, a in got.items():
                if not ok:
                    break
                if name in A:
                    ok = np.array_equal(a[:, cols], np.where(k[:, mem], want.arr(name)[:, mem], 0.0))
                elif name in S:
                    ok = np.array_equal(a[cols], want.sc(name)[mem])
            matches.append(ok)
        assert any(matches), f"dumped window {w} is none of the ensemble's member windows"
    assert not got["status"].any()
