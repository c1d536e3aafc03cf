"""The time-domain diagnostics without a GPU: the numpy restatement of the header's update rule (tests/track_reference.py) on
the CPU oracle's trajectory of the committed melt-onset waves (70 columns: one full block and one of 6; 24 steps), which pins the
conditions tests/test_gpu_tracks.py relies on -- in how many columns the condition T_top >= 0.0 comes to hold and when, where the
ice thickness moves -- so that a test in which nothing ever happens cannot pass; and that the ctypes mirror agrees with the header."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from samsim_amd import capi
from samsim_amd.capi import TrackSpec
from tests import melt_onset_seeds as mo
from tests import track_reference as tr
from tests.helpers import ROOT

SPECS = [TrackSpec.make("scalar", "T_top", sense=+1, threshold=0.0), TrackSpec.make("ice_thickness"), TrackSpec.make("n_active"),
         TrackSpec.make("bulk_salinity"), TrackSpec.make("layer", "T", layer=1), TrackSpec.make("layer", "S_abs", layer=-1)]


@functools.lru_cache(maxsize=None)
def wave_tracks(which, every=1):
    cfg, st, clock, dT, ps, _ = mo.load_wave(which)
    traj, status = mo.oracle_trajectory(cfg, st, clock, dT, ps)
    steps = [clock["step"] + i + 1 for i in range(mo.NSTEPS)]
    samples = [(s, traj[i], np.zeros(st.ncol, dtype=np.int32)) for i, s in enumerate(steps) if s % every == 0]
    return clock["step"], traj, status, tr.apply(SPECS, samples)


# wave: columns in which T_top >= 0.0 comes to hold, distinct values of STEP_FIRST, range of N_HOLD, columns whose thickness moves
TABLE = {"spread": (70, 16, (8, 23), 0), "melt": (11, 2, (0, 14), 64)}


@pytest.mark.parametrize("which", list(TABLE))
def test_reference_on_the_oracle_trajectory(which):
    step0, traj, status, rows = wave_tracks(which)
    holds_in, distinct, (lo, hi), thickness_moves = TABLE[which]
    ttop, thick, nact, salt, t1, sbot = rows
    assert not status.any()                                                       # no column stops
    for r in rows:
        assert (r["N"] == mo.NSTEPS).all() and (r["STEP_MIN"] > step0).all() and (r["STEP_MAX"] <= step0 + mo.NSTEPS).all()
    first = ttop["STEP_FIRST"]
    print(which, "T_top >= 0 holds in", int((first >= 0).sum()), "columns; STEP_FIRST - step0", sorted(set((first[first >= 0] - step0).tolist())),
          "; N_HOLD", ttop["N_HOLD"].min(), "..", ttop["N_HOLD"].max(), "; thickness moves in", int((thick["MIN"] != thick["MAX"]).sum()))
    assert (first >= 0).sum() == holds_in and len(set(first.tolist())) == distinct    # (the -1 of "never" is one of the values)
    assert not (first == step0 + 1).any()                                         # it holds at the first sample in no column
    assert ttop["N_HOLD"].min() == lo and ttop["N_HOLD"].max() == hi
    assert ((first >= 0) == (ttop["N_HOLD"] > 0)).all() and (ttop["STEP_LAST"] >= first).all()
    assert (thick["MIN"] != thick["MAX"]).sum() == thickness_moves
    assert (nact["MIN"] == nact["MAX"]).all() and (nact["M2"] == 0.0).all()       # n_active changes in no column
    # the rule against the plain definitions, on the whole trajectory
    x = np.stack([s.sc("T_top") for s in traj])
    assert np.array_equal(ttop["MIN"], x.min(0)) and np.array_equal(ttop["MAX"], x.max(0)) and np.array_equal(ttop["LAST"], x[-1])
    assert np.array_equal(ttop["STEP_MIN"], step0 + 1 + x.argmin(0)) and np.array_equal(ttop["STEP_MAX"], step0 + 1 + x.argmax(0))
    assert np.array_equal(ttop["N_HOLD"], (x >= 0.0).sum(0))
    assert np.allclose(ttop["MEAN"], x.mean(0), rtol=1e-13, atol=1e-13) and np.allclose(ttop["M2"] / ttop["N"], x.var(0), rtol=1e-10, atol=1e-14)
    na = traj[-1].n_active
    assert np.array_equal(t1["LAST"], traj[-1].arr("T")[0]) and np.array_equal(sbot["LAST"], traj[-1].arr("S_abs")[na - 1, np.arange(na.size)])
    assert (salt["MIN"] > 0.0).all() and (salt["MAX"] < 40.0).all() and (thick["MIN"] > 0.1).all()


def test_cadence_follows_the_absolute_step_count():
    step0, traj, _, rows = wave_tracks("spread", 5)
    # phase and tail, as the GPU test assumes: the wave's clock (step 2 943 783) is a multiple of 3 but of neither 5 nor 7, and 24 is
    # a multiple of neither 5 nor 7
    assert step0 % 3 == 0 and step0 % 5 != 0 and step0 % 7 != 0 and mo.NSTEPS % 5 != 0 and mo.NSTEPS % 7 != 0
    due = [s for s in range(step0 + 1, step0 + mo.NSTEPS + 1) if s % 5 == 0]
    assert (rows[0]["N"] == len(due)).all() and len(due) in (4, 5)
    assert set(rows[0]["STEP_MIN"].tolist()) <= set(due)
    assert np.array_equal(rows[0]["LAST"], traj[due[-1] - step0 - 1].sc("T_top"))


def test_a_nan_is_no_extreme_and_holds_nothing_and_a_missing_layer_is_not_sampled():
    st = capi.State.empty(3, 4)
    st.n_active[:] = (1, 2, 4)
    st.lay[capi.A["T"]] = np.arange(12, dtype=np.float64).reshape(4, 3)
    st.scal[capi.S["T_top"]] = (np.nan, -1.0, 2.0)
    specs = [TrackSpec.make("scalar", "T_top", sense=-1, threshold=0.0), TrackSpec.make("layer", "T", layer=2),
             TrackSpec.make("layer", "T", layer=-3)]
    a, b, c = tr.apply(specs, [(7, st, np.zeros(3, dtype=np.int32)), (9, st, np.array([0, 5, 0], dtype=np.int32))])
    assert a["N"].tolist() == [2, 1, 2] and a["N_HOLD"].tolist() == [0, 1, 0] and a["STEP_FIRST"].tolist() == [-1, 7, -1]
    assert np.isinf(a["MIN"][0]) and a["STEP_MIN"].tolist() == [-1, 7, 7] and np.isnan(a["MEAN"][0])
    assert b["N"].tolist() == [0, 1, 2] and b["LAST"].tolist() == [0.0, 4.0, 5.0] and b["STEP_MAX"].tolist() == [-1, 7, 7]
    assert c["N"].tolist() == [0, 0, 2] and c["LAST"].tolist() == [0.0, 0.0, 5.0]   # layer Na + 1 - 3 = 2 of the third column


def test_the_mirror_agrees_with_the_header():
    text = open(os.path.join(ROOT, "include", "samsim.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)

    def enum(name):
        body = code[code.index("enum %s {" % name):]
        return [n.strip().split("=")[0].strip() for n in body[body.index("{") + 1:body.index("}")].split(",")]
    assert enum("samsim_track_field") == ["SAMSIM_TF_" + f for f in capi.TRACK_FIELDS] + ["SAMSIM_NTF"]
    assert enum("samsim_observable_kind") == ["SAMSIM_OBS_" + k.upper() for k in capi.OBSERVABLES]
    assert capi.NTF == 11 and "#define SAMSIM_MAX_TRACKS %d\n" % capi.MAX_TRACKS in code
    body = code[code.index("typedef struct samsim_track_spec {"):code.index("} samsim_track_spec;")]
    names = [n for decl in re.findall(r"(?:int32_t|double)\s+([^;]+);", body) for n in (x.strip() for x in decl.split(","))]
    assert names == [n for n, _ in TrackSpec._fields_] and C.sizeof(TrackSpec) == 32
    assert [t for n, t in TrackSpec._fields_] == [C.c_int32] * 6 + [C.c_double]
    assert "#define SAMSIM_TRACK_SLOT(track, field) (0x10000 + (track) * 32 + (field))" in code
    assert capi.track_slot(0, "N") == 0x10000 and capi.track_slot(3, "STEP_FIRST") == 0x10000 + 3 * 32 + 9 == capi.track_slot(3, 9)
    assert capi.track_slot(capi.MAX_TRACKS - 1, capi.NTF - 1) < 2 ** 31 and capi.NTF <= 32
    spec = TrackSpec.make("layer", "S_bu", layer=-1, sense=-1, threshold=4.5)
    assert (spec.struct_size, spec.kind, spec.id, spec.layer, spec.sense, spec.reserved, spec.threshold) == (32, 4, capi.A["S_bu"], -1, -1, 0, 4.5)
    for f, v in capi.TRACK_INITIAL.items():
        assert "%s = %s" % (f, {0.0: "0", -1.0: "-1", np.inf: "+inf", -np.inf: "-inf"}[v]) in text, f
