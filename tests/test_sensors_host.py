"""The sensors and the per-column misfit without a GPU: the header, the ctypes mirror, the Fortran binding and the library's symbols
agree, a NULL handle is refused, and the numpy restatement (tests/sensor_reference.py) gives the numbers written out below on a
hand-made case of 5 columns and 4 layers."""
import ctypes as C
import os
import re

import numpy as np

import samsim_amd
from samsim_amd import capi
from samsim_amd.capi import A, S, SensorSpec, State
from tests import sensor_reference as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
FUNCTIONS = ("samsim_set_sensors", "samsim_get_sensor_values", "samsim_score", "samsim_get_scores", "samsim_set_score_state",
             "samsim_reset_scores")
mk = SensorSpec.make


def header():
    return open(os.path.join(ROOT, "include", "samsim.h")).read()


def code_of(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_declares_the_functions_and_constants():
    code = " ".join(code_of(header()).split())
    for decl in ("int samsim_set_sensors(samsim_handle *h, int32_t n, const samsim_sensor_spec *specs);",
                 "int samsim_get_sensor_values(samsim_handle *h, int64_t ncols, const int64_t *cols, double *y );",
                 "int samsim_score(samsim_handle *h, const double *obs , const double *weight , int32_t group);",
                 "int samsim_get_scores(samsim_handle *h, int64_t col0, int64_t ncols, double *out );",
                 "int samsim_set_score_state(samsim_handle *h, int64_t col0, int64_t ncols, const double *in );",
                 "int samsim_reset_scores(samsim_handle *h);"):
        assert decl in code, decl
    assert "#define SAMSIM_SCORE_SLOT(field) (0x30000 + (field))" in code
    assert re.search(r"#define SAMSIM_MAX_SENSORS 32\b", code) and capi.MAX_SENSORS == 32

    def names(enum):
        body = re.search(r"enum %s \{(.*?)\}" % enum, code).group(1)
        return [n.strip() for n in body.split(",")]
    assert names("samsim_sensor_kind") == ["SAMSIM_SENSOR_PROFILE = 0"] + \
        ["SAMSIM_SENSOR_" + k.upper() for k in capi.SENSOR_KINDS[1:]] + ["SAMSIM_NSENSOR_KINDS"]
    assert names("samsim_sensor_interp") == ["SAMSIM_SENSOR_STEP = 0", "SAMSIM_SENSOR_LINEAR = 1"]
    assert capi.SENSOR_INTERPS == {"step": 0, "linear": 1}
    assert names("samsim_score_field") == ["SAMSIM_SF_N_LAST = 0"] + ["SAMSIM_SF_" + f for f in capi.SCORE_FIELDS[1:]] + ["SAMSIM_NSF"]
    assert capi.NSF == 9
    assert "#define SAMSIM_ABI_VERSION 6" in code and capi.ABI_VERSION == 6


def test_struct_layout_matches_the_ctypes_mirror():
    code = code_of(header())
    body = code[code.index("typedef struct samsim_sensor_spec {"):code.index("} samsim_sensor_spec;")]
    fields = []
    for ctype, decl in re.findall(r"(int32_t|double)\s+([^;]+);", body):
        fields += [(n.strip(), C.c_int32 if ctype == "int32_t" else C.c_double) for n in decl.split(",")]
    assert fields == list(SensorSpec._fields_)
    assert C.sizeof(SensorSpec) == 40 and SensorSpec.z.offset == 24
    s = mk("profile", "S_bu", 0.25, "bottom", "linear", -1.0)
    assert (s.struct_size, s.kind, s.id, s.origin, s.interp, s.reserved, s.z, s.missing) == (40, 0, A["S_bu"], 1, 1, 0, 0.25, -1.0)
    s = mk("scalar", "thick_snow")
    assert (s.kind, s.id, s.origin, s.interp, s.z) == (1, S["thick_snow"], 0, 0, 0.0) and np.isnan(s.missing)
    s = mk("ice_thickness")
    assert (s.kind, s.id, s.origin, s.interp, s.z) == (2, 0, 0, 0, 0.0)


def test_slots_do_not_overlap():
    assert capi.score_slot(0) == 0x30000 > capi.func_slot(capi.MAX_FUNCTIONALS - 1)
    assert capi.score_slot("J_SUM") == 0x30005 and capi._slot(capi.score_slot("CALLS")) == 0x30008


def test_fortran_binding_names_every_symbol():
    binding = open(os.path.join(ROOT, "host", "capi_binding.f90")).read()
    for name in FUNCTIONS:
        assert re.search(r"BIND\(C,\s*NAME\s*=\s*['\"]%s['\"]\)" % name, binding, re.I), name
    assert re.search(r"TYPE,\s*BIND\(C\)\s*::\s*samsim_sensor_spec", binding, re.I)
    for name in ("SAMSIM_MAX_SENSORS", "SAMSIM_SENSOR_PROFILE", "SAMSIM_SENSOR_SCALAR", "SAMSIM_SENSOR_ICE_THICKNESS", "SAMSIM_SENSOR_STEP",
                 "SAMSIM_SENSOR_LINEAR", "SAMSIM_NSF", "samsim_score_slot") + tuple("SAMSIM_SF_" + f for f in capi.SCORE_FIELDS):
        assert re.search(r"\b%s\b" % name, binding), name


def test_library_exports_and_refuses_a_null_handle():
    lib = samsim_amd.load()
    assert lib.samsim_abi_version() == 6
    vp, i64 = C.c_void_p, C.c_int64
    sig = {"samsim_set_sensors": [vp, C.c_int32, C.POINTER(SensorSpec)], "samsim_get_sensor_values": [vp, i64, vp, vp],
           "samsim_score": [vp, vp, vp, C.c_int32], "samsim_get_scores": [vp, i64, i64, vp],
           "samsim_set_score_state": [vp, i64, i64, vp], "samsim_reset_scores": [vp]}
    assert sorted(sig) == sorted(FUNCTIONS)
    f = {}
    for name, args in sig.items():
        f[name] = getattr(lib, name)
        f[name].argtypes, f[name].restype = args, C.c_int
    spec = (SensorSpec * 1)(mk("ice_thickness"))
    assert f["samsim_set_sensors"](None, 1, spec) == -1
    assert f["samsim_set_sensors"](None, 0, None) == -1
    cols = np.arange(4, dtype=np.int64)
    out = np.full((capi.NSF, 4), -77.0)
    assert f["samsim_get_sensor_values"](None, 4, cols.ctypes.data, out.ctypes.data) == -1
    assert f["samsim_score"](None, out.ctypes.data, None, -1) == -1
    assert f["samsim_get_scores"](None, 0, 4, out.ctypes.data) == -1
    assert f["samsim_set_score_state"](None, 0, 4, out.ctypes.data) == -1
    assert f["samsim_reset_scores"](None) == -1
    assert (out == -77.0).all()


# ------------------------------------------------------------------------------------------------------------ the reference
def hand_made():
    """5 columns, 4 layers; the values are those of T"""
    thick = [[0.5, 0.5, 0.5, 0.5],        # 0: H = 2
             [0.5, 0.5, 0.5, 0.5],        # 1: Na = 0
             [0.5, 0.0, 0.5, 9.0],        # 2: a layer of zero thickness that holds the extreme value; Na = 3, H = 1
             [0.25, 0.25, 0.25, 0.25],    # 3: a NaN in layer 2; H = 1
             [0.25, 0.25, 9.0, 9.0]]      # 4: Na = 2, H = 0.5
    a = [[1, 2, 3, 4], [1, 2, 3, 4], [5, -9, 5, 99], [2, NAN, 1, 1], [7, 8, 99, 99]]
    st = State.empty(5, 4)
    st.lay[A["thick"]] = np.array(thick).T
    st.lay[A["T"]] = np.array(a, dtype=np.float64).T
    st.scal[S["thick_snow"]] = [10.0, 11.0, 12.0, 13.0, 14.0]
    st.n_active[:] = [4, 0, 3, 4, 2]
    return st


# (spec, expected value per column, expected "in the ice" per column); missing = -1
CASES = [
    # STEP from the top at 0.6: column 2's zero-thickness layer [0.5, 0.5) never contains it, layer 3 [0.5, 1) does
    (mk("profile", "T", 0.6, missing=-1.0), [2.0, -1.0, 5.0, 1.0, -1.0], [1, 0, 1, 1, 0]),
    # LINEAR at 0.6: column 0 between the midpoints 0.25 and 0.75; column 2 between the zero-thickness layer (midpoint 0.5, -9) and
    # layer 3 (0.75, 5); column 3's neighbour is the NaN
    (mk("profile", "T", 0.6, interp="linear", missing=-1.0),
     [1.0 + ((0.6 - 0.25) / 0.5) * 1.0, -1.0, -9.0 + ((0.6 - 0.5) / (0.75 - 0.5)) * 14.0, NAN, -1.0], [1, 0, 1, 1, 0]),
    # LINEAR at 0.1: above the first midpoint there is no upper neighbour
    (mk("profile", "T", 0.1, interp="linear", missing=-1.0), [1.0, -1.0, 5.0, 2.0, 7.0], [1, 0, 1, 1, 1]),
    # z = 2.0 = H of column 0: below the ice everywhere
    (mk("profile", "T", 2.0, missing=-1.0), [-1.0] * 5, [0] * 5),
    (mk("profile", "T", 2.0, interp="linear", missing=NAN), [NAN] * 5, [0] * 5),
    # from the bottom at 0.6: column 0's layer 3 is [0.5, 1); column 2's layer 1 is [0.5, 1); column 3's layer 2 [0.5, 0.75) is the NaN
    (mk("profile", "T", 0.6, "bottom", missing=-1.0), [3.0, -1.0, 5.0, NAN, -1.0], [1, 0, 1, 1, 0]),
    # ... LINEAR: the neighbour below is the one with the larger index and the smaller coordinate
    (mk("profile", "T", 0.6, "bottom", "linear", missing=-1.0),
     [4.0 + ((0.6 - 0.25) / 0.5) * -1.0, -1.0, -9.0 + ((0.6 - 0.5) / (0.75 - 0.5)) * 14.0, NAN, -1.0], [1, 0, 1, 1, 0]),
    # LINEAR at 0.45: column 2's lower neighbour has zero thickness and holds -9; column 3's own layer is the NaN; column 4 is in its
    # last layer below the midpoint: no lower neighbour
    (mk("profile", "T", 0.45, interp="linear", missing=-1.0),
     [1.0 + ((0.45 - 0.25) / 0.5) * 1.0, -1.0, 5.0 + ((0.45 - 0.25) / (0.5 - 0.25)) * -14.0, NAN, 8.0], [1, 0, 1, 1, 1]),
    # STEP at 0.3 in column 3: the NaN itself
    (mk("profile", "T", 0.3, missing=-1.0), [1.0, -1.0, 5.0, NAN, 8.0], [1, 0, 1, 1, 1]),
    (mk("ice_thickness"), [2.0, 0.0, 1.0, 1.0, 0.5], [1] * 5),
    (mk("scalar", "thick_snow"), [10.0, 11.0, 12.0, 13.0, 14.0], [1] * 5),
]


def test_reference_on_the_hand_made_case():
    st = hand_made()
    for n, (spec, want, want_in) in enumerate(CASES):
        info = {}
        got, in_ice = sr.evaluate(spec, st, info=info)
        assert sr.same_bytes(got, np.array(want)), (n, got.tolist(), want)
        assert in_ice.tolist() == [bool(x) for x in want_in], (n, in_ice.tolist())
    info = {}
    sr.evaluate(CASES[7][0], st, info=info)
    assert info["zero_neighbour"].tolist() == [False, False, True, False, False]
    assert info["extrapolated"].tolist() == [False, False, False, False, True]
    sr.evaluate(CASES[2][0], st, info=info)
    assert info["extrapolated"].tolist() == [True, False, True, True, True]


def test_reference_layer_values_follow_get_state():
    """S_abs clamped and S_bu = S_abs / m only after a step, in a running column; the clamp not in an uploaded column; the stored
    S_bu where m == 0"""
    st = State.empty(4, 3)
    st.n_active[:] = 2
    st.lay[A["thick"]] = 1.0
    st.lay[A["S_abs"]] = [[-2.0] * 4, [6.0] * 4, [0.0] * 4]
    st.lay[A["m"]] = [[4.0] * 4, [0.0, 3.0, 3.0, 3.0], [1.0] * 4]
    st.lay[A["S_bu"]] = 77.0
    status = np.array([0, 0, 16, 0], dtype=np.int32)
    uploaded = np.array([False, False, False, True])
    for z, s_abs, s_bu in ((0.5, [0.0, 0.0, -2.0, -2.0], [0.0, 0.0, 77.0, -0.5]), (1.5, [6.0] * 4, [77.0, 2.0, 77.0, 2.0])):
        assert sr.evaluate(mk("profile", "S_abs", z), st, status, uploaded)[0].tolist() == s_abs
        assert sr.evaluate(mk("profile", "S_bu", z), st, status, uploaded)[0].tolist() == s_bu
    assert sr.evaluate(mk("profile", "S_abs", 0.5), st, status, uploaded, stepped=False)[0].tolist() == [-2.0] * 4
    assert sr.evaluate(mk("profile", "S_bu", 0.5), st, status, uploaded, stepped=False)[0].tolist() == [77.0] * 4


def test_score_update_on_the_hand_made_case():
    st = hand_made()
    specs = [CASES[0][0], CASES[1][0], CASES[3][0], CASES[9][0]]      # STEP 0.6, LINEAR 0.6, below the ice, thickness
    y, in_ice = sr.evaluate_all(specs, st)
    assert in_ice[:, 0].tolist() == [True, True, False, True]
    obs, w = np.array([1.5, NAN, 0.0, 1.0]), np.array([2.0, 1.0, 1.0, 0.5])
    scored = np.array([True, True, True, True, False])
    r1 = sr.score_update(sr.zero_rows(5), y, in_ice, obs, w, scored)
    # column 0: sensor 0 (d = 0.5, w = 2) and sensor 3 (d = 1, w = 0.5) are valid; sensor 1 has no observation, sensor 2 is not in the ice
    assert [r1[f][0] for f in capi.SCORE_FIELDS] == [2.0, 1.0, 1.5, 2.5, 2.0, 1.0, 1.5, 2.5, 1.0]
    # column 1 (Na = 0): only the thickness, 0 - 1
    assert [r1[f][1] for f in capi.SCORE_FIELDS] == [1.0, 0.5, -0.5, 0.5, 1.0, 0.5, -0.5, 0.5, 1.0]
    # column 4 is not scored: nothing changes
    assert [r1[f][4] for f in capi.SCORE_FIELDS] == [0.0] * 9
    # without weights: column 2, sensors 0 (5 - 1.5) and 3 (1 - 1)
    r2 = sr.score_update(sr.zero_rows(5), y, in_ice, obs)
    assert [r2[f][2] for f in capi.SCORE_FIELDS] == [2.0, 12.25, 3.5, 2.0, 2.0, 12.25, 3.5, 2.0, 1.0]
    # all observations missing: the LAST fields are 0, the sums stay
    r3 = sr.score_update(r1, y, in_ice, np.full(4, NAN), w, scored)
    for f in capi.SCORE_FIELDS:
        assert sr.same_bytes(r3[f], np.where(scored & f.endswith("LAST"), 0.0, r1[f])), f
    # a NaN value of a valid sensor makes J a NaN: column 3 with LINEAR 0.6
    r4 = sr.score_update(r1, y, in_ice, np.array([NAN, 0.0, NAN, NAN]), None, scored)
    assert np.isnan(r4["J_LAST"][3]) and np.isnan(r4["J_SUM"][3]) and np.isnan(r4["B_SUM"][3])
    assert r4["N_LAST"][3] == 1.0 and r4["W_SUM"][3] == r1["W_SUM"][3] + 1.0 and r4["CALLS"][3] == 2.0
    y0 = 1.0 + ((0.6 - 0.25) / 0.5) * 1.0
    assert r4["J_LAST"][0] == y0 * y0 and r4["B_LAST"][0] == y0 and r4["CALLS"][4] == 0.0
