"""The column functionals without a GPU: the header, the ctypes mirror, the Fortran binding and the library's symbols agree, a NULL
handle is refused, and the numpy restatement (tests/functional_reference.py) gives the numbers written out below on a hand-made
case of 8 columns and 4 layers."""
import ctypes as C
import os
import re

import numpy as np

import samsim_amd
from samsim_amd import capi
from samsim_amd.capi import A, FN, FunctionalSpec, State
from tests import functional_reference as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
INF = float("inf")


def header():
    return open(os.path.join(ROOT, "include", "samsim.h")).read()


def code_of(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_declares_the_functions_and_constants():
    code = " ".join(code_of(header()).split())
    assert "int samsim_set_functionals(samsim_handle *h, int32_t n, const samsim_functional_spec *specs);" in code
    assert "int samsim_get_functionals(samsim_handle *h, int32_t index, int64_t col0, int64_t ncols, double *out );" in code
    assert "#define SAMSIM_FUNC_SLOT(i) (0x20000 + (i))" in code
    assert re.search(r"#define SAMSIM_MAX_FUNCTIONALS 8\b", code) and capi.MAX_FUNCTIONALS == 8
    enum = re.search(r"enum samsim_functional_kind \{(.*?)\}", code).group(1)
    names = [n.split("=")[0].strip() for n in enum.split(",")]
    assert names == ["SAMSIM_FN_" + k.upper() for k in capi.FUNCTIONAL_KINDS] + ["SAMSIM_NFN"]
    assert "SAMSIM_FN_INTEGRAL = 0" in enum
    assert "#define SAMSIM_ABI_VERSION 6" in code and capi.ABI_VERSION == 6


def test_struct_layout_matches_the_ctypes_mirror():
    code = code_of(header())
    body = code[code.index("typedef struct samsim_functional_spec {"):code.index("} samsim_functional_spec;")]
    fields = []
    for ctype, decl in re.findall(r"(int32_t|double)\s+([^;]+);", body):
        fields += [(n.strip(), C.c_int32 if ctype == "int32_t" else C.c_double) for n in decl.split(",")]
    assert fields == list(FunctionalSpec._fields_)
    assert C.sizeof(FunctionalSpec) == 56 and FunctionalSpec.z_lo.offset == 24
    s = FunctionalSpec.make("crossing_depth", "psi_l", "bottom", 0.25, 2.0, -1, 0.05, -1.0)
    assert (s.struct_size, s.kind, s.array, s.origin, s.sense, s.reserved) == (56, FN["crossing_depth"], A["psi_l"], 1, -1, 0)
    assert (s.z_lo, s.z_hi, s.threshold, s.missing) == (0.25, 2.0, 0.05, -1.0)
    d = FunctionalSpec.make(0, 4)
    assert (d.kind, d.array, d.origin, d.z_lo, d.z_hi, d.sense) == (0, 4, 0, 0.0, INF, 0) and np.isnan(d.missing)


def test_slots_do_not_overlap():
    assert capi.func_slot(0) == 0x20000
    assert capi.track_slot(capi.MAX_TRACKS - 1, capi.NTF - 1) < capi.func_slot(0)
    assert capi._slot(capi.func_slot(3)) == 0x20003


def test_fortran_binding_and_namelist():
    binding = open(os.path.join(ROOT, "host", "capi_binding.f90")).read()
    driver = open(os.path.join(ROOT, "host", "host_driver.f90")).read()
    for name in ("samsim_set_functionals", "samsim_get_functionals"):
        assert re.search(r"BIND\(C,\s*NAME\s*=\s*['\"]%s['\"]\)" % name, binding, re.I), name
    assert re.search(r"TYPE,\s*BIND\(C\)\s*::\s*samsim_functional_spec", binding, re.I)
    assert re.search(r"NAMELIST\s*/samsim_run/[^/]*\bpermeable_psi_l\b", driver, re.S)
    assert "dat_ens_permeable.dat" in driver


def test_library_exports_and_refuses_a_null_handle():
    lib = samsim_amd.load()
    assert lib.samsim_abi_version() == 6
    setf, getf = lib.samsim_set_functionals, lib.samsim_get_functionals
    setf.argtypes, setf.restype = [C.c_void_p, C.c_int32, C.POINTER(FunctionalSpec)], C.c_int
    getf.argtypes, getf.restype = [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_void_p], C.c_int
    spec = (FunctionalSpec * 1)(FunctionalSpec.make("integral", "T"))
    assert setf(None, 1, spec) == -1
    assert setf(None, 0, None) == -1
    out = np.full(4, -77.0)
    assert getf(None, 0, 0, 4, out.ctypes.data) == -1
    assert (out == -77.0).all()


# ------------------------------------------------------------------------------------------------------------ the reference
def hand_made():
    """8 columns, 4 layers; the values are those of T"""
    thick = [[0.5, 0.5, 0.5, 0.5],        # 0: H = 2
             [0.5, 0.5, 0.5, 0.5],        # 1: Na = 0
             [0.5, 0.0, 0.5, 9.0],        # 2: a layer of zero thickness that holds the smallest value; Na = 3
             [0.25, 0.25, 0.25, 0.25],    # 3: a NaN in layer 2, a tie of the minimum in layers 3 and 4
             [0.25, 0.25, 9.0, 9.0],      # 4: H = 0.5: the window [0.5, 1) lies below the ice
             [0.5, 0.5, 0.5, 0.5],        # 5: decreasing
             [1.0, 9.0, 9.0, 9.0],        # 6: one layer, a NaN
             [1.0, 1.0, 1.0, 1.0]]        # 7: H = 4
    a = [[1, 2, 3, 4], [1, 2, 3, 4], [5, -9, 5, 99], [2, NAN, 1, 1], [7, 8, 99, 99], [4, 3, 2, 1], [NAN, 99, 99, 99], [0, 10, 0, 10]]
    st = State.empty(8, 4)
    st.lay[A["thick"]] = np.array(thick).T
    st.lay[A["T"]] = np.array(a, dtype=np.float64).T
    st.n_active[:] = [4, 0, 3, 4, 2, 4, 1, 4]
    return st


def test_reference_on_the_hand_made_case():
    st = hand_made()
    mk = FunctionalSpec.make
    cases = [
        (mk("integral", "T"), [5.0, 0.0, 5.0, NAN, 3.75, 5.0, NAN, 20.0]),
        # [0.5, 1): in column 0 the layers [0, 0.5) and [1, 1.5) touch the window and are out; column 3's NaN lies above the window,
        # column 6's in it; column 4 ends at 0.5
        (mk("mean", "T", z_lo=0.5, z_hi=1.0, missing=-1.0), [2.0, -1.0, 5.0, 1.0, -1.0, 3.0, NAN, 0.0]),
        (mk("min", "T", missing=-1.0), [1.0, -1.0, 5.0, 1.0, 7.0, 1.0, -1.0, 0.0]),
        (mk("max", "T", missing=-1.0), [4.0, -1.0, 5.0, 2.0, 8.0, 4.0, -1.0, 10.0]),
        (mk("depth_of_min", "T", missing=-1.0), [0.25, -1.0, 0.25, 0.625, 0.125, 1.75, -1.0, 0.5]),
        (mk("depth_of_max", "T", "bottom", missing=-1.0), [0.25, -1.0, 0.75, 0.875, 0.125, 1.75, -1.0, 2.5]),
        (mk("crossing_depth", "T", z_lo=0.25, sense=1, threshold=3.0, missing=-1.0), [1.0, -1.0, 0.25, -1.0, 0.25, 0.25, -1.0, 1.0]),
        # from the bottom the LARGEST k counts: column 0 has T < 3 in layers 1 and 2, layer 2 is [1, 1.5) above the bottom
        (mk("crossing_depth", "T", "bottom", sense=-1, threshold=3.0, missing=-1.0), [1.0, -1.0, -1.0, 0.0, -1.0, 0.0, -1.0, 1.0]),
        (mk("thickness_where", "T", sense=1, threshold=3.0), [1.0, 0.0, 1.0, 0.0, 0.5, 1.0, 0.0, 2.0]),
        (mk("mean", "T", missing=NAN), [2.5, NAN, 5.0, NAN, 7.5, 2.5, NAN, 5.0]),
    ]
    for spec, want in cases:
        got = fr.evaluate(spec, st)
        assert fr.same_bytes(got, np.array(want)), (capi.FUNCTIONAL_KINDS[spec.kind], got.tolist(), want)


def test_reference_layer_values_follow_get_state():
    """S_abs clamped and S_bu = S_abs / m only after a step, in a running column; the clamp not in an uploaded column; the stored
    S_bu where m == 0"""
    st = State.empty(4, 2)
    st.n_active[:] = 2
    st.lay[A["thick"]] = 1.0
    st.lay[A["S_abs"]] = [[-2.0] * 4, [6.0] * 4]
    st.lay[A["m"]] = [[4.0] * 4, [0.0, 3.0, 3.0, 3.0]]
    st.lay[A["S_bu"]] = 77.0
    status = np.array([0, 0, 16, 0], dtype=np.int32)
    uploaded = np.array([False, False, False, True])
    s_abs, s_bu = FunctionalSpec.make("integral", "S_abs"), FunctionalSpec.make("integral", "S_bu")
    assert fr.evaluate(s_abs, st, status, uploaded).tolist() == [6.0, 6.0, 4.0, 4.0]
    assert fr.evaluate(s_bu, st, status, uploaded).tolist() == [77.0, 2.0, 154.0, 1.5]
    assert fr.evaluate(s_abs, st, status, uploaded, stepped=False).tolist() == [4.0] * 4
    assert fr.evaluate(s_bu, st, status, uploaded, stepped=False).tolist() == [154.0] * 4
