"""samsim_select_columns / samsim_get_columns without a GPU: the header declares both with the agreed signatures, the ctypes
mirror and the Fortran binding agree with it, the library exports both under ABI 6 and refuses a NULL handle, and the numpy
restatement of the predicate (tests/select_reference.py) does what the header says on a hand-made case."""
import ctypes as C
import os
import re

import numpy as np

import samsim_amd
from samsim_amd import capi
from tests import select_reference as sr
from tests.helpers import ROOT

NAMES = ("samsim_select_columns", "samsim_get_columns")


def header():
    return open(os.path.join(ROOT, "include", "samsim.h")).read()


def code():
    return re.sub(r"/\*.*?\*/", "", header(), flags=re.S)


def test_header_declares_both_functions():
    text = re.sub(r"\s+", " ", code())
    assert ("int samsim_select_columns(samsim_handle *h, const samsim_selection *sel, int64_t max_out, int64_t *cols_out, "
            "int64_t *n_match);") in text
    assert ("int samsim_get_columns(samsim_handle *h, int64_t ncols, const int64_t *cols, samsim_state_soa *s, int32_t *status, "
            "int64_t *step, int32_t *layer);") in text
    m = re.search(r"^#define SAMSIM_SELECT_SCRATCH_BYTES\s+\((\d+)ull << 20\)", header(), re.M)
    assert m and 1 <= int(m.group(1)) <= 16


def struct_fields(name):
    body = code()
    body = body[body.index("typedef struct %s {" % name):body.index("} %s;" % name)]
    body = body[body.index("{") + 1:]
    return [n.strip().split("[")[0] for decl in re.findall(r"(?:int32_t|double|samsim_select_term)\s+([^;]+);", body) for n in decl.split(",")]


def test_python_mirror_matches_the_header():
    text = header()
    assert capi.SELECT_MAX_TERMS == int(re.search(r"^#define SAMSIM_SELECT_MAX_TERMS\s+(\d+)", text, re.M).group(1)) == 4
    assert capi.SELECT_MAX_OUT == int(re.search(r"^#define SAMSIM_SELECT_MAX_OUT\s+(\d+)", text, re.M).group(1)) == 262144
    assert struct_fields("samsim_select_term") == [n for n, _ in capi.SelectTerm._fields_] == ["slot", "reserved", "lo", "hi"]
    assert [t for _, t in capi.SelectTerm._fields_] == [C.c_int32, C.c_int32, C.c_double, C.c_double]
    assert C.sizeof(capi.SelectTerm) == 24 and capi.SelectTerm.lo.offset == 8 and capi.SelectTerm.hi.offset == 16
    assert struct_fields("samsim_selection") == [n for n, _ in capi.Selection._fields_] \
        == ["struct_size", "nterms", "group", "status_mode", "code", "reserved", "terms"]
    assert [t for _, t in capi.Selection._fields_][:6] == [C.c_int32] * 6
    assert C.sizeof(capi.Selection) == 24 + 24 * capi.SELECT_MAX_TERMS and capi.Selection.terms.offset == 24
    body = code()
    body = body[body.index("enum samsim_select_status {"):]
    names = [n.strip().split("=")[0].strip() for n in body[body.index("{") + 1:body.index("}")].split(",")]
    assert names == ["SAMSIM_SELECT_" + k.upper() for k in sorted(capi.SELECT_STATUS, key=capi.SELECT_STATUS.get)]
    assert capi.SELECT_STATUS == {"running": 0, "stopped": 1, "code": 2, "any": 3}
    sel = capi.Selection.make([("thickness", -np.inf, 0.3), (capi.track_slot(1, "MAX"), 2.0, 3.0)], group=5, status=99)
    assert (sel.struct_size, sel.nterms, sel.group, sel.status_mode, sel.code, sel.reserved) == (120, 2, 5, 2, 99, 0)
    assert (sel.terms[0].slot, sel.terms[0].reserved, sel.terms[0].lo, sel.terms[0].hi) == (capi.S["thickness"], 0, -np.inf, 0.3)
    assert sel.terms[1].slot == 0x10000 + 32 + 6
    sel = capi.Selection.make()
    assert (sel.nterms, sel.group, sel.status_mode, sel.code) == (0, -1, 0, 0)
    for method in ("select", "select_raw", "get_columns"):
        assert callable(getattr(capi.Solver, method))


def test_fortran_host_binds_both_names_and_both_types():
    text = open(os.path.join(ROOT, "host", "capi_binding.f90")).read()
    for name in NAMES:
        assert re.search(rf"FUNCTION\s+{name}\s*\(.*BIND\(C,\s*name='{name}'\)", text), name
    for typ in ("samsim_select_term", "samsim_selection"):
        assert re.search(rf"TYPE,\s*BIND\(C\)\s*::\s*{typ}\b", text), typ
    driver = open(os.path.join(ROOT, "host", "host_driver.f90")).read()
    assert re.search(r"NAMELIST\s*/samsim_run/[^/]*\bmembers_thinner\b[^/]*\bmembers_max\b", driver, re.S)


def test_library_exports_them_and_the_abi_version_stays_6():
    lib = samsim_amd.load()
    for name in NAMES:
        assert hasattr(lib, name), name
    assert lib.samsim_abi_version() == 6 and capi.ABI_VERSION == 6
    assert "#define SAMSIM_ABI_VERSION 6" in header()


def test_null_handle_is_refused_before_any_device_work():
    """no handle, no device: each of the two calls answers SAMSIM_ERR_ARG from its argument checks"""
    lib = samsim_amd.load()
    sel = capi.Selection.make()
    out, n = np.zeros(8, dtype=np.int64), C.c_int64(-7)
    lib.samsim_select_columns.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    lib.samsim_get_columns.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    assert lib.samsim_select_columns(None, C.addressof(sel), 8, out.ctypes.data, C.addressof(n)) == -1
    assert n.value == -7 and not out.any()
    st = capi.State.empty(2, 20)
    s = st._c()
    cols = np.array([0, 1], dtype=np.int64)
    assert lib.samsim_get_columns(None, 2, cols.ctypes.data, C.addressof(s), None, None, None) == -1


def test_reference_on_a_hand_made_case():
    """columns 0..7: the value 2.0 equals lo of [2, 5) and holds, 5.0 equals hi and does not, a NaN holds nowhere"""
    st = capi.State.empty(8, 4)
    x = np.array([1.0, 2.0, 3.0, 5.0, np.nan, 4.0, -np.inf, np.inf])
    st.scal[capi.S["thickness"]] = x
    st.n_active[:] = (1, 2, 3, 4, 1, 2, 3, 4)
    status = np.array([0, 0, 99, 0, 0, 16, 0, 0], dtype=np.int32)
    labels = np.array([0, 1, 1, 1, 1, -1, 0, 1], dtype=np.int32)
    term = [("thickness", 2.0, 5.0)]

    def sel(*a, **k):
        idx, n = sr.select_reference(st, status, *a, **k)
        assert idx.dtype == np.int64 and n == idx.size
        return idx.tolist()
    assert sel(term) == [1]                                    # 2.0 == lo holds; 5.0 == hi does not; 3.0 and 4.0 are stopped
    assert sel(term, mode="any") == [1, 2, 5]
    assert sel(term, mode="stopped") == [2, 5]
    assert sel(term, mode=99) == [2] and sel(term, mode=16) == [5] and sel(term, mode=7) == []
    assert sel([("thickness", -np.inf, np.inf)], mode="any") == [0, 1, 2, 3, 5, 6]     # neither the NaN nor +inf (x < hi fails)
    assert sel([("thickness", 5.0, 2.0)], mode="any") == [] and sel([("thickness", 3.0, 3.0)], mode="any") == []   # lo >= hi
    assert sel(()) == [0, 1, 3, 4, 6, 7] and sel((), mode="any") == list(range(8))     # nterms = 0
    assert sel((), mode="stopped") == [2, 5] and sel((), mode=0) == [0, 1, 3, 4, 6, 7]
    assert sel((), group=1, labels=labels) == [1, 3, 4, 7] and sel((), group=-1, labels=labels) == [0, 1, 3, 4, 6, 7]
    assert sel(term + [("N_active", 2.0, 3.0)], mode="any") == [1, 5]                  # ANDed; N_active as a double
    idx, n = sr.select_reference(st, status, (), mode="any", max_out=3)
    assert idx.tolist() == [0, 1, 2] and n == 8
    tracks = {1: {f: np.arange(8, dtype=np.float64) + i for i, f in enumerate(capi.TRACK_FIELDS)}}
    assert sel([(capi.track_slot(1, "MAX"), 8.0, 10.0)], mode="any", tracks=tracks) == [2, 3]
