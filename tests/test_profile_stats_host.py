"""samsim_get_profile_stats without a GPU: the boundary (header, exported symbol, ctypes mirror, ABI number) and the numpy
restatement of its semantics (tests/profile_reference.py) on a toy whose answers are worked by hand."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import samsim_amd
from samsim_amd import capi
from samsim_amd.capi import A, ProfileRequest, State
from tests.profile_reference import profile_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    return open(os.path.join(ROOT, "include", "samsim.h")).read()


def test_header_declares_and_library_exports_the_entry_point():
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    assert re.search(r"\bint\s+samsim_get_profile_stats\s*\(\s*samsim_handle\s*\*\s*h\s*,\s*const\s+samsim_profile_request\s*\*", text)
    assert hasattr(samsim_amd.load(), "samsim_get_profile_stats")


def test_abi_version_is_6():
    assert capi.ABI_VERSION == 6
    assert "#define SAMSIM_ABI_VERSION 6" in header()
    assert samsim_amd.load().samsim_abi_version() == 6


def test_request_struct_layout_matches_header():
    """field names, order and size of samsim_profile_request in the header == ctypes mirror"""
    text = header()
    defines = {n: int(v) for n, v in re.findall(r"^#define (SAMSIM_PROFILE_MAX_\w+)\s+(\d+)", text, re.M)}
    assert defines == {"SAMSIM_PROFILE_MAX_BINS": capi.PROFILE_MAX_BINS, "SAMSIM_PROFILE_MAX_ARRAYS": capi.PROFILE_MAX_ARRAYS}
    body = text[text.index("typedef struct samsim_profile_request {"):text.index("} samsim_profile_request;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names, size, align = [], 0, 1
    for ctype, decl in re.findall(r"(int32_t|double)\s+([^;]+);", body):
        width = {"int32_t": 4, "double": 8}[ctype]
        for item in decl.split(","):
            m = re.fullmatch(r"(\w+)(?:\[(\w+)\])?", item.strip())
            names.append(m.group(1))
            count = 1 if m.group(2) is None else defines.get(m.group(2)) or int(m.group(2))
            size = (size + width - 1) // width * width + width * count      # natural alignment
            align = max(align, width)
    size = (size + align - 1) // align * align
    assert names == [n for n, *_ in ProfileRequest._fields_]
    assert C.sizeof(ProfileRequest) == size
    for text_name, table in (("samsim_profile_axis", capi.PROFILE_AXES), ("samsim_profile_origin", capi.PROFILE_ORIGINS)):
        enum = re.search(rf"enum {text_name}\s*\{{([^}}]*)\}}", text).group(1)
        assert sorted(int(v) for v in re.findall(r"=\s*(\d+)", enum)) == sorted(table.values())


def toy():
    """three columns of four layers: column 0 ends inside a bin (H = 0.3125 with dz = 0.125) and has a massless layer; column 1
    has one active layer; column 2 carries a STOP code and absurd values.  Every thickness is a binary fraction, so the
    hand-worked numbers below are exact."""
    st = State.empty(3, 4)
    st.n_active[:] = (3, 1, 4)
    st.arr("thick")[:, 0] = (0.125, 0.125, 0.0625, 9.0)
    st.arr("T")[:, 0] = (-10.0, -6.0, -2.0, 77.0)          # layer 4 is not active: never read
    st.arr("S_abs")[:, 0] = (10.0, 20.0, 7.0, 1.0)
    st.arr("m")[:, 0] = (2.0, 4.0, 0.0, 1.0)               # m(3) = 0: the stored S_bu counts there
    st.arr("S_bu")[:, 0] = (99.0, 99.0, 5.0, 99.0)
    st.arr("thick")[0, 1], st.arr("T")[0, 1] = 0.125, -4.0
    st.arr("S_abs")[0, 1], st.arr("m")[0, 1], st.arr("S_bu")[0, 1] = 9.0, 3.0, 99.0
    st.lay[:, :, 2] = 1.0e30
    return st, np.array([0, 0, 99], dtype=np.int32)


def rows(q):
    return [tuple(r) for r in q.tolist()]


def test_reference_by_layer_on_the_toy():
    st, status = toy()
    q = profile_reference(st, status, ["T", "S_bu"], axis="layer", origin="top", nbins=4)
    assert rows(q["T"]) == [(2, -7.0, -10.0, -4.0, 3.0), (1, -6.0, -6.0, -6.0, 0.0), (1, -2.0, -2.0, -2.0, 0.0), (0, 0.0, 0.0, 0.0, 0.0)]
    assert rows(q["S_bu"]) == [(2, 4.0, 3.0, 5.0, 1.0), (1, 5.0, 5.0, 5.0, 0.0), (1, 5.0, 5.0, 5.0, 0.0), (0, 0.0, 0.0, 0.0, 0.0)]
    q = profile_reference(st, status, ["T"], axis="layer", origin="bottom", nbins=4)
    assert rows(q["T"]) == [(2, -3.0, -4.0, -2.0, 1.0), (1, -6.0, -6.0, -6.0, 0.0), (1, -10.0, -10.0, -10.0, 0.0), (0, 0.0, 0.0, 0.0, 0.0)]


def test_reference_by_depth_on_the_toy():
    st, status = toy()
    # from the top, bins [0, .125), [.125, .25), [.25, .375), [.375, .5): column 0 fills 0.0625 m of the third and ends there
    q = profile_reference(st, status, ["T"], axis="depth", origin="top", nbins=4, z0=0.0, dz=0.125)
    assert rows(q["T"]) == [(2, -7.0, -10.0, -4.0, 3.0), (1, -6.0, -6.0, -6.0, 0.0), (1, -2.0, -2.0, -2.0, 0.0), (0, 0.0, 0.0, 0.0, 0.0)]
    # from the bottom: layer 3 covers [0, .0625), layer 2 [.0625, .1875), layer 1 [.1875, .3125)
    #   bin 0: (0.0625*(-6) + 0.0625*(-2)) / 0.125 = -4 and column 1's -4;  bin 1: (0.0625*(-10) + 0.0625*(-6)) / 0.125 = -8;  bin 2: -10
    q = profile_reference(st, status, ["T"], axis="depth", origin="bottom", nbins=3, z0=0.0, dz=0.125)
    assert rows(q["T"]) == [(2, -4.0, -4.0, -4.0, 0.0), (1, -8.0, -8.0, -8.0, 0.0), (1, -10.0, -10.0, -10.0, 0.0)]
    # z0 = 0.0625 from the top, bins [.0625, .1875), [.1875, .3125), [.3125, .4375):
    #   bin 0: column 0 (0.0625*(-10) + 0.0625*(-6)) / 0.125 = -8, column 1 0.0625*(-4) / 0.0625 = -4
    #   bin 1: column 0 (0.0625*(-6) + 0.0625*(-2)) / 0.125 = -4;  bin 2 starts where column 0 ends: empty
    q = profile_reference(st, status, ["T", "thick"], axis="depth", origin="top", nbins=3, z0=0.0625, dz=0.125)
    assert rows(q["T"]) == [(2, -6.0, -8.0, -4.0, 2.0), (1, -4.0, -4.0, -4.0, 0.0), (0, 0.0, 0.0, 0.0, 0.0)]
    assert rows(q["thick"]) == [(2, 0.125, 0.125, 0.125, 0.0), (1, 0.09375, 0.09375, 0.09375, 0.0), (0, 0.0, 0.0, 0.0, 0.0)]
    # z0 = 0.0625 from the bottom, two bins: bin 0 [.0625, .1875) is layer 2 of column 0 (-6) and half of column 1's layer;
    #   bin 1 [.1875, .3125) is layer 1 of column 0
    q = profile_reference(st, status, ["T"], axis="depth", origin="bottom", nbins=2, z0=0.0625, dz=0.125)
    assert rows(q["T"]) == [(2, -5.0, -6.0, -4.0, 1.0), (1, -10.0, -10.0, -10.0, 0.0)]


def test_python_mirror_fills_the_request():
    """Solver.profile_stats fills the request the header describes and hands the rows back by name (on a Solver without a
    handle whose raw call records the request instead of reaching the library)"""
    seen = []

    class Recorder(capi.Solver):
        def __init__(self):
            self.nlayer = 80

        def profile_stats_raw(self, rq):
            seen.append(rq)
            out = np.zeros((rq.narrays, rq.nbins), dtype=capi.STAT_DTYPE)
            out["count"] = np.arange(rq.narrays)[:, None]
            return out

        def close(self):
            pass
    s = Recorder()
    q = s.profile_stats(["T", "S_bu", "psi_l"], axis="depth", origin="bottom", nbins=32, z0=0.035, dz=0.07)
    rq = seen[-1]
    assert (rq.struct_size, rq.axis, rq.origin, rq.nbins, rq.narrays) == (C.sizeof(ProfileRequest), 1, 1, 32, 3)
    assert list(rq.arrays)[:3] == [A["T"], A["S_bu"], A["psi_l"]] and (rq.z0, rq.dz) == (0.035, 0.07)
    assert list(q) == ["T", "S_bu", "psi_l"] and q["psi_l"].shape == (32,) and (q["psi_l"]["count"] == 2).all()
    s.profile_stats(["thick"])                               # the layer axis from the top, every layer
    rq = seen[-1]
    assert (rq.axis, rq.origin, rq.nbins, rq.narrays, rq.arrays[0]) == (0, 0, 80, 1, A["thick"])
    with pytest.raises(ValueError):
        s.profile_stats(["T"], axis="depth")                 # the depth axis needs nbins and dz
    with pytest.raises(KeyError):
        s.profile_stats(["no_such_array"])
    assert capi.STAT_DTYPE.itemsize == C.sizeof(capi.Stat) == 40
