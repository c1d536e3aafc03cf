"""The STOP seeds of tests/stop_seeds.py on the CPU: every seed keeps the rules of a mutation, the oracle really stops its column
with the aimed-at code within 64 steps (a seed the oracle does not stop is a failure here, so the GPU test cannot pass vacuously),
and the site table names every STOPC of the step kernel's source.  Prints the table (site, seed, code, step, layer)."""
import os
import re

import numpy as np
import pytest

from tests import stop_seeds as ss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "samsim_amd", "csrc")


@pytest.mark.parametrize("seed", ss.SEEDS, ids=lambda s: s.name)
def test_mutation_is_finite_and_touches_only_what_it_may(seed):
    for col in ss.COLUMNS:
        cfg, st, _ = ss.build(seed, col)
        _, clean, _ = ss.build(seed, col, mutated=False)
        assert np.array_equal(st.n_active, clean.n_active), "n_active is never touched"
        assert np.isfinite(st.lay).all() and np.isfinite(st.scal).all(), "only finite values"
        others = np.arange(ss.NCOL) != col
        assert np.array_equal(st.lay[:, :, others], clean.lay[:, :, others]) and np.array_equal(st.scal[:, others], clean.scal[:, others])
        changed = False
        na = int(st.n_active[col])
        for i in range(st.lay.shape[0]):
            diff = np.nonzero(st.lay[i, :, col] != clean.lay[i, :, col])[0]
            if diff.size:
                changed = True
                assert i < len(ss.PROGNOSTIC), f"layer array {i} is not prognostic"
                assert diff.max() < na, "an inactive layer was touched"
        from samsim_amd.capi import SCALARS
        for i, n in enumerate(SCALARS):
            if st.scal[i, col] != clean.scal[i, col]:
                changed = True
                assert n in ss.SNOW, f"scalar {n} is not a snow scalar"
        assert changed


def test_every_seed_stops_the_oracle_with_its_code(capsys):
    rows = []
    for seed in ss.SEEDS:
        for col in (ss.COLUMNS if seed.gpu else ss.COLUMNS[:1]):
            o, cfg, st, clock = ss.run_oracle(seed, col)
            status, step, layer = o.get_status()
            o.close()
            rel = int(step[col]) - clock["step"]
            rows.append((seed.site, seed.name, col, int(status[col]), rel, int(layer[col]), int(st.n_active[col])))
            assert status[col] == seed.code, f"{seed.name}, column {col}: the oracle reports {status[col]}, the seed aims at {seed.code}"
            assert seed.min_step <= rel <= ss.MAX_STEPS, f"{seed.name}: stops in step {rel}"
            assert not np.delete(status, col).any(), f"{seed.name}: a healthy column stopped"
            if seed.layer is not None:
                assert layer[col] == seed.layer, f"{seed.name}: layer {layer[col]}, the contract says {seed.layer}"
            else:
                assert 1 <= layer[col] <= st.n_active[col]
    with capsys.disabled():
        print("\n%-24s %-30s %3s %5s %4s %5s  (k mod 3, N_active)" % ("site", "seed", "col", "code", "step", "layer"))
        for site, name, col, code, rel, lay, na in rows:
            print("%-24s %-30s %3d %5d %4d %5d  (%d, %d)" % (site, name, col, code, rel, lay, lay % 3, na))


def test_the_clean_ensembles_do_not_stop():
    """the replicas are healthy: what a seed's run reports is the mutation's doing"""
    seen = set()
    for seed in ss.SEEDS:
        key = (seed.fixture, seed.config)
        if key in seen:
            continue
        seen.add(key)
        o, *_ = ss.run_oracle(seed, mutated=False)
        assert not o.get_status()[0].any(), key
        o.close()


def stopc_sites():
    """(file, code as written) of every STOPC(...) in the step kernel's source -- and of the one stop written out by hand
    (`c.status = rcc;` in the fused down sweep) -- in source order; the macro's definition and comments excluded"""
    out = []
    for fn in sorted(os.listdir(CSRC)):
        if not fn.endswith((".h", ".hip", ".cpp")):
            continue
        for line in open(os.path.join(CSRC, fn)):
            code = line.split("//")[0]
            if "#define" in code:
                continue
            for m in re.finditer(r"\bSTOPC\(\s*(\w+)\s*,|\bc\.status = (\w+);", code):
                out.append((fn, m.group(1) or m.group(2)))
    return out


def test_site_table_names_every_stopc_of_the_source():
    found = stopc_sites()
    table = [(f, c) for f, c, _, _ in ss.SITES]
    assert len(found) == 17, found
    assert sorted(found) == sorted(table), (sorted(found), sorted(table))
    seeded = set()
    for f, c, what, how in ss.SITES:
        if isinstance(how, list):
            assert how and all(n in ss.BY_NAME for n in how), (f, c)
            seeded.update(how)
        else:
            assert isinstance(how, str) and len(how) > 20, f"{f} STOPC({c}): neither a seed nor a reason"
    assert seeded == set(ss.BY_NAME), "a seed that no site lists, or the other way round"


def test_header_states_the_layer_contract():
    text = open(os.path.join(ROOT, "include", "samsim.h")).read()
    i = text.index("int samsim_get_status(")
    doc = text[text.rindex("/*", 0, i):i]
    rows = [ln for ln in doc.splitlines() if re.match(r"^ \*   \d+ ", ln)]
    codes = [int(ln.split()[1]) for ln in rows]
    # one row per (code, site): the 17 stop sites of the source fall on these 14 rows (fused and unfused order share theirs)
    assert sorted(codes) == sorted([99, 99, 99, 16, 99, 345, 9876, 21234, 1337, 431, 9876, 9876, 7889, 1337]), codes
    for code, last in ((431, "0"), (7889, "0"), (345, "0"), (16, "1")):
        assert [ln.split()[-1] for ln in rows if int(ln.split()[1]) == code] == [last], code
    assert "LARGEST k" in doc and "SMALLEST k" in doc
    # the seeds' layers are the table's
    for seed in ss.SEEDS:
        if seed.code in (431, 7889, 1337) or seed.name == "snow_99":
            assert seed.layer == 0, seed.name
        if seed.code == 16 or seed.name == "coupling_99":
            assert seed.layer == 1, seed.name
