"""LDS is handed out in allocation granules (measured: tools/lds_residency.hip -> profiles/lds_residency.json), so the workgroups per CU
a kernel is built for must fit when every workgroup's LDS is rounded up to the granule.  Checked on the kernel metadata of the built
library, read the way tools/kres.py --lib reads it: the LDS-form traversal kernels at six, the quad-form ones with the tree's top in
LDS at five, the fused tail and the shade kernels at two."""
import importlib.util
import json
import os
import re

import pytest

from conftest import ROOT

LDS_PER_CU = 163840


@pytest.fixture(scope="module")
def granule():
    j = json.load(open(os.path.join(ROOT, "profiles", "lds_residency.json")))
    by_size = {r["lds_bytes"]: r["resident_wgs_per_cu"] for r in j["rows"]}
    assert by_size[26880] == 6 and by_size[27136] == 5  # what the accounting rests on: 21 granules fit six times, 22 do not
    assert j["granule"] in j["granules_consistent"]
    return int(j["granule"])


@pytest.fixture(scope="module")
def kernels(ptrs):
    spec = importlib.util.spec_from_file_location("kres", os.path.join(ROOT, "tools", "kres.py"))
    kres = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kres)
    build = importlib.import_module("pathtracer-rs_amd.build")
    k = kres.library_kernels(build.LIB, build.HIPCC)
    assert len(k) > 100
    return k


def _alloc(lds, granule):
    return -(-lds // granule) * granule


def _trav(kernels):
    for name, r in kernels.items():
        m = re.match(r"k_(extend|connect)_rf<(\d+), (\d+), (true|false), (\d+), (true|false)>$", name)
        if m:
            yield name, int(m.group(3)), int(m.group(5)), r["lds"]


def test_lds_form_kernels_fit_six_workgroups(kernels, granule):
    forms = set()
    for name, depth, geom, lds in _trav(kernels):
        if geom > 0 and geom != 1536:  # (the 1 536-vector form is built for four: 40 960 B)
            assert 6 * _alloc(lds, granule) <= LDS_PER_CU, (name, lds)
            forms.add((depth, geom))
        elif geom == 1536:
            assert 4 * _alloc(lds, granule) <= LDS_PER_CU, (name, lds)
    assert forms == {(8, 640), (9, 528)}


def test_quad_form_kernels_fit_five_workgroups(kernels, granule):
    n = 0
    for name, depth, geom, lds in _trav(kernels):
        if geom == 0 and depth == 8:
            assert 5 * _alloc(lds, granule) <= LDS_PER_CU, (name, lds)
            n += 1
    assert n >= 12


def test_tail_and_shade_kernels_fit_two_workgroups(kernels, granule):
    names = [n for n in kernels if n.startswith("k_tail<") or n.startswith("k_shade<")]
    assert any(n.startswith("k_tail<0, 0, 528, false, 9>") for n in names) and "k_shade<0, 0, false>" in names
    for n in names:
        assert 2 * _alloc(kernels[n]["lds"], granule) <= LDS_PER_CU, (n, kernels[n]["lds"])
