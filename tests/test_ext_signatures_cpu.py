"""The pybind surface of the three compiled extension modules: the ``__doc__`` of every callable -- its name, parameter
names, C++ parameter types, defaults and doc text as pybind renders them -- equals the record in
tests/golden/ext_signatures.json (written only by ``tests/golden/make_golden.py ext_signatures``).  The glue may state a
signature however it likes; what Python sees must not move with it."""
import importlib
import json
import os

import pytest

from conftest import ROOT

SNAP = os.path.join(ROOT, "tests", "golden", "ext_signatures.json")
MODULES = ["hpc_rl_utils", "hpc_torch_utils_network", "hpc_models"]


def current_signatures():
    out = {}
    for mod in MODULES:
        m = importlib.import_module(mod)
        out[mod] = {n: getattr(m, n).__doc__ for n in dir(m) if not n.startswith("__") and callable(getattr(m, n))}
    return out


@pytest.mark.parametrize("mod", MODULES)
def test_docstrings_match_the_record(mod):
    want, got = json.load(open(SNAP))[mod], current_signatures()[mod]
    assert want, mod
    assert sorted(got) == sorted(want), sorted(set(got) ^ set(want))
    for name in sorted(want):
        assert got[name] == want[name], f"{mod}.{name}:\n{got[name]}\n-- recorded --\n{want[name]}"
