#!/usr/bin/env python3
"""Writes tests/golden/ext_signatures_sac.json: the pybind docstring of every callable of the built ``hpc_sac`` module, what
tests/test_sac_continuous_cpu.py compares a build against (the counterpart of tests/tools/write_twohot_signatures.py for the
seventh extension module).  Names and docstrings only.  Written ONLY here."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "di-hpc_amd"))

import torch  # noqa: E402,F401  (libtorch must be loaded before the extension module)
import hpc_sac  # noqa: E402

SNAP = os.path.join(ROOT, "tests", "golden", "ext_signatures_sac.json")
sigs = {n: getattr(hpc_sac, n).__doc__ for n in dir(hpc_sac) if not n.startswith("__") and callable(getattr(hpc_sac, n))}
json.dump({"hpc_sac": sigs}, open(SNAP, "w"), indent=1, sort_keys=True)
print("wrote", SNAP)
