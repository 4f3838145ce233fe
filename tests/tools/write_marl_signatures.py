#!/usr/bin/env python3
"""Writes tests/golden/ext_signatures_marl.json: the pybind docstring of every callable of the built ``hpc_marl`` module, what
tests/test_qmix_cpu.py compares a build against (the counterpart of ``tests/golden/make_golden.py ext_signatures`` for the
fourth extension module).  Names and docstrings only.  Written ONLY here."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "di-hpc_amd"))

import hpc_marl  # noqa: E402

SNAP = os.path.join(ROOT, "tests", "golden", "ext_signatures_marl.json")
sigs = {n: getattr(hpc_marl, n).__doc__ for n in dir(hpc_marl) if not n.startswith("__") and callable(getattr(hpc_marl, n))}
json.dump({"hpc_marl": sigs}, open(SNAP, "w"), indent=1, sort_keys=True)
print("wrote", SNAP)
