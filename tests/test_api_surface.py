"""Drop-in boundary: the public Python surface equals the reference's.

When /root/reference is present (build container) the reference's L1 sources are PARSED (ast, never imported or
executed -- they need the CUDA extension) and every public class / function there must exist here with the same
positional parameter names and defaults for ``__init__`` and ``forward`` (extra trailing keyword parameters such as
``sharded`` / ``group`` are allowed).  On the GPU box the reference is absent and the comparison runs against the
snapshot recorded in tests/golden/api_surface.json (written by this test in the build container)."""
import ast
import importlib
import inspect
import json
import os

import pytest

from conftest import ROOT

REF = "/root/reference"
SNAP = os.path.join(ROOT, "tests", "golden", "api_surface.json")
MODULES = ["hpc_rll.rl_utils.gae", "hpc_rll.rl_utils.td", "hpc_rll.rl_utils.vtrace", "hpc_rll.rl_utils.upgo",
           "hpc_rll.rl_utils.ppo", "hpc_rll.rl_utils.padding", "hpc_rll.torch_utils.network.rnn",
           "hpc_rll.torch_utils.network.scatter_connection"]


def _sig(fn: ast.FunctionDef):
    args = [a.arg for a in fn.args.args]
    defaults = [ast.unparse(d) for d in fn.args.defaults]
    pad = [None] * (len(args) - len(defaults)) + defaults
    return [[a, d] for a, d in zip(args, pad) if a not in ("self", "ctx")]


def reference_surface():
    out = {}
    for mod in MODULES:
        path = os.path.join(REF, *mod.split(".")) + ".py"
        tree = ast.parse(open(path).read())
        entry = {}
        for node in tree.body:
            if isinstance(node, ast.ClassDef) and any(getattr(b, "attr", getattr(b, "id", "")) == "Module" for b in node.bases):
                meths = {f.name: _sig(f) for f in node.body if isinstance(f, ast.FunctionDef) and f.name in ("__init__", "forward")}
                entry[node.name] = meths
            elif isinstance(node, ast.FunctionDef) and not node.name.startswith("_") and node.name != "cum":
                entry[node.name] = {"__call__": _sig(node)}
        out[mod] = entry
    return out


def load_surface():
    """The committed snapshot (written only by tests/golden/make_golden.py api_surface); never rewritten by a test."""
    return json.load(open(SNAP))


def test_snapshot_is_current():
    """The committed snapshot covers exactly MODULES, every entry in the form reference_surface() writes: module classes
    with ``__init__`` / ``forward``, public functions with ``__call__``, each a list of [name, default or None] with no
    required parameter after a defaulted one.  Where the reference tree is present, it must also equal a fresh parse."""
    snap = load_surface()
    assert sorted(snap) == sorted(MODULES)
    for mod, entry in snap.items():
        assert entry, mod
        for name, meths in entry.items():
            assert meths and (set(meths) <= {"__init__", "forward"} or set(meths) == {"__call__"}), (mod, name, meths)
            for mname, params in meths.items():
                names = [p[0] for p in params]
                assert all(len(p) == 2 and isinstance(p[0], str) and p[0].isidentifier() for p in params), (mod, name, mname)
                assert len(set(names)) == len(names), (mod, name, mname, names)
                defaulted = [p[1] is not None for p in params]
                assert defaulted == sorted(defaulted), f"{mod}.{name}.{mname}: required parameter after a defaulted one"
    if os.path.isdir(REF):
        assert json.loads(json.dumps(reference_surface(), sort_keys=True)) == snap


def _norm(d):
    if d is None:
        return None
    return d.replace("'", '"').replace("0.0", "0.").rstrip("0") if isinstance(d, str) else d


@pytest.mark.parametrize("mod", MODULES)
def test_public_surface_matches_reference(mod):
    surf = load_surface()[mod]
    ours = importlib.import_module(mod)
    assert surf, mod
    for name, meths in surf.items():
        assert hasattr(ours, name), f"{mod}.{name} missing"
        obj = getattr(ours, name)
        for mname, ref_params in meths.items():
            fn = obj if mname == "__call__" else getattr(obj, mname)
            params = [p for p in inspect.signature(fn).parameters.values() if p.name not in ("self",)]
            assert len(params) >= len(ref_params), (mod, name, mname)
            for (rname, rdef), p in zip(ref_params, params):
                assert p.name == rname, f"{mod}.{name}.{mname}: parameter {p.name!r} != reference {rname!r}"
                if rdef is None:
                    assert p.default is inspect.Parameter.empty, (mod, name, mname, rname)
                else:
                    assert p.default is not inspect.Parameter.empty, (mod, name, mname, rname)
                    assert float(p.default) == float(eval(rdef)) if rdef.replace(".", "").replace("-", "").isdigit() else \
                        repr(p.default).strip("'\"") == rdef.strip("'\""), (mod, name, mname, rname, rdef, p.default)
            for p in params[len(ref_params):]:       # anything extra must be optional
                assert p.default is not inspect.Parameter.empty, (mod, name, mname, p.name)


def test_native_module_names_match_reference():
    """The three extension modules and their entry points (src/*/entry.cpp) exist under the reference's names."""
    import hpc_models
    import hpc_rl_utils
    import hpc_torch_utils_network
    rl = ["GaeForward", "TdLambdaForward", "TdLambdaBackward", "DistNStepTdForward", "DistNStepTdBackward",
          "QNStepTdForward", "QNStepTdBackward", "QNStepTdRescaleForward", "QNStepTdRescaleBackward",
          "IQNNStepTDErrorForward", "IQNNStepTDErrorBackward", "QRDQNNStepTDErrorForward", "QRDQNNStepTDErrorBackward",
          "VTraceForward", "VTraceBackward", "UpgoForward", "UpgoBackward", "PPOForward", "PPOBackward",
          "Pad1DForward", "GroupPad1DForward", "Unpad1DForward", "Pad2DForward", "GroupPad2DForward", "Unpad2DForward",
          "Pad3DForward", "GroupPad3DForward", "Unpad3DForward", "sample_split_group", "oracle_split_group"]
    for n in rl:
        assert callable(getattr(hpc_rl_utils, n)), n
    for n in ["LstmForward", "LstmBackward", "ScatterConnectionForward", "ScatterConnectionBackward"]:
        assert callable(getattr(hpc_torch_utils_network, n)), n
    for n in ["actor_critic_update_ae", "actor_critic_lstm_activation", "actor_critic_pre_sample"]:
        assert callable(getattr(hpc_models, n)), n
    if os.path.isdir(REF):   # cross-check the list itself against the reference's pybind registrations
        import re
        defs = re.findall(r'm\.def\("(\w+)"', open(os.path.join(REF, "src/rl_utils/entry.cpp")).read())
        assert sorted(defs) == sorted(rl), sorted(set(defs) ^ set(rl))
