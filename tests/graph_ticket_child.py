"""Helper of tests/test_graphed_ops_gpu.py::test_graph_ticket_pool_fallbacks_in_a_fresh_process (not collected): the two
fallbacks of the folded finalisation's ticket pool (csrc/scan_ops.hip: scan_ticket) that only a fresh process can reach.
Prints one JSON line; the test asserts on it.

(a) cold base: the first folded launch of the process is a captured one.  The ticket array's address is not known yet and a
    symbol lookup is refused inside a capture, so the launch gets no ticket and the graph holds scan + finalize.
(b) exhaustion: one capture of 3100 folded launches asks for more graph tickets than the pool has; from the first launch
    without one the graph holds scan + finalize, with the same bits."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "di-hpc_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import cabi  # noqa: E402
from hpc_rll.rl_utils.gae import GAE  # noqa: E402
from hpc_rll.rl_utils.td import TDLambda  # noqa: E402

DEV = torch.device("cuda:0")
NAN = float("nan")


def record():
    """(launches so far, workgroups, how) of the TD(lambda) dispatch record"""
    out = (ctypes.c_int * 11)()                     # HPC_RLL_SCAN_CONFIG_INTS
    assert cabi.lib.hpc_rll_scan_last_config(0, out) == 0          # HPC_RLL_SCAN_OP_TD_LAMBDA
    return out[0], out[9], out[10]


def fresh(g, T, B):
    return torch.randn(T + 1, B, device=DEV, generator=g), torch.randn(T, B, device=DEV, generator=g)


def cold_base(g):
    T, B = 16, 2048
    value, reward = fresh(g, T, B)
    td = TDLambda(T, B)
    with torch.no_grad():
        GAE(T, B)(value, reward)                    # loads the library's device code; a GAE has no loss and takes no ticket
        torch.cuda.synchronize()
        assert record()[0] == 0
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            loss = td(value, reward)
        launches, grid, how = record()
        assert launches == 1
        v2, r2 = fresh(g, T, B)
        value.copy_(v2)
        reward.copy_(r2)
        loss.fill_(NAN)
        graph.replay()
        eager = td(value, reward)
        torch.cuda.synchronize()
    return dict(how_captured=how, workgroups=grid, how_eager_afterwards=record()[2],
                replay_equals_eager=bool(torch.equal(loss, eager)), loss=loss.item())


def exhaustion(g):
    T, B, n = 8, 2048, 3100
    value, reward = fresh(g, T, B)
    td = TDLambda(T, B)
    outs, hows = [], []
    with torch.no_grad():
        td(value, reward)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(n):
                outs.append(td(value, reward))
                hows.append(record()[2])
        grid = record()[1]
        first = hows.index(2) if 2 in hows else -1
        res = dict(launches=n, workgroups=grid, first_fallback=first,
                   folded_before=first >= 0 and all(h == 1 for h in hows[:first]),
                   fallback_from_there_on=first >= 0 and all(h == 2 for h in hows[first:]))
        for k in ("replay_1", "replay_2"):
            v2, r2 = fresh(g, T, B)
            value.copy_(v2)
            reward.copy_(r2)
            for o in outs:
                o.fill_(NAN)
            graph.replay()
            got = torch.cat(outs)
            eager = td(value, reward)
            torch.cuda.synchronize()
            res[k] = dict(all_outputs_equal=bool((got == got[0]).all()), equals_eager=bool(torch.equal(got, eager.expand_as(got))),
                          loss=eager.item())
        res["how_eager_afterwards"] = record()[2]
    return res


def main():
    g = torch.Generator(device=DEV).manual_seed(11)
    out = dict(cold_base=cold_base(g))
    out["exhaustion"] = exhaustion(g)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
