"""TEST-ONLY: the LayerNorm-LSTM's C entry points called directly (tests/cabi.py) on buffers the test owns.

Every operand lies in its own ``guarded.GuardedF32``: inputs at a chosen number of floats past a 16-byte boundary, outputs
prefilled with NaN, the workspace exactly ``hpc_rll_lstm_workspace_floats`` floats long and prefilled with zeros, quiet NaN
or the guard sentinel.  ``LstmCall.check_all()`` asserts after each call that no guard band moved, that no input changed,
that a successful call wrote all of its outputs and that a refused one wrote none.
"""
import functools

import numpy as np
import torch

import cabi
import guarded
from oracle import ref_torch as R

DEV = torch.device("cuda:0")
OK, EINVAL, EALIGN, EUNSUPPORTED = 0, -1, -2, -3            # include/hpc_rll_hip.h

INPUTS = ("x", "h0", "c0", "wx", "wh", "bias", "ln_gamma", "ln_beta", "dy", "dhn", "dcn")
FWD_OUT = ("y", "hn", "cn")
BWD_OUT = ("dx", "dh0", "dc0", "dwx", "dwh", "dbias", "dln_gamma", "dln_beta")
FWD_ARGS = ("x", "h0", "c0", "wx", "wh", "bias", "ln_gamma", "ln_beta", "y", "hn", "cn", "ws")
BWD_ARGS = ("dy", "dhn", "dcn", "x", "h0", "c0", "wx", "wh", "ln_gamma", "ws", "dx", "dh0", "dc0", "dwx", "dwh", "dbias",
            "dln_gamma", "dln_beta")


def sizes(S, B, I, H, L):
    G = 4 * H
    nwx = (I + (L - 1) * H) * G
    return dict(x=S * B * I, h0=L * B * H, c0=L * B * H, wx=nwx, wh=L * H * G, bias=L * G, ln_gamma=L * 2 * G,
                ln_beta=L * 2 * G, dy=S * B * H, dhn=L * B * H, dcn=L * B * H, y=S * B * H, hn=L * B * H, cn=L * B * H,
                dx=S * B * I, dh0=L * B * H, dc0=L * B * H, dwx=nwx, dwh=L * H * G, dbias=L * G, dln_gamma=L * 2 * G,
                dln_beta=L * 2 * G)


@functools.lru_cache(maxsize=4)
def make_inputs(S, B, I, H, L, seed):
    """The draws of test_lstm_oracle: weights uniform +-1/sqrt(H), gamma 1 + 0.1 N, beta 0.1 N, the rest standard normal.
    Flat float32 tensors on the device, in the C ABI's layouts."""
    rng = np.random.default_rng(seed)
    gain = 1.0 / np.sqrt(H)
    dims = [I] + [H] * L
    wx = [rng.uniform(-gain, gain, (dims[l], 4 * H)).astype(np.float32) for l in range(L)]
    wh = [rng.uniform(-gain, gain, (H, 4 * H)).astype(np.float32) for l in range(L)]
    d = dict(wx=np.concatenate([w.reshape(-1) for w in wx]), wh=np.concatenate([w.reshape(-1) for w in wh]))
    d["bias"] = rng.uniform(-gain, gain, (L, 4 * H)).astype(np.float32)
    d["ln_gamma"] = (1 + 0.1 * rng.standard_normal((L, 8 * H))).astype(np.float32)
    d["ln_beta"] = (0.1 * rng.standard_normal((L, 8 * H))).astype(np.float32)
    for k, s in (("x", (S, B, I)), ("h0", (L, B, H)), ("c0", (L, B, H)), ("dy", (S, B, H)), ("dhn", (L, B, H)),
                 ("dcn", (L, B, H))):
        d[k] = rng.standard_normal(s).astype(np.float32)
    return {k: torch.from_numpy(np.ascontiguousarray(v.reshape(-1))).to(DEV) for k, v in d.items()}


@functools.lru_cache(maxsize=None)
def oracle(S, B, I, H, L, seed):
    """oracle.ref_torch.lstm in float64 on the inputs of make_inputs, gradients by autograd: flat float64 tensors under the
    C ABI's output names.  Computed once per shape and shared (never modified)."""
    src = make_inputs(S, B, I, H, L, seed)
    G = 4 * H
    leaf = lambda name, *shape: src[name].double().view(*shape).requires_grad_(True)  # noqa: E731
    x, h0, c0 = leaf("x", S, B, I), leaf("h0", L, B, H), leaf("c0", L, B, H)
    bias, gamma, beta = leaf("bias", L, G), leaf("ln_gamma", L, 2 * G), leaf("ln_beta", L, 2 * G)
    wx, wh, o = [], [], 0
    for l in range(L):
        n = (I if l == 0 else H) * G
        wx.append(src["wx"][o:o + n].double().view(-1, G).requires_grad_(True))
        wh.append(src["wh"][l * H * G:(l + 1) * H * G].double().view(H, G).requires_grad_(True))
        o += n
    y, hn, cn = R.lstm(x, h0, c0, wx, wh, bias, gamma, beta)
    ((y * src["dy"].double().view_as(y)).sum() + (hn * src["dhn"].double().view_as(hn)).sum()
     + (cn * src["dcn"].double().view_as(cn)).sum()).backward()
    out = dict(y=y, hn=hn, cn=cn, dx=x.grad, dh0=h0.grad, dc0=c0.grad, dwx=torch.cat([w.grad.reshape(-1) for w in wx]),
               dwh=torch.cat([w.grad.reshape(-1) for w in wh]), dbias=bias.grad, dln_gamma=gamma.grad, dln_beta=beta.grad)
    return {k: v.detach().reshape(-1).clone() for k, v in out.items()}


def nerr(ref, got):
    """test_lstm_oracle's metric: max |ref - got| / max(max |ref|, 1e-3) of the tensor."""
    ref = ref.double().reshape(-1)
    return float((ref - got.double().reshape(-1)).abs().max()) / max(float(ref.abs().max()), 1e-3)


def saved_floats(S, B, I, H, L, p):
    """(floats at the head of the workspace that hold what the forward saves for the backward -- per layer xw, hw, gates,
    c, hseq, stats, xin_next, then pstash --, offset of the last layer's hseq) from the layout the header documents; every
    region is rounded up to 4 floats.  The second figure must equal hpc_rll_lstm_workspace_y_offset."""
    r4 = lambda n: (n + 3) // 4 * 4  # noqa: E731
    SB, G = S * B, 4 * H
    recompute = B * H >= 1 << 19                      # the gates are not saved, bias / beta are parked in pstash
    off, yoff = 0, -1
    for l in range(L):
        off += 2 * r4(SB * G) + (0 if recompute else r4(SB * G)) + r4(SB * H)
        if l == L - 1:
            yoff = off
        off += r4(SB * H) + r4(SB * 4) + (r4(SB * H) if p > 0 and l < L - 1 else 0)
    return off + (r4(L * 3 * G) if recompute else 0), yoff


class LstmCall:
    """One set of guarded operands for hpc_rll_lstm_forward* / _backward*.

    off:     floats past a 16-byte boundary, one int for every operand (workspace and outputs included) or {name: floats}
             (names of INPUTS, FWD_OUT, BWD_OUT and "ws"; 0 for the others).
    ws_fill: "zero" | "nan" | "sentinel".
    y_mode:  "plain" forward + backward; "ext" forward_y / backward_y with a guarded y of its own; "ws" forward_y /
             backward_y with y = ws + hpc_rll_lstm_workspace_y_offset.
    nulls:   of "dy", "dhn", "dcn", "dx": passed as NULL.   zeros: of "dy", "dhn", "dcn": explicit zero tensors.
    """

    def __init__(self, S, B, I, H, L, p=0.0, seed=0, *, off=0, ws_fill="nan", y_mode="plain", nulls=(), zeros=()):
        self.shape, self.p, self.y_mode, self.nulls = (S, B, I, H, L), float(p), y_mode, tuple(nulls)
        self.dropout_seed = 0x9E3779B97F4A7C15 ^ seed
        o = (lambda name: off) if isinstance(off, int) else (lambda name: off.get(name, 0))
        n = sizes(S, B, I, H, L)
        src = make_inputs(S, B, I, H, L, seed)
        self.src = {k: (torch.zeros_like(src[k]) if k in zeros else src[k]) for k in INPUTS}
        self.g = {k: guarded.GuardedF32(1, n[k], o(k), DEV, src=self.src[k].view(1, -1)) for k in INPUTS}
        for k in FWD_OUT + BWD_OUT:
            if not (k == "y" and y_mode == "ws"):
                self.g[k] = guarded.GuardedF32(1, n[k], o(k), DEV)
        self.ws_floats = cabi.lib.hpc_rll_lstm_workspace_floats(S, B, I, H, L, self.p)
        self.y_offset = cabi.lib.hpc_rll_lstm_workspace_y_offset(S, B, I, H, L, self.p)
        assert self.ws_floats > 0 and 0 <= self.y_offset and self.y_offset + n["y"] <= self.ws_floats
        ws = self.g["ws"] = guarded.GuardedF32(1, self.ws_floats, o("ws"), DEV)
        if ws_fill == "zero":
            ws.t.zero_()
        elif ws_fill == "sentinel":
            ws.t.view(torch.int32).fill_(guarded.SENTINEL32)
        else:
            assert ws_fill == "nan"
        self.y = ws.t[0, self.y_offset:self.y_offset + n["y"]] if y_mode == "ws" else self.g["y"].t[0]
        self.fwd_status = self.bwd_status = None
        self.fwd_path = self.bwd_path = None
        self.ws_after_fwd = self.fwd_out = None

    def ptr(self, name, shift=None):
        if name in self.nulls:
            return None
        p = self.y.data_ptr() if name == "y" else self.g[name].t.data_ptr()
        return p + 4 * (shift or {}).get(name, 0)

    def out(self, name):
        return self.y if name == "y" else self.g[name].t[0]

    def forward(self):
        S, B, I, H, L = self.shape
        fn = cabi.lib.hpc_rll_lstm_forward if self.y_mode == "plain" else cabi.lib.hpc_rll_lstm_forward_y
        self.fwd_status = fn(*[self.ptr(k) for k in FWD_ARGS], S, B, I, H, L, self.p, self.dropout_seed, cabi.stream_ptr(DEV))
        self.fwd_path = cabi.lib.hpc_rll_lstm_last_forward_path()
        torch.cuda.synchronize()
        self.async_error = cabi.lib.hpc_rll_async_error()
        self.ws_after_fwd = self.g["ws"].raw.clone()
        self.fwd_out = {k: self.out(k).clone() for k in FWD_OUT}
        return self.fwd_status

    def backward(self, plain=None, shift=None):
        """plain=True: hpc_rll_lstm_backward whatever the y mode (the pairing test).  shift: {argument: floats} added to
        that pointer (refusal tests: the argument is passed off its boundary without moving the data)."""
        S, B, I, H, L = self.shape
        plain = self.y_mode == "plain" if plain is None else plain
        args = [self.ptr(k, shift) for k in BWD_ARGS]
        if plain:
            fn = cabi.lib.hpc_rll_lstm_backward
        else:
            fn = cabi.lib.hpc_rll_lstm_backward_y
            args.insert(BWD_ARGS.index("ws"), self.ptr("y", shift))
        self.bwd_status = fn(*args, S, B, I, H, L, self.p, self.dropout_seed, cabi.stream_ptr(DEV))
        self.bwd_path = cabi.lib.hpc_rll_lstm_last_backward_path()
        torch.cuda.synchronize()
        self.async_error = cabi.lib.hpc_rll_async_error()
        return self.bwd_status

    def reset_grads(self):
        for k in BWD_OUT:
            self.g[k].t.fill_(float("nan"))
        self.bwd_status = None

    def check_all(self, what=""):
        what = f"{what} {self.shape}"
        for k, g in self.g.items():
            g.check(f"{what} {k}")
        for k in INPUTS:
            assert torch.equal(self.g[k].t[0].view(torch.int32), self.src[k].view(torch.int32)), f"{what}: input {k} was modified"
        if self.fwd_status is not None:
            for k in FWD_OUT:
                t = self.out(k)
                if self.fwd_status == OK:
                    assert not bool(torch.isnan(t).any()), f"{what}: {k} holds NaN after the forward"
                    if self.bwd_status is not None:   # (y inside the workspace included: the backward only reads it)
                        assert torch.equal(t, self.fwd_out[k]), f"{what}: the backward changed {k}"
                elif k != "y" or self.y_mode != "ws":
                    assert bool(torch.isnan(t).all()), f"{what}: a refused forward wrote to {k}"
        for k in BWD_OUT:
            if self.bwd_status == OK and k not in self.nulls:
                self.g[k].assert_written(f"{what} {k}")
            else:
                self.g[k].assert_untouched(f"{what} {k}")

    def outputs(self):
        names = FWD_OUT + tuple(k for k in BWD_OUT if k not in self.nulls)
        return {k: self.out(k).clone() for k in names}


def run(S, B, I, H, L, p=0.0, seed=0, *, off=0, ws_fill="nan", y_mode="plain", nulls=(), zeros=()):
    """Forward and backward on fresh guarded buffers, check_all() after each.  Returns the LstmCall (statuses, paths,
    guard objects, workspace snapshot) and clones of its outputs."""
    c = LstmCall(S, B, I, H, L, p, seed, off=off, ws_fill=ws_fill, y_mode=y_mode, nulls=nulls, zeros=zeros)
    assert c.forward() == OK, c.fwd_status
    assert c.async_error == 0
    c.check_all("after the forward")
    assert c.backward() == OK, c.bwd_status
    assert c.async_error == 0
    c.check_all("after the backward")
    return c, c.outputs()
