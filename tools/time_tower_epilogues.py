#!/usr/bin/env python3
"""Event-timed dfm_linear_backward launches at the headline tower shapes (B = 4096, 624 -> 256 -> 128 -> 64) with each
d-input epilogue: plain store, the lower layer's BatchNorm mask (bn_below) and the FM backward (fm), for parts = 2 (d
input alone) and parts = 3 (the step's launch: d weight + d input).  Every launch takes the next of SETS buffer sets
(inputs, outputs and epilogue operands; >= 8), so z, e and the other operands come from memory that the previous
SETS - 1 launches have pushed through the L2s, as in the step, and not from a warm L2 as in a loop over one set.
The step runs: layer 3 and 2 with bn_below, layer 1 with fm.

The library comes from DFM_LIB_PATH (tools/build_variant.sh; unset: the product), so two builds alternate as two
runs of this tool.  One JSON line on stdout.
usage: python tools/time_tower_epilogues.py [iters=400] [sets=8]"""
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deepfm_amd import _lib  # noqa: E402

B, DIMS, FM_DIM = 4096, (624, 256, 128, 64), 16


def make_set(lib, g, K, N):
    """One buffer set of a layer: everything a launch of any epilogue reads or writes."""
    dev = "cuda"
    s = dict(dz=torch.randn(B, N, device=dev, generator=g) * 1e-3, x=torch.randn(B, K, device=dev, generator=g),
             w=torch.randn(N, K, device=dev, generator=g) / K ** 0.5, gx=torch.empty(B, K, device=dev),
             slabs=torch.zeros(max(lib.dfm_linear_backward_workspace_bytes(B, N, K) // 4, 1), device=dev),
             z=torch.randn(B, K, device=dev, generator=g), dy=torch.empty(B, K, device=dev),
             stats=torch.cat([torch.zeros(K, device=dev), torch.ones(K, device=dev)]),
             gamma=torch.ones(K, device=dev), beta=torch.zeros(K, device=dev), gg=torch.zeros(K, device=dev),
             gb=torch.zeros(K, device=dev), ws=torch.zeros(lib.dfm_bn_bwd_workspace_bytes(B, K) // 4, device=dev),
             g_fm=torch.randn(B, device=dev, generator=g) * 1e-3, S=torch.randn(B, FM_DIM, device=dev, generator=g))
    bn = _lib.BnBwd()
    bn.z, bn.mean_rstd, bn.gamma, bn.beta = (s[k].data_ptr() for k in ("z", "stats", "gamma", "beta"))
    bn.dy, bn.g_gamma, bn.g_beta, bn.workspace = (s[k].data_ptr() for k in ("dy", "gg", "gb", "ws"))
    bn.seed, bn.p_drop, bn.salt = None, 0.0, 0
    fm = _lib.FmBwd()
    fm.g_fm, fm.fm_sum, fm.e, fm.addend, fm.dim = s["g_fm"].data_ptr(), s["S"].data_ptr(), s["x"].data_ptr(), None, FM_DIM
    s["bn"], s["fm"] = bn, fm
    return s


def timed(fn, iters, sets):
    for i in range(2 * sets):
        fn(i % sets)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(iters):
        fn(i % sets)
    b.record()
    torch.cuda.synchronize()
    return round(a.elapsed_time(b) / iters * 1e3, 2)


def main():
    iters = int(sys.argv[1]) if len(sys.argv) > 1 else 400
    sets = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    assert sets >= 1 and iters >= sets
    lib = _lib.load()
    st = _lib.stream_handle()
    g = torch.Generator(device="cuda").manual_seed(0)
    out = {"lib": os.path.basename(_lib.LIB_PATH), "iters": iters, "sets": sets, "us": {}}
    for layer in (3, 2, 1):
        K, N = DIMS[layer - 1], DIMS[layer]
        pool = [make_set(lib, g, K, N) for _ in range(sets)]
        for epi in ("plain", "bn_below", "fm"):
            for parts in (2, 3):
                def run(i):
                    s = pool[i]
                    _lib.check(lib.dfm_linear_backward(
                        s["dz"].data_ptr(), B, N, s["x"].data_ptr(), K, s["w"].data_ptr(), s["gx"].data_ptr(),
                        C.byref(s["bn"]) if epi == "bn_below" else None, C.byref(s["fm"]) if epi == "fm" else None,
                        parts, s["slabs"].data_ptr(), st))
                out["us"][f"L{layer}_{K}x{N}_{epi}_parts{parts}"] = timed(run, iters, sets)
        del pool
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
