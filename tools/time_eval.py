"""Eval-mode forward time: the default path against the fused plans (Settings.fused_eval), in ONE process.

    python tools/time_eval.py [--rounds 5] [--seconds 1.0] [--shapes 32x1x256x256,2x1x256x256,1x3x512x512] [--json out.json]
    python tools/time_eval.py --profile-run 32x1x256x256 [--path fused]     # one path's forwards only: the workload of a kernel-trace run

Paths: "default" (Settings()), "fused" (fused_eval=True: fp16 hi | mid slots), "bf16" (fused_eval="bf16" under conv == "auto": one-part
bf16 slots, depth by the fill rule) and "bf16/bf16" (the same under conv == "bf16": every legal level) time the forward `m(X)`.
Labels-only paths time a call that returns the labels alone: "fused:segment" and "bf16/bf16:segment" are `segment(m, X)` under the
settings of "fused" / "bf16/bf16", "fused+head" and "bf16/bf16+head" are `segment(m, X, head="fused")` under the same settings (the
head in the last convolution's epilogue).
"+pool" paths -- "fused+pool", "bf16+pool", "bf16/bf16+pool" and the labels-only "fused+pool+head", "bf16/bf16+pool+head" -- are the paths
of the same name without it under fused_eval = "fp16x2+pool" / "bf16+pool": the four units in front of a max-pool in one launch each.
Per shape: every path is warmed up, the number of calls that fills `--seconds` is measured, then `--rounds` interleaved rounds
(default, fused, bf16, bf16/bf16, fused:segment, fused+head, ..., default, ...) of that many calls each are timed with device events
under no_grad (the "+pool" paths ride in the same rounds, so each is interleaved with its own baseline).  Reported: ms per call (median over rounds), images/s, the round-to-round spread (max - min over rounds) and
torch.cuda.max_memory_allocated of each path.  A verdict compares the difference of two medians with the SUM of the two spreads: every
fused path against the default path, the one-part plans against the fp16 plan, each +head path against segment() of its plan, and each
"+pool" path against the path without it."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def _model(C, dev):
    from onet_amd import Onet
    torch.manual_seed(1981)
    return Onet(in_chns=C, binit=True, bshare=True).to(dev).eval()      # (fresh running statistics: the time does not depend on values)


def _timed(m, X, n, call=None):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    call = m if call is None else call
    e0.record()
    for _ in range(n):
        out = call(X)
    e1.record()
    e1.synchronize()
    del out
    return e0.elapsed_time(e1) / n


def _settings():
    from onet_amd import ops
    return {"default": ops.Settings(), "fused": ops.Settings(fused_eval=True), "bf16": ops.Settings(fused_eval="bf16"),
            "bf16/bf16": ops.Settings(conv="bf16", fused_eval="bf16"), "fused+pool": ops.Settings(fused_eval="fp16x2+pool"),
            "bf16+pool": ops.Settings(fused_eval="bf16+pool"), "bf16/bf16+pool": ops.Settings(conv="bf16", fused_eval="bf16+pool")}


PATHS = ("default", "fused", "bf16", "bf16/bf16", "fused+pool", "bf16+pool", "bf16/bf16+pool", "fused:segment", "fused+head",
         "fused+pool+head", "bf16/bf16:segment", "bf16/bf16+head", "bf16/bf16+pool+head")
# each "+pool" path and the path it is held against
POOL_PAIRS = (("fused", "fused+pool"), ("bf16", "bf16+pool"), ("bf16/bf16", "bf16/bf16+pool"), ("fused+head", "fused+pool+head"),
              ("bf16/bf16+head", "bf16/bf16+pool+head"))


def _paths(m):
    """-> {path: (settings, the timed call)}: the forward paths, then segment() with and without the fused head on the two plans"""
    import onet_amd
    sets = _settings()
    out = {name: (st, m) for name, st in sets.items()}
    for name in ("fused", "bf16/bf16"):
        out[name + ":segment"] = (sets[name], lambda X: onet_amd.segment(m, X))
        out[name + "+head"] = (sets[name], lambda X: onet_amd.segment(m, X, head="fused"))
        out[name + "+pool+head"] = (sets[name + "+pool"], lambda X: onet_amd.segment(m, X, head="fused"))
    assert tuple(out) == PATHS
    return out


def _verdict(base, other):
    """-> (gain of `other` over `base` in ms, noise, verdict): the difference of the medians against the sum of the spreads"""
    gain = base["ms"] - other["ms"]
    noise = base["spread_ms"] + other["spread_ms"]
    return gain, noise, "faster" if gain > noise else ("slower" if -gain > noise else "within spread")


def time_shape(shape, rounds, seconds, dev):
    import onet_amd
    B, C, H, W = shape
    m = _model(C, dev)
    X = torch.rand((B, C, H, W), device=dev)
    sets = _paths(m)
    res = {"shape": list(shape), "plans": {}}
    for name, (st, _) in sets.items():
        if name != "default":
            m.settings = st
            plan = onet_amd.fused_eval_plan(m, X.shape, head="fused" if name.endswith("+head") else None)
            res["plans"][name] = {"fused": plan["fused"], "depth": plan["depth"], "operands": plan["operands"], "reason": plan["reason"],
                                  "last_unit": plan["layers"].get("up4.c2"),
                                  "pooled_units": sorted(k for k, v in plan["layers"].items() if v == "fused+pool")}
    res["plan_fused"], res["depth"], res["reason"] = (res["plans"]["fused"][k] for k in ("fused", "depth", "reason"))
    with torch.no_grad():
        n = {}
        for name, (st, call) in sets.items():
            m.settings = st
            for _ in range(3):
                call(X)
            torch.cuda.synchronize()
            n[name] = max(2, int(seconds * 1e3 / _timed(m, X, 5, call)) + 1)
        ms = {k: [] for k in sets}
        mem = {}
        for r in range(rounds):
            for name, (st, call) in sets.items():
                m.settings = st
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                ms[name].append(_timed(m, X, n[name], call))
                mem[name] = max(mem.get(name, 0), torch.cuda.max_memory_allocated())
    for name in sets:
        v = sorted(ms[name])
        med = v[len(v) // 2]
        res[name] = {"ms": med, "img_s": 1e3 * B / med, "spread_ms": v[-1] - v[0], "rounds_ms": ms[name], "forwards_per_round": n[name],
                     "max_mem_MiB": mem[name] / 2 ** 20}
    res["gain_ms"], res["noise_ms"], res["verdict"] = _verdict(res["default"], res["fused"])
    res["versus"] = {}
    for base, other in (("default", "fused"), ("default", "bf16"), ("default", "bf16/bf16"), ("fused", "bf16"), ("fused", "bf16/bf16"),
                        ("fused:segment", "fused+head"), ("bf16/bf16:segment", "bf16/bf16+head")) + POOL_PAIRS:
        g, nz, v = _verdict(res[base], res[other])
        res["versus"][f"{other} vs {base}"] = {"gain_ms": g, "noise_ms": nz, "verdict": v}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--shapes", default="32x1x256x256,2x1x256x256,1x3x512x512")
    ap.add_argument("--json", default=None)
    ap.add_argument("--profile-run", default=None, help="BxCxHxW: run 3 warm-up + 10 forwards of --path and exit")
    ap.add_argument("--path", default="fused", choices=list(PATHS))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    if a.profile_run:
        B, C, H, W = (int(v) for v in a.profile_run.split("x"))
        m = _model(C, dev)
        m.settings, call = _paths(m)[a.path]
        X = torch.rand((B, C, H, W), device=dev)
        with torch.no_grad():
            for _ in range(13):
                call(X)
        torch.cuda.synchronize()
        return
    out = []
    for s in a.shapes.split(","):
        shape = tuple(int(v) for v in s.split("x"))
        r = time_shape(shape, max(5, a.rounds), a.seconds, dev)
        out.append(r)
        print("x".join(map(str, shape)), flush=True)
        for name in PATHS:
            p = r["plans"].get(name)
            print("  %-19s %s %8.3f ms (%6.0f img/s, spread %.3f, %5.0f MiB)" % (
                name, "depth %d" % p["depth"] if p else "       ", r[name]["ms"], r[name]["img_s"], r[name]["spread_ms"], r[name]["max_mem_MiB"]),
                flush=True)
        for k, v in r["versus"].items():
            print("  %-35s gain %7.3f ms vs noise %.3f: %s" % (k, v["gain_ms"], v["noise_ms"], v["verdict"]), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
