"""Validation-step time: metrics.evaluate against onet_amd.validate, in ONE process (the method of tools/time_eval.py).

    python tools/time_validate.py [--rounds 5] [--seconds 1.0] [--shapes 32x1x256x256,1x3x512x512] [--json out.json]

Paths, each one validation step on a batch X with float32 ground truth (the reference's label dtype):
  evaluate              metrics.evaluate(m, X, gt) under Settings(): forward, int64 labels, two conversion passes, confusion counts, a host
                        synchronisation, the flip, counts again, a second synchronisation
  evaluate/bf16+pool    the same under Settings(fused_eval="bf16+pool") (evaluate's forward takes the fused plan, not the labels-only one)
  validate              onet_amd.validate(m, X, gt, into=EvalCounts) under Settings(): the ordinary forward, then one launch
  validate/bf16+pool    the same under Settings(fused_eval="bf16+pool"): the labels-only plan, then one launch
A validate round is an "epoch" of its own: the EvalCounts is reset, the calls are made, and rows() -- the one device-to-host copy --
is inside the timed region.  Per shape every path is warmed up, the number of calls that fills `--seconds` is measured, then `--rounds`
interleaved rounds of that many calls each are timed with device events.  Reported: ms per call (median over rounds) and the
round-to-round spread (max - min); a verdict holds the difference of two medians against the SUM of the two spreads."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

PATHS = ("evaluate", "evaluate/bf16+pool", "validate", "validate/bf16+pool")


def _paths(m, gt, n_max):
    """-> {path: (settings, round(X, n))}: `round` makes n calls"""
    import onet_amd
    from onet_amd import metrics, ops
    ec = onet_amd.EvalCounts(n_max * gt.shape[0], gt.device)

    def evaluate(X, n):
        for _ in range(n):
            metrics.evaluate(m, X, gt)

    def validate(X, n):
        ec.reset()
        for _ in range(n):
            onet_amd.validate(m, X, gt, into=ec)
        return ec.rows()

    plain, pool = ops.Settings(), ops.Settings(fused_eval="bf16+pool")
    return {"evaluate": (plain, evaluate), "evaluate/bf16+pool": (pool, evaluate), "validate": (plain, validate),
            "validate/bf16+pool": (pool, validate)}


def _timed(call, X, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    call(X, n)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def _verdict(base, other):
    gain, noise = base["ms"] - other["ms"], base["spread_ms"] + other["spread_ms"]
    return {"gain_ms": gain, "noise_ms": noise, "verdict": "faster" if gain > noise else ("slower" if -gain > noise else "within spread")}


def time_shape(shape, rounds, seconds, dev, n_max=4096):
    import onet_amd
    from onet_amd import Onet
    B, C, H, W = shape
    torch.manual_seed(1981)
    m = Onet(in_chns=C, binit=True, bshare=True).to(dev).eval()
    X = torch.rand((B, C, H, W), device=dev)
    gt = (torch.rand((B, H, W), device=dev) > 0.7).to(torch.float32)
    paths = _paths(m, gt, n_max)
    res = {"shape": list(shape)}
    m.settings = paths["validate/bf16+pool"][0]
    plan = onet_amd.fused_eval_plan(m, X.shape, head="fused")
    res["plan"] = {"fused": plan["fused"], "depth": plan["depth"], "last_unit": plan["layers"].get("up4.c2"), "reason": plan["reason"]}
    n, ms = {}, {k: [] for k in paths}
    for name, (st, call) in paths.items():
        m.settings = st
        call(X, 3)
        torch.cuda.synchronize()
        n[name] = min(n_max, max(2, int(seconds * 1e3 / _timed(call, X, 5)) + 1))
    for _ in range(rounds):
        for name, (st, call) in paths.items():
            m.settings = st
            torch.cuda.synchronize()
            ms[name].append(_timed(call, X, n[name]))
    for name in paths:
        v = sorted(ms[name])
        res[name] = {"ms": v[len(v) // 2], "spread_ms": v[-1] - v[0], "rounds_ms": ms[name], "calls_per_round": n[name]}
    res["versus"] = {f"{b} vs {a}": _verdict(res[a], res[b]) for a, b in (("evaluate", "validate"), ("evaluate", "validate/bf16+pool"),
                                                                          ("evaluate/bf16+pool", "validate/bf16+pool"))}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--shapes", default="32x1x256x256,1x3x512x512")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = []
    for s in a.shapes.split(","):
        shape = tuple(int(v) for v in s.split("x"))
        r = time_shape(shape, max(5, a.rounds), a.seconds, dev)
        out.append(r)
        print("x".join(map(str, shape)), "labels-only plan:", r["plan"], flush=True)
        for name in PATHS:
            print("  %-19s %8.3f ms (spread %.3f, %d calls per round)" % (name, r[name]["ms"], r[name]["spread_ms"], r[name]["calls_per_round"]),
                  flush=True)
        for k, v in r["versus"].items():
            print("  %-42s gain %7.3f ms vs noise %.3f: %s" % (k, v["gain_ms"], v["noise_ms"], v["verdict"]), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
