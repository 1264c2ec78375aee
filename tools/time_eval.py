"""Eval-mode forward time: the default path against the fused plan (Settings.fused_eval), in ONE process.

    python tools/time_eval.py [--rounds 5] [--seconds 1.0] [--shapes 32x1x256x256,2x1x256x256,1x3x512x512] [--json out.json]
    python tools/time_eval.py --profile-run 32x1x256x256      # fused forwards only: the workload of a rocprofv3 --kernel-trace run

Per shape: both paths are warmed up, the number of forwards that fills `--seconds` is measured, then `--rounds` interleaved rounds
(default, fused, default, fused, ...) of that many forwards each are timed with device events under no_grad.  Reported: ms per
forward (median over rounds), images/s, the round-to-round spread (max - min over rounds) and torch.cuda.max_memory_allocated of
each path.  The verdict per shape compares the difference of the medians with the SUM of the two spreads."""
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


def _timed(m, X, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        out = m(X)
    e1.record()
    e1.synchronize()
    del out
    return e0.elapsed_time(e1) / n


def time_shape(shape, rounds, seconds, dev):
    import onet_amd
    from onet_amd import ops
    B, C, H, W = shape
    m = _model(C, dev)
    X = torch.rand((B, C, H, W), device=dev)
    sets = {"default": ops.Settings(), "fused": ops.Settings(fused_eval=True)}
    m.settings = sets["fused"]
    plan = onet_amd.fused_eval_plan(m, X.shape)
    res = {"shape": list(shape), "plan_fused": plan["fused"], "depth": plan["depth"], "reason": plan["reason"]}
    with torch.no_grad():
        n = {}
        for name, st in sets.items():
            m.settings = st
            for _ in range(3):
                m(X)
            torch.cuda.synchronize()
            n[name] = max(2, int(seconds * 1e3 / _timed(m, X, 5)) + 1)
        ms = {k: [] for k in sets}
        mem = {}
        for r in range(rounds):
            for name, st in sets.items():
                m.settings = st
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                ms[name].append(_timed(m, X, n[name]))
                mem[name] = max(mem.get(name, 0), torch.cuda.max_memory_allocated())
    for name in sets:
        v = sorted(ms[name])
        med = v[len(v) // 2]
        res[name] = {"ms": med, "img_s": 1e3 * B / med, "spread_ms": v[-1] - v[0], "rounds_ms": ms[name], "forwards_per_round": n[name],
                     "max_mem_MiB": mem[name] / 2 ** 20}
    gain = res["default"]["ms"] - res["fused"]["ms"]
    noise = res["default"]["spread_ms"] + res["fused"]["spread_ms"]
    res["gain_ms"], res["noise_ms"] = gain, noise
    res["verdict"] = "faster" if gain > noise else ("slower" if -gain > noise else "within spread")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--shapes", default="32x1x256x256,2x1x256x256,1x3x512x512")
    ap.add_argument("--json", default=None)
    ap.add_argument("--profile-run", default=None, help="BxCxHxW: run 3 warm-up + 10 fused forwards and exit")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    if a.profile_run:
        from onet_amd import ops
        B, C, H, W = (int(v) for v in a.profile_run.split("x"))
        m = _model(C, dev)
        m.settings = ops.Settings(fused_eval=True)
        X = torch.rand((B, C, H, W), device=dev)
        with torch.no_grad():
            for _ in range(13):
                m(X)
        torch.cuda.synchronize()
        return
    out = []
    for s in a.shapes.split(","):
        shape = tuple(int(v) for v in s.split("x"))
        r = time_shape(shape, max(5, a.rounds), a.seconds, dev)
        out.append(r)
        print("%s  depth %d  default %.3f ms (%.0f img/s, spread %.3f, %.0f MiB)  fused %.3f ms (%.0f img/s, spread %.3f, %.0f MiB)  gain %.3f ms "
              "vs noise %.3f: %s" % ("x".join(map(str, shape)), r["depth"], r["default"]["ms"], r["default"]["img_s"], r["default"]["spread_ms"],
                                     r["default"]["max_mem_MiB"], r["fused"]["ms"], r["fused"]["img_s"], r["fused"]["spread_ms"],
                                     r["fused"]["max_mem_MiB"], r["gain_ms"], r["noise_ms"], r["verdict"]), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
