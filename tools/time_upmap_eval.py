"""Validation-step and labels-only time of the eval plan with every ConvTranspose2d edge on slot operands: the plan whose edges with an
odd-w input map or a padded output take the `pack` route ("bf16+pool+anymap+pairs": the level below also writes fp32, a memset, the
general ConvTranspose2d kernel and one conversion pass) against the plan that runs them as ONE launch of the slot-operand GEMM
("bf16+pool+anymap+pairs+up"), in ONE process, interleaved like tools/time_pairs_eval.py.

    python tools/time_upmap_eval.py [--rounds 5] [--seconds 0.4] [--shapes 32x1x200x200@auto,...] [--json out.json] [--md out.md]

A shape is BxCxHxW@conv.  Per shape two settings -- "pairs" (fused_eval = "bf16+pool+anymap+pairs": what the tree launched before the
new value existed -- the yardstick) and "up" (fused_eval = "bf16+pool+anymap+pairs+up") -- each timing two calls: `validate(m, X, gt)`
and `segment(m, X, head="fused")` of a weight-shared Onet.  Every path is warmed up, the number of calls that fills `--seconds` is
measured, then `--rounds` interleaved rounds of that many calls each are timed with device events.  Reported: ms per call (median over
rounds), the round-to-round spread (max - min), the plan's depth and its ConvTranspose2d edges; a verdict holds the difference of the
two medians against the SUM of the two spreads.  224 x 224 and 256 x 256 have no such edge: controls, the two values launch the same
kernels there."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from time_eval import _model, _timed, _verdict  # noqa: E402

VALUES = {"pairs": "bf16+pool+anymap+pairs", "up": "bf16+pool+anymap+pairs+up"}
CALLS = ("validate", "segment")
PATHS = tuple(f"{kind}:{call}" for kind in VALUES for call in CALLS)
SHAPES = "32x1x200x200@auto,16x3x200x200@auto,2x1x200x200@bf16,32x1x224x224@auto,32x1x256x256@auto"


def time_shape(shape, conv, rounds, seconds, dev):
    import onet_amd
    from onet_amd import ops
    B, C, H, W = shape
    m = _model(C, dev)
    X = torch.rand((B, C, H, W), device=dev)
    gt = (torch.rand((B, H, W), device=dev) > 0.5).to(torch.uint8)
    calls = {"validate": lambda X: onet_amd.validate(m, X, gt).counts, "segment": lambda X: onet_amd.segment(m, X, head="fused")}
    paths = {f"{kind}:{call}": (ops.Settings(conv=conv, fused_eval=value), calls[call]) for kind, value in VALUES.items() for call in CALLS}
    assert tuple(paths) == PATHS
    res = {"shape": list(shape), "conv": conv, "plans": {}}
    for name, (st, _) in paths.items():
        m.settings = st
        plan = onet_amd.fused_eval_plan(m, X.shape, head="fused")
        res["plans"][name] = {"fused": plan["fused"], "depth": plan["depth"], "twin": plan.get("twin"), "reason": plan["reason"],
                              "convt": plan["convt"]}
    with torch.no_grad():
        n = {}
        for name, (st, call) in paths.items():
            m.settings = st
            for _ in range(3):
                call(X)
            torch.cuda.synchronize()
            n[name] = max(2, int(seconds * 1e3 / _timed(m, X, 5, call)) + 1)
        ms = {k: [] for k in paths}
        for _ in range(rounds):
            for name, (st, call) in paths.items():
                m.settings = st
                torch.cuda.synchronize()
                ms[name].append(_timed(m, X, n[name], call))
    for name in paths:
        v = sorted(ms[name])
        med = v[len(v) // 2]
        res[name] = {"ms": med, "img_s": 1e3 * B / med, "spread_ms": v[-1] - v[0], "rounds_ms": ms[name], "calls_per_round": n[name]}
    res["versus"] = {}
    for call in CALLS:
        g, nz, v = _verdict(res[f"pairs:{call}"], res[f"up:{call}"])
        res["versus"][f"{call}: up vs pairs"] = {"gain_ms": g, "noise_ms": nz, "verdict": v}
    return res


def _edges(p):
    return " ".join(f"{k}={v}" for k, v in p["convt"].items())


def to_md(out, rounds, seconds):
    lines = [f"{rounds} interleaved rounds per path, about {seconds} s of calls per round; ms per call: median over rounds (spread = max - min).", ""]
    for r in out:
        lines += ["### " + "x".join(map(str, r["shape"])) + f", conv = {r['conv']!r}", "",
                  "| path | depth | ConvTranspose2d edges | validate ms (spread) | segment(head=fused) ms (spread) |", "|---|---|---|---|---|"]
        for kind in VALUES:
            a, b, p = r[f"{kind}:validate"], r[f"{kind}:segment"], r["plans"][f"{kind}:validate"]
            lines.append(f"| {kind} | {p['depth'] if p['fused'] else '-'} | {_edges(p)} | {a['ms']:.3f} ({a['spread_ms']:.3f}) | "
                         f"{b['ms']:.3f} ({b['spread_ms']:.3f}) |")
        lines += ["", "| comparison | gain ms | summed spreads ms | verdict |", "|---|---|---|---|"]
        lines += [f"| {k} | {v['gain_ms']:.3f} | {v['noise_ms']:.3f} | {v['verdict']} |" for k, v in r["versus"].items()]
        lines.append("")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.4)
    ap.add_argument("--shapes", default=SHAPES)
    ap.add_argument("--json", default=None)
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = []
    for s in a.shapes.split(","):
        s, _, conv = s.partition("@")
        shape = tuple(int(v) for v in s.split("x"))
        r = time_shape(shape, conv or "auto", max(5, a.rounds), a.seconds, dev)
        out.append(r)
        print(s + "@" + r["conv"], flush=True)
        for name in PATHS:
            p = r["plans"][name]
            print("  %-16s %s %8.3f ms (%6.0f img/s, spread %.3f)  %s" % (name, "depth %d" % p["depth"] if p["fused"] else "       ", r[name]["ms"],
                                                                         r[name]["img_s"], r[name]["spread_ms"], _edges(p)), flush=True)
        for k, v in r["versus"].items():
            print("  %-28s gain %7.3f ms vs noise %.3f: %s" % (k, v["gain_ms"], v["noise_ms"], v["verdict"]), flush=True)
        if a.json:
            with open(a.json, "w") as f:
                json.dump(out, f, indent=1)
        if a.md:
            with open(a.md, "w") as f:
                f.write(to_md(out, max(5, a.rounds), a.seconds))


if __name__ == "__main__":
    main()
