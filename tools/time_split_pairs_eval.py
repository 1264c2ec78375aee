"""Validation-step and labels-only time of the fp32-level (fp16 hi | mid) eval plan at FULL depth: the plan that stops above the bottom
level ("fp16x2+ragged": depth 4 at 224 and 256 pixels, level 4 on the fp32 fall-back kernels) against the plan that fuses it on
image-pair tiles ("fp16x2+ragged+pairs": depth 5), in ONE process, interleaved like tools/time_pairs_eval.py.

    python tools/time_split_pairs_eval.py [--rounds 5] [--seconds 0.4] [--shapes 32x1x224x224,...] [--json out.json] [--md out.md]

Per shape and per conv in ("split", "auto") three settings -- "default" (Settings(conv)), "ragged" (fused_eval = "fp16x2+ragged": what
the tree launched before the new value existed -- the yardstick) and "pairs" (fused_eval = "fp16x2+ragged+pairs") -- each timing two
calls: `validate(m, X, gt)` and `segment(m, X, head="fused")` of a weight-shared Onet.  Every path is warmed up, the number of calls
that fills `--seconds` is measured, then `--rounds` interleaved rounds of that many calls each are timed with device events.
Reported: ms per call (median over rounds), the round-to-round spread (max - min), the plan's depth; a verdict holds the difference of
two medians against the SUM of the two spreads: "pairs" against "ragged" and "default".  32 x 1 x 200 x 200 is the control: both
values build the same plan there (depth 2), so the two must agree within the spread."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from time_eval import _model, _timed, _verdict  # noqa: E402

CONVS = ("split", "auto")
KINDS = ("default", "ragged", "pairs")
CALLS = ("validate", "segment")
PATHS = tuple(f"{conv}:{kind}:{call}" for conv in CONVS for kind in KINDS for call in CALLS)
SHAPES = "32x1x224x224,32x1x256x256,16x3x224x224,2x1x224x224,32x1x200x200"
VERSUS = (("ragged", "pairs"), ("default", "pairs"), ("default", "ragged"))


def _paths(m, gt):
    """-> {path: (settings, the timed call)}"""
    import onet_amd
    from onet_amd import ops
    calls = {"validate": lambda X: onet_amd.validate(m, X, gt).counts, "segment": lambda X: onet_amd.segment(m, X, head="fused")}
    out = {}
    for conv in CONVS:
        sets = {"default": ops.Settings(conv=conv), "ragged": ops.Settings(conv=conv, fused_eval="fp16x2+ragged"),
                "pairs": ops.Settings(conv=conv, fused_eval="fp16x2+ragged+pairs")}
        for kind in KINDS:
            for call in CALLS:
                out[f"{conv}:{kind}:{call}"] = (sets[kind], calls[call])
    assert tuple(out) == PATHS
    return out


def time_shape(shape, rounds, seconds, dev):
    import onet_amd
    B, C, H, W = shape
    m = _model(C, dev)
    X = torch.rand((B, C, H, W), device=dev)
    gt = (torch.rand((B, H, W), device=dev) > 0.5).to(torch.uint8)
    paths = _paths(m, gt)
    res = {"shape": list(shape), "plans": {}}
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
    for conv in CONVS:
        for call in CALLS:
            for base, other in VERSUS:
                g, nz, v = _verdict(res[f"{conv}:{base}:{call}"], res[f"{conv}:{other}:{call}"])
                res["versus"][f"{conv}:{call}: {other} vs {base}"] = {"gain_ms": g, "noise_ms": nz, "verdict": v}
    return res


def to_md(out, rounds, seconds):
    lines = [f"{rounds} interleaved rounds per path, about {seconds} s of calls per round; ms per call: median over rounds (spread = max - min).", ""]
    for r in out:
        lines += ["### " + "x".join(map(str, r["shape"])), "", "| conv | path | depth | validate ms (spread) | rounds ms | segment(head=fused) ms (spread) | rounds ms |",
                  "|---|---|---|---|---|---|---|"]
        for conv in CONVS:
            for kind in KINDS:
                a, b = r[f"{conv}:{kind}:validate"], r[f"{conv}:{kind}:segment"]
                p = r["plans"][f"{conv}:{kind}:validate"]
                ra, rb = (" ".join(f"{v:.3f}" for v in x["rounds_ms"]) for x in (a, b))
                lines.append(f"| {conv} | {kind} | {p['depth'] if p['fused'] else '-'} | {a['ms']:.3f} ({a['spread_ms']:.3f}) | {ra} | "
                             f"{b['ms']:.3f} ({b['spread_ms']:.3f}) | {rb} |")
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
        shape = tuple(int(v) for v in s.split("x"))
        r = time_shape(shape, max(5, a.rounds), a.seconds, dev)
        out.append(r)
        print("x".join(map(str, shape)), flush=True)
        for name in PATHS:
            p = r["plans"][name]
            print("  %-28s %s %8.3f ms (%6.0f img/s, spread %.3f)" % (name, "depth %d" % p["depth"] if p["fused"] else "       ", r[name]["ms"],
                                                                       r[name]["img_s"], r[name]["spread_ms"]), flush=True)
        for k, v in r["versus"].items():
            print("  %-44s gain %7.3f ms vs noise %.3f: %s" % (k, v["gain_ms"], v["noise_ms"], v["verdict"]), flush=True)
        if a.json:
            with open(a.json, "w") as f:
                json.dump(out, f, indent=1)
        if a.md:
            with open(a.md, "w") as f:
                f.write(to_md(out, max(5, a.rounds), a.seconds))


if __name__ == "__main__":
    main()
