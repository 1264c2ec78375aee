"""Time of one batch of the performance report (verify_onet_simclutter: confusion counts AND the SNR-gain column) and of one batch of
the two-stage cascade, on the device against what a user of this tree composes without the new calls, in ONE process, interleaved
like tools/time_upmap_eval.py.

    python tools/time_verify.py [--rounds 5] [--seconds 0.5] [--shapes 32x1x224x224,2x1x224x224] [--json out.json] [--md out.md]

Per shape and settings (Settings() and Settings(fused_eval="bf16+pool+anymap+pairs+up")) four paths of a weight-shared Onet:
  composed:report   validate(m, X, gt, into, want_labels=True) for the counts, then scores(m, X) -- a second forward -- for Vt, Vd, then
                    measure_snr_on_fg's steps in torch: tensor_normal_per_frame of both, the hard re-assignment on the labels, torch.equal
                    to choose the foreground, get_psnr's formulas on X and on the foreground with their .item()s
  verify_step       verify_step(m, X, gt, into, snr): one forward, two streaming launches, no synchronisation
  composed:cascade  validate(m, X, gt, into), the flip decision read on the host from the batch's counts (.tolist()),
                    tensor_normal_per_frame of the chosen map, validate(m2, X2, gt, into2)
  verify_cascade    verify_cascade(m, m2, X, gt, into, into2)
A round is an epoch of its own: the accumulators' reset(), the calls, and rows() -- the epoch's device-to-host copy -- inside the timed
region.  Every path is warmed up, the number of calls that fills `--seconds` is measured, then `--rounds` interleaved rounds of that
many calls each are timed with device events.  Reported: ms per batch (median over rounds), the spread (max - min); a verdict holds the
difference of two medians against the SUM of the two spreads."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from time_eval import _model, _verdict  # noqa: E402

SETTINGS = {"default": {}, "fused": {"fused_eval": "bf16+pool+anymap+pairs+up"}}
PATHS = ("composed:report", "verify_step", "composed:cascade", "verify_cascade")
VERSUS = (("composed:report", "verify_step"), ("composed:cascade", "verify_cascade"))
SHAPES = "32x1x224x224,2x1x224x224"


def _psnr(img, label):
    """peak signal / mean clutter power and mean target power / mean clutter power in dB, with the host reads the report's loop makes"""
    target = img * label
    n_t = label.sum()
    erc = ((img - target) ** 2).sum() / (img.numel() - n_t)
    psnr = 10 * torch.log10(target.max() ** 2 / erc)
    snr = 10 * torch.log10((target ** 2).sum() / n_t / erc)
    return psnr.item(), snr.item()


def _paths(m, m2, gt, acc):
    import onet_amd
    from onet_amd import metrics
    ec, ec2, es = acc

    def composed_report(X):
        v = onet_amd.validate(m, X, gt, into=ec, want_labels=True)
        Vt, Vd, _ = onet_amd.scores(m, X)
        nt, nd = metrics.tensor_normal_per_frame(Vt), metrics.tensor_normal_per_frame(Vd)
        pred = metrics.re_assign_label(v.labels, gt)
        fg = nd if torch.equal(v.labels, pred) else nt
        return _psnr(X[:, 0], gt), _psnr(fg[:, 0], gt)

    def composed_cascade(X):
        v1 = onet_amd.validate(m, X, gt, into=ec)
        tp, fp, fn, tn = v1.counts.sum(0).tolist()
        X2 = metrics.tensor_normal_per_frame(v1.Vt if tp + tn < fp + fn else v1.Vd)
        return onet_amd.validate(m2, X2, gt, into=ec2).counts

    return {"composed:report": composed_report, "verify_step": lambda X: onet_amd.verify_step(m, X, gt, into=ec, snr=es).moments,
            "composed:cascade": composed_cascade, "verify_cascade": lambda X: onet_amd.verify_cascade(m, m2, X, gt, into=ec, into2=ec2)[1].counts}


def _epoch(call, X, n, acc):
    """ms per batch of one epoch of n batches: reset, the calls, the rows' copy to the host"""
    for a in acc:
        a.reset()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        call(X)
    rows = [a.rows() for a in acc if len(a)]
    e1.record()
    e1.synchronize()
    del rows
    return e0.elapsed_time(e1) / n


def time_shape(shape, which, rounds, seconds, dev, cap=512):
    import onet_amd
    from onet_amd import ops
    B, C, H, W = shape
    m, m2 = _model(C, dev), _model(C, dev)
    m.settings = m2.settings = ops.Settings(**SETTINGS[which])
    X = torch.rand((B, C, H, W), device=dev)
    gt = (torch.rand((B, H, W), device=dev) > 0.9).to(torch.float32)           # (the reference's label dtype)
    acc = (onet_amd.EvalCounts(cap * B, dev), onet_amd.EvalCounts(cap * B, dev), onet_amd.EvalSnr(cap * B, dev))
    paths = _paths(m, m2, gt, acc)
    plan = onet_amd.fused_eval_plan(m, X.shape, head="fused")
    res = {"shape": list(shape), "settings": which, "plan": {"fused": plan.get("fused"), "depth": plan.get("depth"), "reason": plan.get("reason")}}
    with torch.no_grad():
        n = {}
        for name, call in paths.items():
            _epoch(call, X, 3, acc)
            n[name] = min(cap, max(2, int(seconds * 1e3 / _epoch(call, X, 5, acc)) + 1))
        ms = {k: [] for k in paths}
        for _ in range(rounds):
            for name, call in paths.items():
                torch.cuda.synchronize()
                ms[name].append(_epoch(call, X, n[name], acc))
    for name in paths:
        v = sorted(ms[name])
        med = v[len(v) // 2]
        res[name] = {"ms": med, "spread_ms": v[-1] - v[0], "rounds_ms": ms[name], "calls_per_round": n[name]}
    res["versus"] = {}
    for base, new in VERSUS:
        g, nz, v = _verdict(res[base], res[new])
        res["versus"][f"{new} vs {base}"] = {"gain_ms": g, "noise_ms": nz, "verdict": v}
    return res


def to_md(out, rounds, seconds):
    lines = [f"{rounds} interleaved rounds per path, about {seconds} s of calls per round; ms per batch: median over rounds (spread = max - min).", ""]
    for r in out:
        p = r["plan"]
        lines += ["### " + "x".join(map(str, r["shape"])) + f", settings = {r['settings']} (labels-only plan: "
                  + (f"depth {p['depth']}" if p["fused"] else "not taken") + ")", "",
                  "| path | ms per batch | spread | calls per round | rounds (ms) |", "|---|---|---|---|---|"]
        for name in PATHS:
            a = r[name]
            lines.append(f"| `{name}` | {a['ms']:.3f} | {a['spread_ms']:.3f} | {a['calls_per_round']} | " + " ".join(f"{v:.3f}" for v in a["rounds_ms"]) + " |")
        lines += ["", "| comparison | gain ms | summed spreads ms | verdict |", "|---|---|---|---|"]
        lines += [f"| {k} | {v['gain_ms']:.3f} | {v['noise_ms']:.3f} | {v['verdict']} |" for k, v in r["versus"].items()]
        lines.append("")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--shapes", default=SHAPES)
    ap.add_argument("--json", default=None)
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = []
    for s in a.shapes.split(","):
        shape = tuple(int(v) for v in s.split("x"))
        for which in SETTINGS:
            r = time_shape(shape, which, max(5, a.rounds), a.seconds, dev)
            out.append(r)
            print(f"{s} {which} (plan: {r['plan']})", flush=True)
            for name in PATHS:
                print("  %-18s %8.3f ms (spread %.3f, %d calls per round)" % (name, r[name]["ms"], r[name]["spread_ms"], r[name]["calls_per_round"]), flush=True)
            for k, v in r["versus"].items():
                print("  %-40s gain %7.3f ms vs noise %.3f: %s" % (k, v["gain_ms"], v["noise_ms"], v["verdict"]), flush=True)
            if a.json:
                with open(a.json, "w") as f:
                    json.dump(out, f, indent=1)
            if a.md:
                with open(a.md, "w") as f:
                    f.write(to_md(out, max(5, a.rounds), a.seconds))


if __name__ == "__main__":
    main()
