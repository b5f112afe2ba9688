#!/usr/bin/env python3
"""Measures the 32-slot bf16 decode (gemm_b16x2_kernel) and writes profiles/bf16_b32.json.

Workload: bench.py's bf16 lines (Magpie-357M shapes, T = 64, 256 frames, greedy, EOS masked).
Every figure is one process's median of 5 decodes, frames/s over the device time of the
graph replays; configurations alternate process by process for `--rounds` rounds on one
GPU, the parent's process before or after this tree's by turns. `--parent-lib` names a libmagpie_hip.so built from the parent commit (the ABI the
binding uses is unchanged): its B = 16 and f32 B = 1 are measured between this tree's.

    python magpie-tts.cpp_amd/tools/bf16_b32_profile.py --parent-lib /path/to/parent/libmagpie_hip.so
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPO = os.path.dirname(PKG)
FRAMES, T = 256, 64


def worker(a):
    sys.path.insert(0, PKG)
    import magpie_amd as ma
    os.makedirs(a.cache, exist_ok=True)
    model = ma.synth_gguf(os.path.join(a.cache, "magpie_357m_f32_k32.gguf"), lt_head_scale=ma.DECISIVE)
    toks = [ma.synthetic_tokens(T, seed=1000 + b) for b in range(a.B)]
    dev = ma.Device(model, weights=a.weights, kv=a.kv)
    kw = dict(max_dec_steps=FRAMES, ignore_eos=True)
    dev.synthesize(toks, **kw)  # warm-up: code objects, graph capture
    runs = [dev.synthesize(toks, **kw) for _ in range(5)]
    ms = statistics.median(r.decode_ms for r in runs)
    it = runs[0].iterations
    out = {"frames_per_s": a.B * FRAMES / (ms * 1e-3), "us_per_iter": ms * 1e3 / it}
    if a.ops:
        us, names, acc = dev.profile_ops(32), dev.ops(), {}
        for n, u in zip(names, us):
            acc[n] = round(acc.get(n, 0.0) + float(u), 2)
        out["ops_us"] = acc
    dev.close()
    print("RESULT " + json.dumps(out))


def run(cfg, lib, ops=False):
    env = dict(os.environ)
    if lib:
        env["MAGPIE_LIB"] = lib
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--weights", cfg[0], "--kv", cfg[1], "--B", str(cfg[2]),
           "--cache", ARGS.cache] + (["--ops"] if ops else [])
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        sys.exit(f"{cfg} (lib {lib or 'this tree'}) failed with {p.returncode}:\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
    return json.loads(next(l for l in p.stdout.splitlines() if l.startswith("RESULT "))[7:])


def main():
    sys.path.insert(0, PKG)
    import magpie_amd as ma
    this = [("bf16", "f32", 32), ("bf16", "f32", 16), ("bf16", "bf16", 32), ("bf16", "bf16", 16), ("f32", "f32", 1)]
    parent = [("bf16", "f32", 16), ("bf16", "bf16", 16), ("f32", "f32", 1)] if ARGS.parent_lib else []
    res = {("this",) + c: [] for c in this}
    res.update({("parent",) + c: [] for c in parent})
    ops = {}
    for rnd in range(ARGS.rounds):
        for c in this:
            last = rnd == ARGS.rounds - 1 and c[0] == "bf16" and c[1] == "f32"
            if c in parent and rnd % 2:  # which library goes first alternates by round
                res[("parent",) + c].append(run(c, ARGS.parent_lib))
            r = run(c, None, ops=last)
            res[("this",) + c].append(r)
            if last:
                ops[f"B{c[2]}"] = r["ops_us"]
            if c in parent and not rnd % 2:
                res[("parent",) + c].append(run(c, ARGS.parent_lib))
        print(f"round {rnd} done", flush=True)

    def med(k, f="frames_per_s"):
        return statistics.median(r[f] for r in res[k])

    def spread(k):
        v = [r["frames_per_s"] for r in res[k]]
        return (max(v) - min(v)) / statistics.median(v)

    rows = []
    for kv in ("f32", "bf16"):
        row = {"weights": "bf16", "kv": kv,
               "this_b32_frames_per_s": [round(r["frames_per_s"], 1) for r in res[("this", "bf16", kv, 32)]],
               "this_b32_us_per_iter": round(med(("this", "bf16", kv, 32), "us_per_iter"), 2),
               "this_b16_frames_per_s": [round(r["frames_per_s"], 1) for r in res[("this", "bf16", kv, 16)]],
               "this_b16_us_per_iter": round(med(("this", "bf16", kv, 16), "us_per_iter"), 2)}
        if parent:
            pk = ("parent", "bf16", kv, 16)
            row.update({"parent_b16_frames_per_s": [round(r["frames_per_s"], 1) for r in res[pk]],
                        "parent_b16_us_per_iter": round(med(pk, "us_per_iter"), 2),
                        "parent_spread": round(spread(pk), 4),
                        "b32_over_parent_b16": round(med(("this", "bf16", kv, 32)) / med(pk), 4),
                        "b16_over_parent_b16": round(med(("this", "bf16", kv, 16)) / med(pk), 4)})
        rows.append(row)
    row = {"weights": "f32", "kv": "f32", "this_b1_frames_per_s": [round(r["frames_per_s"], 1) for r in res[("this", "f32", "f32", 1)]]}
    if parent:
        pk = ("parent", "f32", "f32", 1)
        row.update({"parent_b1_frames_per_s": [round(r["frames_per_s"], 1) for r in res[pk]], "parent_spread": round(spread(pk), 4),
                    "b1_over_parent_b1": round(med(("this", "f32", "f32", 1)) / med(pk), 4)})
    rows.append(row)
    out = {"what": "bf16 decode at 32 slots against 16 (this tree and the parent commit's library): alternating processes in "
                   f"one call on one MI355X, Magpie-357M shapes, T = {T}, {FRAMES} frames, greedy, ignore_eos; each entry a "
                   f"process's median of 5 decodes, frames/s over the device time of the graph replays; {ARGS.rounds} rounds; "
                   "ops_us: mp_hip_profile_ops event pairs summed over an iteration's launches of that name, last round, f32 cache",
           "lib_sha16": ma.lib_sha16(), "rows": rows, "ops_us": ops}
    os.makedirs(os.path.dirname(ARGS.out), exist_ok=True)
    with open(ARGS.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--weights", default="bf16")
    ap.add_argument("--kv", default="f32")
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--ops", action="store_true")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--cache", default=os.environ.get("MAGPIE_CACHE", "/tmp/magpie_amd_cache"))
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bf16_b32.json"))
    ARGS = ap.parse_args()
    worker(ARGS) if ARGS.worker else main()
