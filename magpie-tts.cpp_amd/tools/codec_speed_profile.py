#!/usr/bin/env python3
"""Measures the speaking-rate call (tsm_kernel in front of the resampler) and writes
profiles/codec_speed.json.

Every figure is one process's median of 9 calls' device time (mp_hip_codec_last_ms: the codec's
launch sequence, the stretch, the resampler) at 22 050 Hz, 16-bit, fixed seeded codes; processes
alternate for `--rounds` rounds on one GPU. `--parent-lib` names a libmagpie_hip.so built from the
parent commit: its mp_hip_codec_decode_pcm is measured between this tree's, first or second by turns.

    python magpie-tts.cpp_amd/tools/codec_speed_profile.py --parent-lib /path/to/parent/libmagpie_hip.so
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPO = os.path.dirname(PKG)
FRAMES, SPEEDS = (32, 256), (50, 125, 200)


def worker(a):
    sys.path.insert(0, PKG)
    import numpy as np
    import magpie_amd as ma
    os.makedirs(a.cache, exist_ok=True)
    codec = ma.Codec(ma.synth_gguf(os.path.join(a.cache, "nano_codec.gguf"), kind="codec"))
    out = {}
    for F in FRAMES:
        codes = np.random.default_rng(F).integers(0, 2016, (8, F)).astype(np.int32)
        for s in (100,) + (SPEEDS if a.speeds else ()):
            kw = dict(speed_pct=s) if s != 100 else {}
            ms = []
            for _ in range(11):  # the first two warm up: code objects, buffers, tables
                codec.decode_pcm(codes, 22050, ma.PCM_S16, **kw)
                ms.append(codec.last_ms())
            out[f"{F}@{s}"] = statistics.median(ms[2:])
    codec.close()
    print("RESULT " + json.dumps(out))


def run(lib):
    env = dict(os.environ)
    if lib:
        env["MAGPIE_LIB"] = lib
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--cache", ARGS.cache] + ([] if lib else ["--speeds"])
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    if p.returncode != 0:
        sys.exit(f"worker (lib {lib or 'this tree'}) failed with {p.returncode}:\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
    return json.loads(next(l for l in p.stdout.splitlines() if l.startswith("RESULT "))[7:])


def main():
    sys.path.insert(0, PKG)
    import magpie_amd as ma
    this, parent = [], []
    for rnd in range(ARGS.rounds):
        if ARGS.parent_lib and rnd % 2:
            parent.append(run(ARGS.parent_lib))
        this.append(run(None))
        if ARGS.parent_lib and not rnd % 2:
            parent.append(run(ARGS.parent_lib))
        print(f"round {rnd} done", flush=True)

    def med(rs, k):
        return statistics.median(r[k] for r in rs)

    rows = []
    for F in FRAMES:
        k = f"{F}@100"
        row = {"frames": F, "decode_pcm_ms": [round(r[k], 4) for r in this]}
        for s in SPEEDS:
            row[f"speed_{s}_ms"] = [round(r[f"{F}@{s}"], 4) for r in this]
            row[f"speed_{s}_over_decode_pcm"] = round(med(this, f"{F}@{s}") / med(this, k), 4)
        if parent:
            v = [r[k] for r in parent]
            row.update({"parent_decode_pcm_ms": [round(x, 4) for x in v],
                        "parent_spread": round((max(v) - min(v)) / statistics.median(v), 4),
                        "decode_pcm_over_parent": round(med(this, k) / med(parent, k), 4)})
        rows.append(row)
    out = {"what": "mp_hip_codec_decode_pcm_speed against mp_hip_codec_decode_pcm of the same frames (this tree, and the parent "
                   "commit's library for the plain call): alternating processes in one call on one MI355X, 22 050 Hz, 16-bit; "
                   f"each entry a process's median of 9 calls' device time (mp_hip_codec_last_ms), ms; {ARGS.rounds} rounds",
           "lib_sha16": ma.lib_sha16(), "rows": rows}
    os.makedirs(os.path.dirname(ARGS.out), exist_ok=True)
    with open(ARGS.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--speeds", action="store_true")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--cache", default=os.environ.get("MAGPIE_CACHE", "/tmp/magpie_amd_cache"))
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "codec_speed.json"))
    ARGS = ap.parse_args()
    worker(ARGS) if ARGS.worker else main()
