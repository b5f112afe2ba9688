#!/usr/bin/env python3
"""Frame cost by cache position, f32 B=1 on the full model (the benchmark's text): the
decode's time over N frames for each N given, REPS decodes each (median), and the mean cost
per frame of every segment between consecutive N. With the defaults 145 256 512 the segments
are frames 0..144 (L = 111..255: one K/V batch per SA split), 145..255 (L = 256..366: two)
and 256..511 (L up to 622: two, then three from frame 402).
usage: frame_cost_by_pos.py [N ...]   (MAGPIE_LIB selects the library; REPS=7)"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "magpie-tts.cpp_amd"))
import magpie_amd as ma  # noqa: E402


def main():
    ns = sorted(int(a) for a in sys.argv[1:]) or [145, 256, 512]
    reps = int(os.environ.get("REPS", "7"))
    cache = os.environ.get("MAGPIE_CACHE", "/tmp/magpie_amd_cache")
    os.makedirs(cache, exist_ok=True)
    model = ma.synth_gguf(os.path.join(cache, "magpie_357m_f32_k32.gguf"), lt_head_scale=ma.DECISIVE)
    dev = ma.Device(model)
    tok = [ma.synthetic_tokens(64, seed=1000)]
    ms = {}
    for n in ns:
        dev.synthesize(tok, speakers=[0], max_dec_steps=n, ignore_eos=True)  # preamble + warm-up decode
        runs = [dev.decode(1, n).decode_ms for _ in range(reps)]
        ms[n] = float(np.median(runs))
        print(f"{n:4d} frames: median {ms[n]:8.3f} ms (min {min(runs):.3f} max {max(runs):.3f}) = "
              f"{1e3 * ms[n] / n:6.1f} us/frame")
    dev.close()
    for a, b in zip([0] + ns[:-1], ns):
        d = ms[b] - ms.get(a, 0.0)
        print(f"frames {a:4d}..{b - 1:4d} (L = {111 + a}..{110 + b}): {1e3 * d / (b - a):6.1f} us/frame")


if __name__ == "__main__":
    main()
