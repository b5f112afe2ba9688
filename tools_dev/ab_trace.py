"""A/B numerics: one decode with the library MAGPIE_LIB names (or the default),
saved as $OUT/<tag>.npz (codes, hidden trace; OUT defaults to bench_out, as in ab_lib.sh).
Usage: ab_trace.py TAG WEIGHTS [B [STEPS]]
ab_trace.py --cmp A.npz B.npz ... (pairs): says whether each pair's arrays are bit-identical;
.npy files (bench.py --dump-outputs) compare likewise. Exit status 1 if any pair differs."""
import os
import sys

import numpy as np


def compare(files):
    bad = 0
    for a, b in zip(files[::2], files[1::2]):
        za, zb = np.load(a), np.load(b)
        keys = za.files if hasattr(za, "files") else [None]
        for k in keys:
            xa, xb = (za[k], zb[k]) if k else (za, zb)
            same = xa.shape == xb.shape and xa.tobytes() == xb.tobytes()
            bad += not same
            print(os.path.basename(a), os.path.basename(b), k or "", xa.shape, "bit-identical" if same else "DIFFERS")
    return 1 if bad else 0


if sys.argv[1] == "--cmp":
    sys.exit(compare(sys.argv[2:]))

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "magpie-tts.cpp_amd"))
import magpie_amd as ma  # noqa: E402

tag, weights = sys.argv[1], sys.argv[2]
B = int(sys.argv[3]) if len(sys.argv) > 3 else 1
steps = int(sys.argv[4]) if len(sys.argv) > 4 else 24
cache = os.environ.get("MAGPIE_CACHE", "/tmp/magpie_amd_cache")
os.makedirs(cache, exist_ok=True)
if weights == "q8":  # the Q8 mode needs a file with Q8_0 tensors
    path = ma.synth_gguf(os.path.join(cache, "magpie_357m_q8_k32.gguf"), dtype="q8_0", lt_head_scale=ma.DECISIVE)
elif weights == "f16":  # and the F16 mode one with F16 projections
    path = ma.synth_gguf(os.path.join(cache, "magpie_357m_f16_k32.gguf"), dtype="f16", lt_head_scale=ma.DECISIVE)
else:
    path = ma.synth_gguf(os.path.join(cache, "magpie_357m_f32_k32.gguf"), lt_head_scale=ma.DECISIVE)
dev = ma.Device(path, weights=weights)
toks = [ma.synthetic_tokens(64, seed=1000 + b) for b in range(B)]
r = dev.synthesize(toks, speakers=[0] * B, max_dec_steps=steps, ignore_eos=True, trace=True)
out = os.environ.get("OUT", "bench_out")
os.makedirs(out, exist_ok=True)
np.savez(f"{out}/{tag}.npz", codes=np.asarray(r.codes), hidden=r.hidden)
print(tag, "saved")
