"""The decode iteration's launch list per batch configuration, as JSON:
{case: {"names": dev.ops(), "bytes": [dev.op_bytes(i) ...]}} on the 2-layer synthetic
models. tests/golden/op_lists.json is this tool's output with the library of the commit
before the list got its builder (MAGPIE_LIB selects a library, as for ab_trace.py);
tests/test_op_list_gpu.py compares the current build against it.
Usage: dump_op_lists.py OUT.json"""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "magpie-tts.cpp_amd"))

# (model, weights, B, env knobs, xa form)
_GRID = [
    ("small", "f32", (1, 2, 8)), ("small", "bf16", (1, 8, 16)), ("f16", "f16", (1, 8, 16)),
    ("q8", "q8", (1, 4, 8, 16)), ("q4", "q4", (1,)),
]
_VARIANTS = [
    ("small", "f32", 1, {}, "direct"),
    ("small", "bf16", 8, {"MAGPIE_MERGE8": "0"}, "auto"),
    ("small", "bf16", 16, {"MAGPIE_SA16": "0"}, "auto"),
    ("q8", "q8", 1, {"MAGPIE_Q8_UNFUSED": "1"}, "auto"),
    ("q8", "q8", 1, {"MAGPIE_LTQ8": "0"}, "auto"),
]


def _name(weights, B, env, xa):
    tail = [f"{k[len('MAGPIE_'):].lower()}={v}" for k, v in env.items()] + ([f"xa_{xa}"] if xa != "auto" else [])
    return "_".join([weights, f"b{B}"] + tail)


CASES = {_name(w, B, {}, "auto"): (m, w, B, {}, "auto") for m, w, Bs in _GRID for B in Bs}
CASES.update({_name(w, B, env, xa): (m, w, B, env, xa) for m, w, B, env, xa in _VARIANTS})

# the synthetic files of tests/conftest.py's fixtures (small_model, f16_model, q8_model, q4_model)
MODEL_FILES = {"small": ("magpie_small_l2e1_k32.gguf", "f32"), "f16": ("magpie_small_f16_k32.gguf", "f16"),
               "q8": ("magpie_small_q8_k32.gguf", "q8_0"), "q4": ("magpie_small_q4_k32.gguf", "q4_0")}


def run_case(ma, path, case, eager=False):
    """One greedy 8-frame decode of 24-token prompts; returns (result, names, bytes).
    The knobs are read when the list is built: set before the Device exists."""
    _, weights, B, env, xa = CASES[case]
    env = dict(env, **({"MAGPIE_EAGER": "1"} if eager else {}))
    os.environ.update(env)
    try:
        dev = ma.Device(path, weights=weights, xa=xa)
        toks = [ma.synthetic_tokens(24, seed=9100 + b) for b in range(B)]
        r = dev.synthesize(toks, speakers=[b % 5 for b in range(B)], max_dec_steps=8, ignore_eos=True, trace=True)
        names = dev.ops()
        nbytes = [dev.op_bytes(i) for i in range(len(names))]
        dev.close()
    finally:
        for k in env:
            os.environ.pop(k, None)
    return r, names, nbytes


def main():
    import magpie_amd as ma
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    out = sys.argv[1]
    cache = os.environ.get("MAGPIE_CACHE", "/tmp/magpie_amd_cache")
    os.makedirs(cache, exist_ok=True)
    paths = {k: ma.synth_gguf(os.path.join(cache, f), dtype=dt, dec_layers=2, enc_layers=1, lt_head_scale=ma.DECISIVE)
             for k, (f, dt) in MODEL_FILES.items()}
    res = {}
    for case, spec in CASES.items():
        _, names, nbytes = run_case(ma, paths[spec[0]], case)
        res[case] = {"names": names, "bytes": nbytes}
        print(f"{case}: {len(names)} ops")
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    with open(out, "w") as f:  # one case per line
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(res[k])}" for k in sorted(res)) + "\n}\n")
    print("library", ma.lib_sha16(), "->", out)


if __name__ == "__main__":
    main()
