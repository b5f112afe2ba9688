"""Continuous (stateful stream) against stateless codec chunks of the same shape.

Device time (mp_hip_codec_last_ms, median of 20 after a warm-up call) of one call decoding
`lanes` chunks of `frames` frames, stateless (decode_chunks) and on a stream's lanes, and the
time to first audio of f32 batch-1 streaming with 4-frame chunks in both modes (bench.py's
stream_f32_batch1 workload). Writes one JSON (argv[1]) that names the library it measured.
"""
import json, os, sys
import numpy as np
sys.path.insert(0, "magpie-tts.cpp_amd")
import magpie_amd as ma

out_path = sys.argv[1]
C = os.environ.get("MAGPIE_CACHE", "/tmp/magpie_amd_cache")
os.makedirs(C, exist_ok=True)
cdc = ma.Codec(ma.synth_gguf(C + "/nano_codec.gguf", kind="codec"))
res = {"lib_sha16": ma.lib_sha16(), "reps": 20, "chunks": [], "unit": "ms, device time of the call's launch sequence"}
for lanes, F in ((1, 4), (1, 32), (16, 4), (16, 32)):
    codes = np.random.default_rng(lanes * 100 + F).integers(0, 2016, (lanes, 8, F)).astype(np.int32)
    st = cdc.stream(lanes)
    row = {"lanes": lanes, "frames": F}
    for name, call in (("stateless", lambda: cdc.decode_chunks(codes)), ("continuous", lambda: st.decode(codes))):
        call()
        ms = []
        for _ in range(res["reps"]):
            call()
            ms.append(cdc.last_ms())
        row[name + "_ms"] = round(float(np.median(ms)), 4)
        row[name + "_min_ms"] = round(float(min(ms)), 4)
    st.close()
    row["continuous_over_stateless"] = round(row["continuous_ms"] / row["stateless_ms"], 3)
    res["chunks"].append(row)
    print(row, flush=True)

model = ma.synth_gguf(C + "/magpie_357m_f32_k32.gguf", lt_head_scale=ma.DECISIVE)
dev = ma.Device(model)
tok = [ma.synthetic_tokens(64, seed=1000)]
res["stream_f32_batch1"] = {"chunk_frames": 4, "frames": 64, "runs": 5}
for name, cont in (("stateless", False), ("continuous", True)):
    dev.synthesize_stream(cdc, tok, lambda u, a: True, max_dec_steps=32, continuous=cont)  # warm-up
    fa = []
    for _ in range(5):
        _, _, tm = dev.synthesize_stream(cdc, tok, lambda u, a: True, max_dec_steps=64, ignore_eos=True, continuous=cont)
        fa.append(tm.first_audio_ms)
    res["stream_f32_batch1"][name + "_first_audio_ms"] = round(float(np.median(fa)), 3)
    res["stream_f32_batch1"][name + "_first_audio_min_ms"] = round(float(min(fa)), 3)
    print(name, fa, flush=True)
dev.close()
cdc.close()
with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
