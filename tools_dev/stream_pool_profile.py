"""The streaming slot pool (Device.stream_queue) against the two things it replaces.

Mix: Magpie-357M bf16, 8 slots, 32 utterances of 8..48 tokens, EOS live (eos_bias 0.09),
budget 200. Arms, alternating in one process, medians over `reps` repetitions of the whole
call's wall clock (preambles included):
  stream_pool_continuous / stream_pool_stateless  Device.stream_queue, 4-frame chunks
  queue_then_decode   Device.synthesize_queue, then Codec.decode of every utterance
  stream_batches      Device.synthesize_stream, 8 utterances at a time (continuous codec)
and the device time (mp_hip_codec_last_ms, median of 20 after a warm-up) of one ragged stream
decode of 8 lanes, one at 1 frame and 7 at 4, against the same work as a 7-lane call plus a
1-lane call of mp_hip_codec_stream_decode. Writes one JSON (argv[1]) that names the library it
measured.
"""
import json, os, sys, time
import numpy as np
sys.path.insert(0, "magpie-tts.cpp_amd")
import magpie_amd as ma

out_path = sys.argv[1]
C = os.environ.get("MAGPIE_CACHE", "/tmp/magpie_amd_cache")
os.makedirs(C, exist_ok=True)
cdc = ma.Codec(ma.synth_gguf(C + "/nano_codec.gguf", kind="codec"))
res = {"lib_sha16": ma.lib_sha16(), "reps": 3}

# ---- one ragged call against a uniform call per length
codes = np.random.default_rng(7).integers(0, 2016, (8, 8, 4)).astype(np.int32)
st = cdc.stream(8)
lens = [1] + [4] * 7
def ragged():
    st.decode_ragged(codes, lens)
    return cdc.last_ms()
def two_calls():
    st.decode(codes[1:], lanes=list(range(1, 8)))
    a = cdc.last_ms()
    st.decode(codes[:1, :, :1], lanes=[0])
    return a + cdc.last_ms()
row = {"lanes": 8, "frames": lens, "reps": 20, "unit": "ms, device time of the launch sequences"}
for name, call in (("ragged_call", ragged), ("seven_lane_plus_one_lane_call", two_calls)):
    call()
    ms = [call() for _ in range(20)]
    row[name + "_ms"] = round(float(np.median(ms)), 4)
    row[name + "_min_ms"] = round(float(min(ms)), 4)
st.close()
res["ragged_call"] = row
print(row, flush=True)

# ---- the mix
N, SLOTS, BUDGET, FPC = 32, 8, 200, 4
model = ma.synth_gguf(C + "/magpie_357m_f32_eosb0.09.gguf", eos_bias=0.09)
dev = ma.Device(model, weights="bf16")
toks = [ma.synthetic_tokens(8 + 5 * ((7 * i) % 9), seed=3000 + i) for i in range(N)]
spks = [i % 5 for i in range(N)]


def stream_pool(cont):
    t0 = time.perf_counter()
    r = dev.stream_queue(cdc, toks, lambda u, a: True, speakers=spks, slots=SLOTS, frames_per_chunk=FPC, continuous=cont,
                         max_dec_steps=BUDGET)
    wall = time.perf_counter() - t0
    return {"wall_ms": wall * 1e3, "frames": int(r.useful_slot_iters), "first_audio_ms": r.first_audio_ms,
            "iterations": r.iterations, "refills": r.refills, "utilisation": r.utilisation, "loop_ms": r.decode_ms}


def queue_then_decode():
    t0 = time.perf_counter()
    r = dev.synthesize_queue(toks, spks, slots=SLOTS, max_dec_steps=BUDGET)
    t1 = time.perf_counter()
    for c in r.codes:
        if len(c):
            cdc.decode(np.ascontiguousarray(c.T))
    wall = time.perf_counter() - t0
    return {"wall_ms": wall * 1e3, "frames": int(r.useful_slot_iters), "first_audio_ms": None, "iterations": r.iterations,
            "refills": r.refills, "utilisation": r.utilisation, "codes_ms": (t1 - t0) * 1e3}


def stream_batches():
    t0 = time.perf_counter()
    frames = iters = 0
    first = None
    for b0 in range(0, N, SLOTS):
        cs, _, tm = dev.synthesize_stream(cdc, toks[b0:b0 + SLOTS], lambda u, a: True, speakers=spks[b0:b0 + SLOTS],
                                          max_dec_steps=BUDGET, frames_per_chunk=FPC, continuous=True, stream_base=b0)
        frames += sum(len(c) for c in cs)
        iters += tm.iterations
        if first is None:
            first = tm.first_audio_ms  # from the loop's start, as the pool's
    wall = time.perf_counter() - t0
    # (the streaming batch emits the EOS frame: up to one frame more per utterance)
    return {"wall_ms": wall * 1e3, "frames": frames, "first_audio_ms": first, "iterations": iters, "refills": 0,
            "utilisation": frames / max(1, iters * SLOTS)}


arms = {"stream_pool_continuous": lambda: stream_pool(True), "stream_pool_stateless": lambda: stream_pool(False),
        "queue_then_decode": queue_then_decode, "stream_batches": stream_batches}
for f in arms.values():  # warm-up: graphs captured, buffers grown
    f()
runs = {k: [] for k in arms}
for _ in range(res["reps"]):
    for k, f in arms.items():
        runs[k].append(f())
mix = {"model": "Magpie-357M synthetic, bf16 weights, eos_bias 0.09", "utterances": N, "slots": SLOTS, "budget": BUDGET,
       "frames_per_chunk": FPC, "arms": {}}
for k, rs in runs.items():
    wall = float(np.median([r["wall_ms"] for r in rs]))
    row = dict(rs[0])
    row["wall_ms"] = round(wall, 2)
    row["wall_all_ms"] = [round(r["wall_ms"], 2) for r in rs]
    row["frames_per_s"] = round(row["frames"] / wall * 1e3, 1)
    fa = [r["first_audio_ms"] for r in rs if r["first_audio_ms"] is not None]
    row["first_audio_ms"] = round(float(np.median(fa)), 3) if fa else None
    row["utilisation"] = round(row["utilisation"], 4)
    for key in ("loop_ms", "codes_ms"):
        if key in row:
            row[key] = round(float(np.median([r[key] for r in rs])), 2)
    mix["arms"][k] = row
    print(k, row, flush=True)
res["mix"] = mix
dev.close()
cdc.close()
with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
