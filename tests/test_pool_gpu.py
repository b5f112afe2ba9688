"""Continuous batching on the device (mp_hip_decode_queue, Device.synthesize_queue): a
finished decode slot is refilled from the queue between two graph replays. Every
utterance must equal the same utterance decoded alone, bit for bit, in every weight mode,
cache type and cross-attention form, and the iteration count must be the one the
schedule's Python restatement (magpie_amd.dist.simulate_pool) gives.

The mix is tests/test_queue_gpu.py's (EOS live, 4..48 frames), with utterance 9 cut to
a single token; in claim order 0, 1, ... utterance 5 (48 tokens) is longer than every
initially resident text, so its install changes the text stride. On the CPU oracle the
frames are 4 4 48 48 48 5 4 39 17 48: simulate_pool gives 96 iterations at 4 slots
against 144 for the batched queue (batch=4, longest first)."""
import json
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STEPS = 48
LENS = [8 + 5 * ((7 * i) % 9) for i in range(9)] + [1]
SPKS = [i % 5 for i in range(10)]


@pytest.fixture(scope="module")
def ma():
    import magpie_amd
    if magpie_amd.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    return magpie_amd


def _cache():
    cache = os.environ.get("MAGPIE_CACHE", "/tmp/magpie_amd_cache")
    os.makedirs(cache, exist_ok=True)
    return cache


@pytest.fixture(scope="module")
def eos_model(ma):
    return ma.synth_gguf(os.path.join(_cache(), "magpie_small_eosb0.09.gguf"), dec_layers=2, enc_layers=1, eos_bias=0.09)


@pytest.fixture(scope="module")
def toks(ma):
    return [ma.synthetic_tokens(n, seed=1700 + i) for i, n in enumerate(LENS)]


@pytest.fixture(scope="module")
def dev(ma, eos_model):
    d = ma.Device(eos_model, xa="reassoc")
    yield d
    d.close()


@pytest.fixture(scope="module")
def singles(dev, toks):
    """greedy f32 single runs, computed once and left unchanged"""
    return [dev.synthesize([t], speakers=[SPKS[i]], max_dec_steps=STEPS).codes[0] for i, t in enumerate(toks)]


def _assert_equal_singles(res, refs):
    assert len(res.codes) == len(refs)
    for i, ref in enumerate(refs):
        assert res.codes[i] is not None, i
        assert res.n_frames[i] == len(ref), (i, res.n_frames[i], len(ref))
        assert np.array_equal(res.codes[i], ref), i


@pytest.mark.parametrize("slots", [2, 4])
def test_pool_equals_single_runs_greedy(dev, toks, singles, slots):
    assert len(toks[5]) > max(len(t) for t in toks[:slots]) and len(toks[9]) == 1
    res = dev.synthesize_queue(toks, SPKS, slots=slots, max_dec_steps=STEPS)
    _assert_equal_singles(res, singles)
    assert res.slots == slots and res.refills == len(toks) - slots
    assert res.useful_slot_iters == sum(len(r) for r in singles)
    assert len({len(r) for r in singles}) >= 3  # unequal lengths: slots really free up at different frames


def test_pool_iterations_match_simulation_and_beat_batches(dev, toks, singles):
    from magpie_amd.dist import gather_results, simulate_pool, synthesize_queue
    frames = [len(r) for r in singles]
    res = dev.synthesize_queue(toks, SPKS, slots=4, poll=8, max_dec_steps=STEPS)
    _assert_equal_singles(res, singles)
    batched = []

    def synth(tb, sb):
        r = dev.synthesize(tb, speakers=sb, max_dec_steps=STEPS)
        batched.append(r.iterations)
        return r.codes
    got = gather_results(synthesize_queue(synth, toks, SPKS, batch=4), len(toks))
    for i, ref in enumerate(singles):
        assert np.array_equal(got[i], ref), i
    print(f"frames {frames}: pool {res.iterations} iterations, batched queue {sum(batched)} {batched}; "
          f"useful / (iterations x slots) = {res.useful_slot_iters} / ({res.iterations} x {res.slots}) = "
          f"{res.utilisation:.3f} (batched {sum(frames) / (4 * sum(batched)):.3f})")
    assert (res.iterations, res.useful_slot_iters) == simulate_pool(frames, 4, 8, STEPS)
    assert res.iterations < sum(batched)


def test_pool_sampling_follows_the_utterance(dev, toks):
    kw = dict(max_dec_steps=STEPS, temperature=0.7, top_k=80, seed=20260)
    res = dev.synthesize_queue(toks, SPKS, slots=4, **kw)
    drew = 0
    for i, t in enumerate(toks):
        ref = dev.synthesize([t], speakers=[SPKS[i]], stream_base=i, **kw).codes[0]
        assert res.n_frames[i] == len(ref), i
        assert np.array_equal(res.codes[i], ref), i
        other = dev.synthesize([t], speakers=[SPKS[i]], stream_base=i + 1, **kw).codes[0] if i == 6 else ref
        drew += not (len(other) == len(ref) and np.array_equal(other, ref))
    assert drew == 1  # the stream matters: a refilled utterance with its slot's stream would differ


def test_pool_bf16_kv_bf16_16_slots(ma, eos_model):
    """the 16-slot merge lists and the 2-byte cache copy"""
    steps = 24
    toks = [ma.synthetic_tokens(8 + 5 * ((7 * i) % 9), seed=1900 + i) for i in range(20)]
    spks = [i % 5 for i in range(20)]
    d = ma.Device(eos_model, weights="bf16", kv="bf16", xa="reassoc")
    try:
        res = d.synthesize_queue(toks, spks, slots=16, max_dec_steps=steps)
        assert res.slots == 16 and res.refills == 4
        for i, t in enumerate(toks):
            ref = d.synthesize([t], speakers=[spks[i]], max_dec_steps=steps).codes[0]
            assert np.array_equal(res.codes[i], ref), i
    finally:
        d.close()


def test_pool_q8_direct_xa(ma, toks):
    """a Q8_0 file: direct XA, nothing to copy for K' / V'"""
    path = ma.synth_gguf(os.path.join(_cache(), "magpie_small_q8_eosb0.09.gguf"), dtype="q8_0", dec_layers=2,
                         enc_layers=1, eos_bias=0.09)
    d = ma.Device(path, weights="q8")
    try:
        res = d.synthesize_queue(toks, SPKS, slots=4, max_dec_steps=STEPS)
        for i, t in enumerate(toks):
            ref = d.synthesize([t], speakers=[SPKS[i]], max_dec_steps=STEPS).codes[0]
            assert np.array_equal(res.codes[i], ref), i
    finally:
        d.close()


def test_pool_f32_direct_xa(ma, eos_model, toks):
    d = ma.Device(eos_model, xa="direct")
    try:
        res = d.synthesize_queue(toks, SPKS, slots=4, max_dec_steps=STEPS)
        for i, t in enumerate(toks):
            ref = d.synthesize([t], speakers=[SPKS[i]], max_dec_steps=STEPS).codes[0]
            assert np.array_equal(res.codes[i], ref), i
    finally:
        d.close()


def test_plain_batch_after_pool_is_restored(dev, toks, singles):
    """the stream table and the decode state of a pool run do not leak into the next batch"""
    kw = dict(max_dec_steps=STEPS, temperature=0.7, top_k=80, seed=7)
    dev.synthesize_queue(toks, SPKS, slots=4, **kw)
    batch = dev.synthesize(toks[:4], speakers=SPKS[:4], **kw)
    for b in range(4):
        ref = dev.synthesize([toks[b]], speakers=[SPKS[b]], stream_base=b, **kw).codes[0]
        assert np.array_equal(batch.codes[b], ref), b
    greedy = dev.synthesize(toks[4:8], speakers=SPKS[4:8], max_dec_steps=STEPS)
    for b in range(4):
        assert np.array_equal(greedy.codes[b], singles[4 + b]), b


def test_pool_argument_errors_leave_device_usable(ma, dev, toks, singles):
    bad = [t.copy() for t in toks]
    bad[-1][0] = 5000  # a token id out of range in the LAST utterance: refused before anything runs
    cases = [dict(tokens=toks, slots=0), dict(tokens=toks, slots=dev.max_batch() + 1), dict(tokens=bad, slots=4),
             dict(tokens=toks, slots=4, trace=True)]
    for kw in cases:
        tk = kw.pop("tokens")
        with pytest.raises(ma.MagpieError, match="MP_ERR_ARG"):
            dev.synthesize_queue(tk, SPKS, max_dec_steps=STEPS, **kw)
        r = dev.synthesize([toks[0]], speakers=[SPKS[0]], max_dec_steps=STEPS)
        assert np.array_equal(r.codes[0], singles[0])
    res = dev.synthesize_queue(toks, SPKS, slots=4, max_dec_steps=STEPS)
    _assert_equal_singles(res, singles)


def test_cpp_queue_equals_synthesize_codes(ma, eos_model):
    """magpie_synthesize_codes_queue (include/magpie.h) through bin/magpie-queue-probe"""
    exe = os.path.join(ma.PKG_DIR, "bin", "magpie-queue-probe")
    out = subprocess.run([exe, eos_model, "2", "24"] + [str(n) for n in (8, 43, 33, 48, 1, 23)], capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr[-2000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert r["ok"] and r["equal"] and len(r["frames"]) == 6 and all(0 < f <= 24 for f in r["frames"]), r
