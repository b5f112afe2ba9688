"""The streaming slot pool (mp_hip_decode_queue_stream, Device.stream_queue): the slot pool of
tests/test_pool_gpu.py (same small EOS model and mix) handing out every utterance's audio
chunk by chunk. Per utterance the codes are its single run's; the chunks are
frames_per_chunk frames each and the remainder; in continuous mode (one ragged stream decode
per round, slot b on lane b) the concatenated audio is, bit for bit, Codec.decode of the
codes, in stateless mode every chunk is Codec.decode of that chunk's codes alone; and the
order of all events is the one magpie_amd.dist.simulate_pool_stream gives for the frame
counts."""
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
def codec(ma, codec_model):
    c = ma.Codec(codec_model)
    yield c
    c.close()


@pytest.fixture(scope="module")
def singles(dev, toks):
    """greedy f32 single runs, computed once and left unchanged"""
    return [dev.synthesize([t], speakers=[SPKS[i]], max_dec_steps=STEPS).codes[0] for i, t in enumerate(toks)]


@pytest.fixture(scope="module")
def one_shots(codec, singles):
    """Codec.decode of every single run's codes, computed once and left unchanged"""
    return [codec.decode(np.ascontiguousarray(c.T)) for c in singles]


class Listener:
    """what on_audio heard: every event in order, the chunks per utterance"""

    def __init__(self, n, stop=None):
        self.events, self.chunks, self.ends, self.stop = [], [[] for _ in range(n)], [0] * n, stop or {}
        self.late = []

    def __call__(self, utt, samples):
        if samples is None:
            self.events.append((utt, 0))
            self.ends[utt] += 1
            return True
        if self.ends[utt]:
            self.late.append(utt)
        assert samples.size % 1024 == 0
        self.events.append((utt, samples.size // 1024))
        self.chunks[utt].append(samples)
        return len(self.chunks[utt]) < self.stop.get(utt, 1 << 30)

    def audio(self, utt):
        return np.concatenate(self.chunks[utt]) if self.chunks[utt] else np.zeros(0, np.float32)


def _assert_chunking(L, frames, fpc):
    assert not L.late, f"chunks after the end notice: {L.late}"
    for u, f in enumerate(frames):
        sizes = [c.size // 1024 for c in L.chunks[u]]
        assert sizes == [fpc] * (f // fpc) + ([f % fpc] if f % fpc else []), (u, sizes, f)
        assert L.ends[u] == 1, (u, L.ends[u])


def _assert_codes(res, refs):
    assert len(res.codes) == len(refs)
    for i, ref in enumerate(refs):
        assert res.codes[i] is not None, f"done was not called for utterance {i}"
        assert res.n_frames[i] == len(ref), (i, res.n_frames[i], len(ref))
        assert np.array_equal(res.codes[i], ref), i


@pytest.mark.parametrize("fpc", [4, 3])
def test_continuous_equals_single_runs_and_one_shot_audio(dev, codec, toks, singles, one_shots, fpc):
    from magpie_amd.dist import simulate_pool_stream
    frames = [len(r) for r in singles]
    assert len({f % fpc for f in frames}) >= 2 and len(set(frames)) >= 3  # short last chunks, unequal ends
    L = Listener(len(toks))
    res = dev.stream_queue(codec, toks, L, speakers=SPKS, slots=4, frames_per_chunk=fpc, continuous=True,
                           max_dec_steps=STEPS)
    _assert_codes(res, singles)
    _assert_chunking(L, frames, fpc)
    for u in range(len(toks)):
        np.testing.assert_array_equal(L.audio(u), one_shots[u], err_msg=f"utterance {u}")
    it, rounds = simulate_pool_stream(frames, 4, fpc, STEPS)
    assert L.events == [e for r in rounds for e in r]
    assert res.iterations == it
    assert res.slots == 4 and res.refills == len(toks) - 4
    assert res.useful_slot_iters == sum(frames)
    assert res.first_audio_ms is not None and res.first_audio_ms > 0
    print(f"fpc {fpc}: frames {frames}, {res.iterations} iterations, first audio after {res.first_audio_ms:.2f} ms, "
          f"utilisation {res.utilisation:.3f}")


def test_stateless_chunks_are_decoded_alone(dev, codec, toks, singles, one_shots):
    fpc = 4
    frames = [len(r) for r in singles]
    L = Listener(len(toks))
    res = dev.stream_queue(codec, toks, L, speakers=SPKS, slots=4, frames_per_chunk=fpc, continuous=False,
                           max_dec_steps=STEPS)
    _assert_codes(res, singles)
    _assert_chunking(L, frames, fpc)
    later_differs = False
    for u, ref in enumerate(singles):
        for k, chunk in enumerate(L.chunks[u]):
            alone = codec.decode(np.ascontiguousarray(ref[k * fpc:k * fpc + chunk.size // 1024].T))
            np.testing.assert_array_equal(chunk, alone, err_msg=f"utterance {u} chunk {k}")
            if k >= 1:  # the continuous run's chunk k is the one-shot's samples: it saw the frames before it
                later_differs |= not np.array_equal(chunk, one_shots[u][k * fpc * 1024:k * fpc * 1024 + chunk.size])
    assert later_differs, "stateless and continuous chunks agree everywhere: the mode is not switched"


def test_sampling_follows_the_utterance(dev, codec, toks):
    kw = dict(max_dec_steps=STEPS, temperature=0.7, top_k=80, seed=20260)
    L = Listener(len(toks))
    res = dev.stream_queue(codec, toks, L, speakers=SPKS, slots=4, continuous=True, **kw)
    refs = [dev.synthesize([t], speakers=[SPKS[i]], stream_base=i, **kw).codes[0] for i, t in enumerate(toks)]
    _assert_codes(res, refs)
    _assert_chunking(L, [len(r) for r in refs], 4)


def test_bf16_kv_bf16_16_slots(ma, eos_model, codec):
    steps = 24
    toks = [ma.synthetic_tokens(8 + 5 * ((7 * i) % 9), seed=1900 + i) for i in range(20)]
    spks = [i % 5 for i in range(20)]
    d = ma.Device(eos_model, weights="bf16", kv="bf16", xa="reassoc")
    try:
        L = Listener(len(toks))
        res = d.stream_queue(codec, toks, L, speakers=spks, slots=16, continuous=True, max_dec_steps=steps)
        assert res.slots == 16 and res.refills == 4
        refs = [d.synthesize([t], speakers=[spks[i]], max_dec_steps=steps).codes[0] for i, t in enumerate(toks)]
        _assert_codes(res, refs)
        for u, ref in enumerate(refs):
            np.testing.assert_array_equal(L.audio(u), codec.decode(np.ascontiguousarray(ref.T)), err_msg=f"utterance {u}")
    finally:
        d.close()


def test_callback_stops_one_utterance(dev, codec, toks, singles, one_shots):
    fpc = 4
    frames = [len(r) for r in singles]
    assert frames[2] > 2 * fpc  # utterance 2 has more to give when it is stopped
    before_plain = dev.synthesize(toks[:4], speakers=SPKS[:4], max_dec_steps=STEPS).codes
    Lb = Listener(4)
    before_stream = dev.synthesize_stream(codec, toks[:4], Lb, speakers=SPKS[:4], max_dec_steps=STEPS, continuous=True)[0]
    L = Listener(len(toks), stop={2: 1})
    res = dev.stream_queue(codec, toks, L, speakers=SPKS, slots=4, frames_per_chunk=fpc, continuous=True,
                           max_dec_steps=STEPS)
    assert [c.size for c in L.chunks[2]] == [fpc * 1024]
    assert res.n_frames[2] == fpc and np.array_equal(res.codes[2], singles[2][:fpc])
    np.testing.assert_array_equal(L.audio(2), one_shots[2][:fpc * 1024])
    assert L.ends == [1] * len(toks) and not L.late
    for u in range(len(toks)):
        if u == 2:
            continue
        assert np.array_equal(res.codes[u], singles[u]), u
        np.testing.assert_array_equal(L.audio(u), one_shots[u], err_msg=f"utterance {u}")
    assert res.refills == len(toks) - 4
    # nothing leaks into the next plain batch or the next streaming batch
    after_plain = dev.synthesize(toks[:4], speakers=SPKS[:4], max_dec_steps=STEPS).codes
    La = Listener(4)
    after_stream = dev.synthesize_stream(codec, toks[:4], La, speakers=SPKS[:4], max_dec_steps=STEPS, continuous=True)[0]
    for b in range(4):
        assert np.array_equal(after_plain[b], before_plain[b]) and np.array_equal(after_plain[b], singles[b]), b
        assert np.array_equal(after_stream[b], before_stream[b]), b
        np.testing.assert_array_equal(La.audio(b), Lb.audio(b), err_msg=f"utterance {b}")


def _batch_rounds(frames, fpc):
    """the chunk lengths the streaming batch hands out round by round: round r carries frames
    r*fpc .. of every utterance that still has some"""
    return [[min(fpc, f - r * fpc) for f in frames if f > r * fpc] for r in range((max(frames) + fpc - 1) // fpc)]


@pytest.mark.parametrize("fpc", [4, 3])
def test_batch_continuous_round_mixes_full_and_short_chunks(dev, codec, toks, fpc):
    """mp_hip_decode_stream in continuous mode through rounds whose chunks differ in length (one
    ragged stream decode per round), and through an utterance that ends on a chunk boundary"""
    utts = [0, 5, 8, 7, 2]
    kw = dict(max_dec_steps=STEPS, frames_per_chunk=fpc)

    def stream(us, continuous):
        L = Listener(len(us))
        codes, total, _ = dev.synthesize_stream(codec, [toks[u] for u in us], L, speakers=[SPKS[u] for u in us],
                                                continuous=continuous, **kw)
        assert total == 1024 * sum(len(c) for c in codes)
        return L, codes

    L, codes = stream(utts, True)
    frames = [len(c) for c in codes]
    print(f"fpc {fpc}: frames {frames}, rounds {_batch_rounds(frames, fpc)}")
    # the inputs' property, from the frame counts: with 4-frame chunks some round holds a full
    # chunk beside two short ones of different lengths; at this chunk size some round holds a full
    # chunk beside a short one, and some utterance ends on a chunk boundary
    assert any(4 in r and len({n for n in r if n < 4}) >= 2 for r in _batch_rounds(frames, 4)), frames
    assert any(fpc in r and min(r) < fpc for r in _batch_rounds(frames, fpc)), frames
    assert any(f % fpc == 0 for f in frames), frames
    assert not L.late
    for b, f in enumerate(frames):
        sizes = [c.size // 1024 for c in L.chunks[b]]
        assert sizes == [fpc] * (f // fpc) + ([f % fpc] if f % fpc else []), (b, sizes, f)
    for b, u in enumerate(utts):
        alone = stream([u], True)[1][0]
        assert np.array_equal(codes[b], alone), (b, u)
        np.testing.assert_array_equal(L.audio(b), codec.decode(np.ascontiguousarray(codes[b].T)), err_msg=f"utterance {u}")
    Ls, codes_s = stream(utts, False)
    for b, u in enumerate(utts):
        assert np.array_equal(codes_s[b], codes[b]), (b, u)
        assert [c.size for c in Ls.chunks[b]] == [c.size for c in L.chunks[b]], (b, u)
        for k, chunk in enumerate(Ls.chunks[b]):
            own = codec.decode(np.ascontiguousarray(codes[b][k * fpc:k * fpc + chunk.size // 1024].T))
            np.testing.assert_array_equal(chunk, own, err_msg=f"utterance {u} chunk {k}")


def test_argument_errors_leave_device_usable(ma, dev, codec, toks, singles, one_shots):
    bad = [t.copy() for t in toks]
    bad[-1][0] = 5000  # a token id out of range in the LAST utterance: refused before anything runs
    cases = [dict(tokens=toks, slots=4, codec=None), dict(tokens=toks, slots=0), dict(tokens=toks, slots=dev.max_batch() + 1),
             dict(tokens=bad, slots=4)]
    for kw in cases:
        tk, cd = kw.pop("tokens"), kw.pop("codec", codec)
        L = Listener(len(toks))
        with pytest.raises(ma.MagpieError, match="MP_ERR_ARG"):
            dev.stream_queue(cd, tk, L, speakers=SPKS, max_dec_steps=STEPS, **kw)
        assert L.events == []
        r = dev.synthesize([toks[0]], speakers=[SPKS[0]], max_dec_steps=STEPS)
        assert np.array_equal(r.codes[0], singles[0])
        np.testing.assert_array_equal(codec.decode(np.ascontiguousarray(singles[0].T)), one_shots[0])
    L = Listener(len(toks))
    res = dev.stream_queue(codec, toks, L, speakers=SPKS, slots=4, continuous=True, max_dec_steps=STEPS)
    _assert_codes(res, singles)
    np.testing.assert_array_equal(L.audio(3), one_shots[3])


@pytest.mark.parametrize("continuous", [1, 0])
def test_cpp_streaming_queue_probe(ma, eos_model, codec_model, continuous):
    """magpie_synthesize_streaming_queue (include/magpie.h) through bin/magpie-stream-queue-probe"""
    exe = os.path.join(ma.PKG_DIR, "bin", "magpie-stream-queue-probe")
    out = subprocess.run([exe, eos_model, codec_model, "2", "24", str(continuous)] + [str(n) for n in (8, 43, 33, 48, 1, 23)],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr[-2000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert r["ok"] and r["equal"] and r["continuous"] == bool(continuous), r
    assert len(r["frames"]) == 6 and all(0 < f <= 24 for f in r["frames"]), r
