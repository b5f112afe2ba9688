"""mp_hip_set_sampling on the device (the float64 definition, table and margin rule: test_nucleus_cpu.py)."""
import os

import numpy as np
import pytest

import pick_cases as pc
from test_nucleus_cpu import CASES, FRAMES, SEED, expected

pytestmark = pytest.mark.gpu
MIX = [(0.0, 80, 1.0, 0.0), (0.7, 80, 1.0, 0.0), (0.7, 2024, 0.5, 0.0), (0.7, 2024, 1.0, 0.1), (0.7, 2024, 0.9, 0.0)]


@pytest.fixture(scope="module")
def ma():
    import magpie_amd
    if magpie_amd.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    return magpie_amd


@pytest.fixture(scope="module")
def crafted_devs(ma, small_model):
    held = {}

    def get(name, weights):
        if (name, weights) not in held:
            src = pc.moved_source(ma) if name == "moved" else small_model
            held[(name, weights)] = ma.Device(pc.crafted(src, name), weights=weights)
            held[(name, weights)].lt_calls = 0
        return held[(name, weights)]
    yield get
    for d in held.values():
        d.close()


def _toks(ma, b):
    return ma.synthetic_tokens(6 + b % 5, seed=900 + b)


def _hold(oracle, case, codes, stream, steps):
    want, ok, _ = expected(oracle, case, stream, steps)
    bad = np.argwhere((np.asarray(codes).reshape(-1, 8) != want) & ok)
    assert len(bad) == 0, (case[0], stream, [(int(f), int(c), int(np.asarray(codes)[f, c]), int(want[f, c])) for f, c in bad[:8]])


@pytest.mark.parametrize("site", ["lt_sample", "f32_b1", "bf16_b32"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_against_float64(ma, oracle, crafted_devs, case, site):
    d = crafted_devs(case[1], "bf16" if site == "bf16_b32" else "f32")
    d.set_sampling(case[2:])
    try:
        if site == "lt_sample":  # stream -1, step 4 + the device's call count; the call's own T and k are not read
            rng = np.random.default_rng(1)
            got = [d.lt_sample(rng.standard_normal(768).astype(np.float32), 0.0, 80, True, SEED)[0] for _ in range(FRAMES)]
            _hold(oracle, case, got, -1, range(4 + d.lt_calls, 4 + d.lt_calls + FRAMES))
            d.lt_calls += FRAMES
            return
        slots = (0,) if site == "f32_b1" else (0, 15, 16, 31)
        B = max(slots) + 1
        r = d.synthesize([_toks(ma, b) for b in range(B)], speakers=[b % 5 for b in range(B)], max_dec_steps=FRAMES,
                         temperature=0.0, seed=SEED, ignore_eos=True)
        for b in slots:
            assert r.n_frames[b] == FRAMES
            _hold(oracle, case, r.codes[b], b, range(FRAMES))
    finally:
        d.set_sampling(None)


@pytest.mark.parametrize("model,weights,B,scale", [("small_model", "f32", 5, 0.0), ("small_model", "bf16", 17, 0.0),
                                                   ("q8_model", "f32", 4, 0.0), ("small_model", "f32", 2, 2.5)])
def test_a_mixed_batch_equals_its_single_runs(ma, request, model, weights, B, scale):
    d = ma.Device(request.getfixturevalue(model), weights=weights)
    d.set_cfg(scale)
    mix = [MIX[b % len(MIX)] for b in range(B)]
    kw = dict(max_dec_steps=FRAMES, seed=SEED, ignore_eos=True, trace=True)
    toks = [_toks(ma, b) for b in range(B)]
    d.set_sampling(mix)
    r = d.synthesize(toks, speakers=[b % 5 for b in range(B)], **kw)
    for b in range(B):
        d.set_sampling(mix[b])
        s = d.synthesize([toks[b]], speakers=[b % 5], stream_base=b, **kw)
        assert np.array_equal(r.codes[b], s.codes[0]), b
        assert np.array_equal(r.hidden[b], s.hidden[0]), b
        if scale:
            assert np.array_equal(r.hidden_uncond[b], s.hidden_uncond[0]), b
    d.close()


def test_pools_follow_the_utterance(ma, codec_model):
    eos = ma.synth_gguf(os.path.join(os.environ.get("MAGPIE_CACHE", "/tmp/magpie_amd_cache"), "magpie_small_eosb0.09.gguf"),
                        dec_layers=2, enc_layers=1, eos_bias=0.09)
    d, codec = ma.Device(eos, xa="reassoc"), ma.Codec(codec_model)
    toks = [ma.synthetic_tokens(n, seed=1700 + i) for i, n in enumerate((8, 43, 33, 48, 23))]
    kw = dict(max_dec_steps=24, seed=SEED)
    singles = []
    for i, t in enumerate(toks):
        d.set_sampling(MIX[i])
        singles.append(d.synthesize([t], speakers=[i % 5], stream_base=i, **kw).codes[0])
    assert len({len(s) for s in singles}) > 1, "different lengths"
    res = d.synthesize_queue(toks, [i % 5 for i in range(5)], slots=2, sampling=MIX, **kw)
    stm = d.stream_queue(codec, toks, lambda utt, audio: True, speakers=[i % 5 for i in range(5)], slots=2, continuous=True,
                         sampling=MIX, **kw)
    for i, s in enumerate(singles):
        assert np.array_equal(res.codes[i], s) and np.array_equal(stm.codes[i], s), i
    d.close()
    codec.close()


def test_off_is_off_and_refusals(ma, small_model):
    d = ma.Device(small_model)
    toks = [_toks(ma, b) for b in range(2)]
    kw = dict(max_dec_steps=FRAMES, seed=SEED, ignore_eos=True, trace=True)
    plain = {T: d.synthesize(toks, temperature=T, top_k=80, **kw) for T in (0.0, 0.7)}

    def same(T):
        r = d.synthesize(toks, temperature=T, top_k=80, **kw)
        return all(np.array_equal(a, b) for a, b in zip(r.codes, plain[T].codes)) and np.array_equal(r.hidden, plain[T].hidden)
    d.set_sampling((0.7, 2024, 0.9, 0.0))
    assert not all(np.array_equal(a, b) for a, b in zip(d.synthesize(toks, temperature=0.0, **kw).codes, plain[0.0].codes))
    d.set_sampling([(0.0, 80, 1.0, 0.0), (0.001, 0, 0.3, 0.2)])  # every utterance greedy: the plain greedy run
    assert same(0.0)
    d.set_sampling(None)
    assert same(0.0) and same(0.7)
    for bad in [(0.7, 80, 0.0, 0.0), (0.7, 80, 1.5, 0.0), (0.7, 80, float("nan"), 0.0), (0.7, 80, 1.0, 1.0), (0.7, 80, 1.0, -0.1),
                (0.7, 80, 1.0, float("inf")), (0.7, 0, 1.0, 0.0), (0.7, 2025, 1.0, 0.0)]:
        with pytest.raises(ma.MagpieError):
            d.set_sampling(bad)
    d.set_sampling([MIX[1]] * 3)  # n != B
    with pytest.raises(ma.MagpieError):
        d.synthesize(toks, **kw)
    d.set_sampling(None)
    assert same(0.7)
    d.close()
