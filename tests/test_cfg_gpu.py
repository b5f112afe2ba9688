"""Classifier-free guidance on the device (mp_hip_set_cfg, Device.set_cfg): a guided
utterance is two decode slots whose logits are mixed in every code pick.

  parity      the f32 path against the numpy f64 restatement (tests/golden/make_cfg.py,
              cfg_small.npz; no stored decision is a near-tie, tests/test_cfg_cpu.py): every
              frame's codes, n_frames, and both branches' hidden traces within 2e-5, the bar
              tests/test_indep_gpu.py holds the plain decode to
  identity    at scale 1 the mix is the conditional logit exactly: the plain run's codes
  pairs       a guided batch reproduces each utterance's guided run alone, bit for bit
  graph       the scale lives in device memory: one captured graph serves 2.5, then 1.0
  streaming, refusals, and off = the plain decode
"""
import os

import numpy as np
import pytest

from parity import compare_codes

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")

# mp_hip_begin_batch under guidance: f32 (as stored) and bf16 weights run
GUIDED_MODES = ["f32", "bf16"]


@pytest.fixture(scope="module")
def ma():
    import magpie_amd
    if magpie_amd.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    return magpie_amd


@pytest.fixture(scope="module")
def cfg():
    return np.load(os.path.join(GOLD, "cfg_small.npz"))


@pytest.fixture(scope="module")
def indep():
    return np.load(os.path.join(GOLD, "indep_small.npz"))


@pytest.fixture(scope="module")
def eos_model(ma):
    """the slot pool tests' model: EOS live, utterances of unequal length"""
    cache = os.environ.get("MAGPIE_CACHE", "/tmp/magpie_amd_cache")
    os.makedirs(cache, exist_ok=True)
    return ma.synth_gguf(os.path.join(cache, "magpie_small_eosb0.09.gguf"), dec_layers=2, enc_layers=1, eos_bias=0.09)


def _cases(d):
    n = 0
    while f"g{n}_tokens" in d:
        n += 1
    return range(n)


def _kw(d, i):
    spk, steps = (int(v) for v in d[f"g{i}_meta"])
    temp, top_k, seed, stream = d[f"g{i}_sampling"]
    kw = dict(speakers=[spk], max_dec_steps=steps)
    if temp >= 0.01:
        kw.update(temperature=float(temp), top_k=int(top_k), seed=int(seed), stream_base=int(stream))
    return kw


def _plain_equals_indep(dev, indep):
    """the known plain codes (tests/test_indep_gpu.py's first case) on this device"""
    spk, steps = (int(v) for v in indep["c0_meta"])
    r = dev.synthesize([indep["c0_tokens"]], speakers=[spk], max_dec_steps=steps, trace=True)
    np.testing.assert_array_equal(r.codes[0], indep["c0_codes"])
    assert r.hidden_uncond is None
    return r


def test_guided_decode_matches_restatement(ma, small_model, cfg):
    dev = ma.Device(small_model)
    try:
        for i in _cases(cfg):
            dev.set_cfg(float(cfg[f"g{i}_scale"]))
            r = dev.synthesize([cfg[f"g{i}_tokens"]], trace=True, **_kw(cfg, i))
            ref = cfg[f"g{i}_codes"]
            res = compare_codes(r.codes[0], ref, cfg[f"g{i}_margins"], min_frames=None)
            assert res["identical"] and int(r.n_frames[0]) == len(ref)
            for name, got in (("hidden", r.hidden), ("hidden_uncond", r.hidden_uncond)):
                want = cfg[f"g{i}_{name}"].astype(np.float64)
                err = np.abs(got[0, :len(want)].astype(np.float64) - want).max()
                print(f"case {i} (scale {float(cfg[f'g{i}_scale'])}): {len(ref)} frames identical, {name} max abs err {err:.2e}")
                assert err < 2e-5
    finally:
        dev.close()


@pytest.mark.parametrize("kv", ["f32", "bf16"])
@pytest.mark.parametrize("weights", GUIDED_MODES)
def test_scale_one_is_the_plain_run(ma, small_model, weights, kv):
    toks = [ma.synthetic_tokens(n, seed=40 + n) for n in (9, 21, 14)]
    dev = ma.Device(small_model, weights=weights, kv=kv)
    try:
        for smp in (dict(), dict(temperature=0.7, top_k=80, seed=5, stream_base=3)):
            kw = dict(speakers=[0, 2, 4], max_dec_steps=8, **smp)
            dev.set_cfg(0.0)
            plain = dev.synthesize(toks, **kw)
            dev.set_cfg(1.0)
            guided = dev.synthesize(toks, **kw)
            assert np.array_equal(guided.n_frames, plain.n_frames)
            for b in range(3):
                assert np.array_equal(guided.codes[b], plain.codes[b]), (weights, kv, smp, b)
    finally:
        dev.close()


@pytest.mark.parametrize("weights", GUIDED_MODES)
def test_pairs_are_independent(ma, eos_model, weights):
    """Natural EOS is live: at scale 1.25 the 43-token utterance ends within a few frames
    (frame 5 in the f64 restatement) while the others run on, so its pair sits frozen in
    the batch for most of the decode."""
    steps, scale = 24, 1.25
    lens = [8 + 5 * ((7 * i) % 9) for i in range(9)]  # the slot pool tests' mix
    pick, spks = [0, 1, 8], [0, 1, 3]
    toks = [ma.synthetic_tokens(lens[i], seed=1700 + i) for i in pick]
    assert len({len(t) for t in toks}) == 3
    dev = ma.Device(eos_model, weights=weights)
    try:
        dev.set_cfg(scale)
        batch = dev.synthesize(toks, speakers=spks, max_dec_steps=steps, trace=True)
        nf = [int(n) for n in batch.n_frames]
        print(f"{weights}: guided frames {nf}")
        assert min(nf) < max(nf) and min(nf) < steps - 8  # one pair ends while others continue
        for b in range(3):
            alone = dev.synthesize([toks[b]], speakers=[spks[b]], max_dec_steps=steps, trace=True, stream_base=b)
            assert int(alone.n_frames[0]) == nf[b]
            assert np.array_equal(alone.codes[0], batch.codes[b]), b
            # rows 0 .. n: written by the live pair, row n again by every frozen iteration; the
            # rest never
            n = nf[b] if nf[b] < steps else steps - 1
            for got, want in ((batch.hidden, alone.hidden), (batch.hidden_uncond, alone.hidden_uncond)):
                assert np.array_equal(got[b, :n + 1], want[0, :n + 1]), b
                assert not got[b, n + 1:].any() and got[b, n].any()
    finally:
        dev.close()


def test_scale_is_live_in_the_graph(ma, small_model, cfg, indep):
    """two begin + decode calls of one shape: the second reuses the captured graph"""
    assert float(cfg["g0_scale"]) == 2.5 and cfg["g0_sampling"][0] < 0.01
    tok, kw = cfg["g0_tokens"], _kw(cfg, 0)
    dev = ma.Device(small_model)
    try:
        dev.set_cfg(2.5)
        a = dev.synthesize([tok], **kw)
        dev.set_cfg(1.0)
        b = dev.synthesize([tok], **kw)
        dev.set_cfg(0.0)
        plain = dev.synthesize([tok], **kw)
    finally:
        dev.close()
    np.testing.assert_array_equal(a.codes[0], cfg["g0_codes"])
    np.testing.assert_array_equal(b.codes[0], plain.codes[0])
    assert not np.array_equal(a.codes[0], plain.codes[0])


def test_streaming_delivers_the_guided_codes(ma, small_model, codec_model):
    toks = [ma.synthetic_tokens(n, seed=70 + n) for n in (7, 19, 12)]
    codec = ma.Codec(codec_model)
    dev = ma.Device(small_model)
    try:
        dev.set_cfg(2.5)
        chunks = {}

        def on_audio(utt, samples):
            chunks.setdefault(utt, []).append(samples)
            return True
        codes, total, _ = dev.synthesize_stream(codec, toks, on_audio, speakers=[1, 0, 3], max_dec_steps=10,
                                                frames_per_chunk=4)
        ref = dev.synthesize(toks, speakers=[1, 0, 3], max_dec_steps=10)
        dev.set_cfg(0.0)
        plain = dev.synthesize(toks, speakers=[1, 0, 3], max_dec_steps=10)
    finally:
        dev.close()
        codec.close()
    assert sorted(chunks) == [0, 1, 2]  # audio for the 3 utterances, none for their partners
    assert total == 3 * 10 * 1024
    for b in range(3):
        assert np.array_equal(codes[b], ref.codes[b]), b
        assert [len(c) for c in chunks[b]] == [4096, 4096, 2048]
    assert any(not np.array_equal(ref.codes[b], plain.codes[b]) for b in range(3))


def test_refusals_leave_the_device_usable(ma, small_model, codec_model, indep):
    toks = [ma.synthetic_tokens(6 + b, seed=90 + b) for b in range(5)]
    codec = ma.Codec(codec_model)
    dev = ma.Device(small_model)
    try:
        assert dev.max_batch() == 8
        # a non-finite scale
        for bad in (float("nan"), float("inf")):
            with pytest.raises(ma.MagpieError, match="MP_ERR_ARG"):
                dev.set_cfg(bad)
        _plain_equals_indep(dev, indep)
        # 2 B > max_batch
        dev.set_cfg(2.5)
        with pytest.raises(ma.MagpieError, match="MP_ERR_ARG.*half of mp_hip_max_batch = 8"):
            dev.synthesize(toks, max_dec_steps=4)
        dev.set_cfg(0.0)
        _plain_equals_indep(dev, indep)
        # the slot pool
        dev.set_cfg(2.5)
        with pytest.raises(ma.MagpieError, match="MP_ERR_UNSUPPORTED"):
            dev.synthesize_queue(toks, slots=2, max_dec_steps=4)
        dev.set_cfg(0.0)
        _plain_equals_indep(dev, indep)
        dev.set_cfg(2.5)
        with pytest.raises(ma.MagpieError, match="MP_ERR_UNSUPPORTED"):
            dev.stream_queue(codec, toks, lambda u, a: True, slots=2, max_dec_steps=4)
        dev.set_cfg(0.0)
        _plain_equals_indep(dev, indep)
    finally:
        dev.close()
        codec.close()


@pytest.mark.parametrize("weights,model", [("f16", "f16_model"), ("q8", "q8_model"), ("q4", "q4_model")])
def test_unsupported_weight_modes_refuse_guidance(ma, request, weights, model):
    """F16 and Q8_0 / Q4_0 are documented as refused (include/magpie_hip.h): MP_ERR_UNSUPPORTED
    from mp_hip_begin_batch, and the same device then decodes plainly, as a fresh one does."""
    path = request.getfixturevalue(model)
    tok = ma.synthetic_tokens(10, seed=33)
    fresh = ma.Device(path, weights=weights)
    want = fresh.synthesize([tok], max_dec_steps=6)
    fresh.close()
    dev = ma.Device(path, weights=weights)
    try:
        dev.set_cfg(2.5)
        with pytest.raises(ma.MagpieError, match="MP_ERR_UNSUPPORTED"):
            dev.synthesize([tok], max_dec_steps=6)
        dev.set_cfg(0.0)
        got = dev.synthesize([tok], max_dec_steps=6)
    finally:
        dev.close()
    assert np.array_equal(got.codes[0], want.codes[0]) and len(got.codes[0]) == 6


def test_off_is_off(ma, small_model, indep):
    dev = ma.Device(small_model)
    try:
        dev.set_cfg(2.5)
        dev.synthesize([indep["c0_tokens"]], max_dec_steps=4)
        dev.set_cfg(0.0)
        i = 0
        while f"c{i}_tokens" in indep:
            spk, steps = (int(v) for v in indep[f"c{i}_meta"])
            r = dev.synthesize([indep[f"c{i}_tokens"]], speakers=[spk], max_dec_steps=steps, trace=True)
            ref_hidden = indep[f"c{i}_hidden"]
            np.testing.assert_array_equal(r.codes[0], indep[f"c{i}_codes"])
            assert np.abs(r.hidden[0, :len(ref_hidden)].astype(np.float64) - ref_hidden).max() < 2e-5
            assert r.hidden_uncond is None
            i += 1
        assert i >= 2
    finally:
        dev.close()
