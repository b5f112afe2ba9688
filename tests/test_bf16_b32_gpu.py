"""32 decode slots in the bf16 weight mode (gemm_b16x2_kernel, mp_decode_b16.hip): a column of
the second 16-column MFMA tile computes what the same utterance computes alone, bit for bit,
in every cache type, XA form, under sampling, guidance, the attention prior and in both slot
pools; one second-tile slot is also held to the oracle's bf16 mode, teacher forced. The other
weight modes keep their limits."""
import os

import numpy as np
import pytest

from parity import compare_forced
from test_configs_gpu import TIE_EPS, _hidden_ok

pytestmark = pytest.mark.gpu

EPS, W = 0.1, 5


@pytest.fixture(scope="module")
def ma():
    import magpie_amd
    if magpie_amd.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    return magpie_amd


def _toks(ma, n, seed):
    return [ma.synthetic_tokens(8 + 3 * (b % 11), seed=seed + b) for b in range(n)], [b % 5 for b in range(n)]


@pytest.mark.parametrize("kv,xa", [("f32", "reassoc"), ("bf16", "reassoc"), ("f32", "direct"), ("bf16", "direct")])
@pytest.mark.parametrize("B", [17, 32])
def test_batch_equals_single(ma, small_model, B, kv, xa):
    toks, spk = _toks(ma, B, 3200)
    kw = dict(max_dec_steps=16, ignore_eos=True, trace=True)
    dev = ma.Device(small_model, weights="bf16", kv=kv, xa=xa)
    try:
        rb = dev.synthesize(toks, speakers=spk, **kw)
        for b in (0, 15, 16, B - 1):
            rs = dev.synthesize([toks[b]], speakers=[spk[b]], **kw)
            assert np.array_equal(rb.codes[b], rs.codes[0]), f"slot {b} codes"
            assert np.array_equal(rb.hidden[b], rs.hidden[0]), f"slot {b} hidden"
    finally:
        dev.close()


def test_second_tile_slot_against_oracle(ma, oracle, full_model):
    B, steps = 32, 32
    toks = [ma.synthetic_tokens(40 + 3 * (b % 16), seed=7000 + b) for b in range(B)]
    spk = [b % 5 for b in range(B)]
    dev = ma.Device(full_model, weights="bf16")
    try:
        rb = dev.synthesize(toks, speakers=spk, max_dec_steps=steps, ignore_eos=True, trace=True)
    finally:
        dev.close()
    om = oracle.Model(full_model)
    om.set_weight_mode(1)
    o = om.synthesize_forced(toks[16], rb.codes[16], speaker=spk[16], ignore_eos=True)
    om.close()
    assert compare_forced(rb.codes[16], o, tie_eps=TIE_EPS, max_ties=6)["decisions"] == steps * 8
    _hidden_ok(rb.hidden[16, :steps + 1], o["hidden"])


def test_sampled_batch_equals_single(ma, small_model):
    toks, spk = _toks(ma, 32, 3300)
    kw = dict(max_dec_steps=16, ignore_eos=True, temperature=0.7, top_k=80, seed=20261)
    dev = ma.Device(small_model, weights="bf16")
    try:
        rb = dev.synthesize(toks, speakers=spk, **kw)
        for b in (16, 31):
            rs = dev.synthesize([toks[b]], speakers=[spk[b]], stream_base=b, **kw)
            assert np.array_equal(rb.codes[b], rs.codes[0]), f"slot {b}"
    finally:
        dev.close()


@pytest.mark.parametrize("cfg,prior", [(2.5, None), (0.0, (EPS, W, 0, 0)), (2.5, (EPS, W, 0, 0))])
@pytest.mark.parametrize("B", [9, 16])
def test_guidance_and_prior_across_the_tiles(ma, small_model, B, cfg, prior):
    """B = 9: 18 slots, partners 9..17 straddle the tile boundary; B = 16: every pair does"""
    toks = [ma.synthetic_tokens(n, seed=3400 + b) for b, n in enumerate(([70, 5, 12, 33] * 4)[:B])]
    spk = [b % 5 for b in range(B)]
    kw = dict(max_dec_steps=12, trace=True)
    dev = ma.Device(small_model, weights="bf16")
    try:
        dev.set_cfg(cfg)
        dev.set_attn_prior(*(prior or (None,)))
        rb = dev.synthesize(toks, speakers=spk, **kw)
        ab = dev.alignment() if prior else None
        for b in (0, 6, 7, B - 1):
            rs = dev.synthesize([toks[b]], speakers=[spk[b]], **kw)
            n = int(rs.n_frames[0])
            assert int(rb.n_frames[b]) == n and np.array_equal(rb.codes[b], rs.codes[0]), f"utterance {b} codes"
            assert np.array_equal(rb.hidden[b], rs.hidden[0]), f"utterance {b} hidden"
            if cfg:
                assert np.array_equal(rb.hidden_uncond[b], rs.hidden_uncond[0]), f"utterance {b} unconditional hidden"
            if prior:
                assert np.array_equal(ab[b, :n], dev.alignment()[0, :n]), f"utterance {b} alignment"
        if cfg:
            with pytest.raises(ma.MagpieError, match="MP_ERR_ARG"):
                dev.begin(toks[:1] * 17, max_dec_steps=12)
    finally:
        dev.close()


def test_pools_at_24_slots(ma, codec_model):
    from test_pool_stream_gpu import Listener
    steps, N = 24, 40
    model = ma.synth_gguf(os.path.join(os.environ.get("MAGPIE_CACHE", "/tmp/magpie_amd_cache"), "magpie_small_eosb0.09.gguf"),
                          dec_layers=2, enc_layers=1, eos_bias=0.09)
    toks = [ma.synthetic_tokens(8 + 5 * ((7 * i) % 9), seed=1900 + i) for i in range(N)]
    spks = [i % 5 for i in range(N)]
    codec = ma.Codec(codec_model)
    dev = ma.Device(model, weights="bf16", xa="reassoc")
    try:
        refs = [dev.synthesize([t], speakers=[spks[i]], max_dec_steps=steps).codes[0] for i, t in enumerate(toks)]
        assert len({len(r) for r in refs}) >= 3  # EOS live: slots free up at different frames
        res = dev.synthesize_queue(toks, spks, slots=24, max_dec_steps=steps)
        L = Listener(N)
        rs = dev.stream_queue(codec, toks, L, speakers=spks, slots=24, continuous=True, max_dec_steps=steps)
        assert res.slots == rs.slots == 24 and res.refills == rs.refills == N - 24
        for i, ref in enumerate(refs):
            assert np.array_equal(res.codes[i], ref), f"queue utterance {i}"
            assert np.array_equal(rs.codes[i], ref), f"stream queue utterance {i}"
            np.testing.assert_array_equal(L.audio(i), codec.decode(np.ascontiguousarray(ref.T)), err_msg=f"utterance {i}")
    finally:
        dev.close()
        codec.close()


@pytest.mark.parametrize("weights,model,limit", [("bf16", "small_model", 32), ("f16", "f16_model", 16), ("f32", "small_model", 8)])
def test_limits(ma, request, weights, model, limit):
    tok = ma.synthetic_tokens(8, seed=3500)
    dev = ma.Device(request.getfixturevalue(model), weights=weights)
    try:
        assert dev.max_batch() == limit
        want = dev.synthesize([tok], max_dec_steps=4, ignore_eos=True).codes[0]
        with pytest.raises(ma.MagpieError, match="MP_ERR_ARG"):
            dev.begin([tok] * (limit + 1), max_dec_steps=4)
        assert np.array_equal(dev.synthesize([tok], max_dec_steps=4, ignore_eos=True).codes[0], want)
    finally:
        dev.close()
