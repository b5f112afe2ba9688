"""Reloading models on one device handle (mp_hip_load_model_ex called again and again).

magpie_model_load reloads on one mp_dev by default (Q8, then F16, then as stored), so a
load must leave nothing of the previous model behind: not its weight views, not the batch,
not the slot pool's staging workspaces, not the LT-sample scratch. After every load of the
walk below the handle must compute exactly what a fresh handle on the same file and weight
mode computes, and a failed load must leave the handle empty and loadable.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MP_ERR_IO, MP_ERR_STATE, MP_ERR_UNSUPPORTED = -3, -5, -6
STEPS = 6


@pytest.fixture(scope="module")
def ma():
    import magpie_amd
    if magpie_amd.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    return magpie_amd


@pytest.fixture(scope="module")
def l1_model(ma):
    cache = os.environ.get("MAGPIE_CACHE", "/tmp/magpie_amd_cache")
    os.makedirs(cache, exist_ok=True)
    return ma.synth_gguf(os.path.join(cache, "magpie_small_l1e1_k32.gguf"), dec_layers=1, enc_layers=1,
                         lt_head_scale=ma.DECISIVE)


def test_reload_equals_fresh_device(ma, small_model, q8_model, f16_model, l1_model):
    utts = [ma.synthetic_tokens(5, seed=4100), ma.synthetic_tokens(9, seed=4101)]
    queue_utts = utts + [ma.synthetic_tokens(7, seed=4102)]
    hidden = np.random.default_rng(4103).standard_normal(768).astype(np.float32)
    kw = dict(max_dec_steps=STEPS, ignore_eos=True, temperature=0.0)

    def synth(d):
        return d.synthesize(utts, **kw).codes

    def queue(d):
        return d.synthesize_queue(queue_utts, slots=2, **kw).codes

    fresh = {}  # (path, mode) -> what a fresh handle computes

    def reference(path, mode):
        if (path, mode) not in fresh:
            d = ma.Device(path, weights=mode)
            try:
                fresh[path, mode] = {"codes": synth(d), "queue": queue(d), "lt": d.lt_sample(hidden)}
            finally:
                d.close()
        return fresh[path, mode]

    def same(got, want, what):
        assert len(got) == len(want), what
        for b, (g, w) in enumerate(zip(got, want)):
            assert g.shape == (STEPS, 8), f"{what}: utterance {b} has shape {g.shape}"
            assert np.array_equal(g, w), f"{what}: utterance {b} differs from a fresh handle"

    dev = ma.Device(q8_model, weights="q8")  # the walk's first load
    try:
        def load(path, mode):
            return dev.lib.mp_hip_load_model_ex(dev.h, path.encode(), ma.Device.WEIGHT_MODES[mode])

        def check(path, mode, lt=False, with_queue=False):
            ref = reference(path, mode)
            what = f"{os.path.basename(path)} as {mode}"
            assert dev.lib.mp_hip_weight_mode(dev.h) == ma.Device.WEIGHT_MODES[mode], what
            same(synth(dev), ref["codes"], what)
            if lt:
                for g, w in zip(dev.lt_sample(hidden), ref["lt"]):
                    assert np.array_equal(g, w), f"{what}: lt_sample differs from a fresh handle"
            if with_queue:  # leaves the staging workspaces alive for the next load
                same(queue(dev), ref["queue"], what + " (queue)")

        check(q8_model, "q8")
        assert load(small_model, "bf16") == ma.MP_OK
        check(small_model, "bf16", lt=True)
        assert load(f16_model, "f16") == ma.MP_OK
        check(f16_model, "f16", lt=True, with_queue=True)
        assert load(l1_model, "f32") == ma.MP_OK
        assert dev.model_info()["dec_layers"] == 1
        check(l1_model, "f32")

        assert load(small_model, "q8") == MP_ERR_UNSUPPORTED  # an f32 file has no quantised tensors
        assert dev.lib.mp_hip_weight_mode(dev.h) == MP_ERR_STATE
        with pytest.raises(ma.MagpieError):
            dev.begin(utts, **kw)

        assert load(small_model, "f32") == ma.MP_OK
        check(small_model, "f32")

        assert load(os.path.join(os.path.dirname(small_model), "no_such_model.gguf"), "f32") == MP_ERR_IO
        assert dev.lib.mp_hip_weight_mode(dev.h) == MP_ERR_STATE
        assert load(small_model, "f32") == ma.MP_OK
        check(small_model, "f32")
    finally:
        dev.close()
