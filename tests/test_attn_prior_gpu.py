"""The attention prior on the device (mp_hip_set_attn_prior) against the numpy f64 restatement
of tests/attn_prior_cases.py, built from tests/golden/make_indep.py's Magpie with the semantics
of include/magpie_hip.h.
The token seeds were chosen on the CPU: the reference's own decisions are no near-ties (asserted
per case) and the prior changes codes and alignment entries against the plain run."""
import contextlib

import numpy as np
import pytest

from attn_prior_cases import EPS, MIN_ALIGN_MARGIN, MIN_MARGIN, mi, restate

pytestmark = pytest.mark.gpu

STEPS = 12
# (T, XA form, W, start_step, layers) -> token seed
CASES = [(5, "reassoc", 1, 0, 0, 124), (70, "reassoc", 5, 0, 0, 1), (70, "direct", 5, 2, 0, 2), (70, "reassoc", 5, 0, 2, 20)]


@pytest.fixture(scope="module")
def ma():
    import magpie_amd
    if magpie_amd.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    return magpie_amd


@pytest.fixture(scope="module")
def model64(small_model):
    return mi.Magpie(small_model)


@contextlib.contextmanager
def device(ma, *a, **kw):
    dev = ma.Device(*a, **kw)
    try:
        yield dev
    finally:
        dev.close()


def run(dev, toks, prior=None, speakers=None, steps=STEPS, **kw):
    """(SynthResult, att) of a traced greedy batch; prior: (eps, W, start, layers) or None"""
    dev.set_attn_prior(*(prior or (None,)))
    r = dev.synthesize(toks, speakers=speakers or [0] * len(toks), max_dec_steps=steps, trace=True, **kw)
    return r, (dev.alignment() if prior else None)


def same_bits(r0, a0, b0, r1, a1, b1):
    n = int(r0.n_frames[b0])
    assert n == int(r1.n_frames[b1]) and np.array_equal(r0.codes[b0], r1.codes[b1])
    assert np.array_equal(r0.hidden[b0, :n + 1].view(np.uint32), r1.hidden[b1, :n + 1].view(np.uint32))
    if a0 is not None and a1 is not None:
        assert np.array_equal(a0[b0, :n], a1[b1, :n])


@pytest.mark.parametrize("T,xa,W,start,layers,seed", CASES)
def test_matches_f64_restatement(ma, small_model, model64, T, xa, W, start, layers, seed):
    tok = ma.synthetic_tokens(T, seed=seed)
    ref = restate(model64, tok, 0, STEPS, EPS, W, start, layers)
    plain = restate(model64, tok, 0, STEPS, None, W, start, layers)
    n = len(ref["codes"])
    assert ref["margins"].min() >= MIN_MARGIN and ref["amargins"].min() >= MIN_ALIGN_MARGIN  # the reference alone
    m = min(n, len(plain["codes"]))
    dc, da = int((ref["codes"][:m] != plain["codes"][:m]).sum()), int((ref["att"][:m] != plain["att"][:m]).sum())
    print(f"T {T} {xa} W {W} start {start} layers {layers}: {dc} codes and {da} att entries differ from the plain run")
    if T > W + 2:
        assert dc >= 1 and da >= 1
    with device(ma, small_model, xa=xa) as dev:
        r, att = run(dev, [tok], (EPS, W, start, layers))
    assert int(r.n_frames[0]) == n == STEPS and np.array_equal(r.codes[0], ref["codes"])
    assert np.array_equal(att[0, :STEPS], ref["att"])  # the max_dec_steps-th frame's entry included
    err = np.abs(r.hidden[0, :len(ref["hidden"])].astype(np.float64) - ref["hidden"]).max()
    print(f"  hidden max abs err {err:.2e}")
    assert err < 2e-5


@pytest.mark.parametrize("T,eps", [(70, 1.0), (3, EPS)])
def test_no_ops_are_exact(ma, small_model, T, eps):
    tok = ma.synthetic_tokens(T, seed=11)
    with device(ma, small_model) as dev:
        plain, _ = run(dev, [tok])
        r, att = run(dev, [tok], (eps, 5, 0, 0))
    same_bits(r, None, 0, plain, None, 0)
    a = att[0, :int(r.n_frames[0])]
    assert a.min() >= 0 and a.max() <= T - 1 and np.all(np.diff(a) >= 0)


@pytest.mark.parametrize("weights,lens,singles", [("f32", [70, 5, 12], [0, 1, 2]), ("bf16", [70, 5, 12, 33] * 4, [0, 7, 15])])
def test_batch_equals_single(ma, small_model, weights, lens, singles):
    toks = [ma.synthetic_tokens(n, seed=100 + b) for b, n in enumerate(lens)]
    spk = [b % 5 for b in range(len(lens))]
    with device(ma, small_model, weights=weights) as dev:
        rb, ab = run(dev, toks, (EPS, 5, 0, 0), spk)
        for b in singles:
            r1, a1 = run(dev, [toks[b]], (EPS, 5, 0, 0), [spk[b]])
            same_bits(rb, ab, b, r1, a1, 0)


def test_guidance_scale_one_is_the_prior_alone(ma, small_model):
    toks = [ma.synthetic_tokens(n, seed=60 + n) for n in (70, 9)]
    with device(ma, small_model) as dev:
        alone, a0 = run(dev, toks, (EPS, 5, 0, 0))
        dev.set_cfg(1.0)
        guided, a1 = run(dev, toks, (EPS, 5, 0, 0))
    for b in range(2):
        same_bits(guided, a1, b, alone, a0, b)


def test_eos_stopped_slot_is_frozen(ma, eos_model):
    """the stopped slots sit frozen until the poll at 8: they equal single runs that end at the stop"""
    toks = [ma.synthetic_tokens(40, seed=7), ma.synthetic_tokens(52, seed=9)]
    with device(ma, eos_model) as dev:
        rb, ab = run(dev, toks, (EPS, 3, 0, 0), [0, 1], steps=64)
        assert 0 < int(rb.n_frames.min()) < 8
        for b in range(2):
            r1, a1 = run(dev, [toks[b]], (EPS, 3, 0, 0), [b], steps=int(rb.n_frames[b]) + 1)
            same_bits(rb, ab, b, r1, a1, 0)


def test_refusals_leave_the_device_usable(ma, small_model, codec_model):
    tok = ma.synthetic_tokens(16, seed=1000)
    codec = ma.Codec(codec_model)
    with device(ma, small_model) as dev:
        want, _ = run(dev, [tok])
        for bad in ((0.0, 5, 0, 0), (1.5, 5, 0, 0), (float("nan"), 5, 0, 0), (EPS, -1, 0, 0), (EPS, 5, -1, 0)):
            with pytest.raises(ma.MagpieError, match="MP_ERR_ARG"):
                dev.set_attn_prior(*bad)
        dev.set_attn_prior(EPS, 5, 0, 0)
        with pytest.raises(ma.MagpieError, match="MP_ERR_UNSUPPORTED"):
            dev.synthesize_queue([tok, tok], slots=2, max_dec_steps=STEPS)
        with pytest.raises(ma.MagpieError, match="MP_ERR_UNSUPPORTED"):
            dev.stream_queue(codec, [tok, tok], lambda u, s: True, slots=2, max_dec_steps=STEPS)
        got, _ = run(dev, [tok])
        same_bits(got, None, 0, want, None, 0)
    codec.close()


@pytest.mark.parametrize("weights,model", [("f16", "f16_model"), ("q8", "q8_model")])
def test_unsupported_weight_modes_refuse(ma, request, weights, model):
    tok = ma.synthetic_tokens(16, seed=1000)
    with device(ma, request.getfixturevalue(model), weights=weights) as dev:
        want, _ = run(dev, [tok])
        dev.set_attn_prior(EPS, 5, 0, 0)
        with pytest.raises(ma.MagpieError, match="MP_ERR_UNSUPPORTED"):
            dev.begin([tok], max_dec_steps=STEPS)
        same_bits(run(dev, [tok])[0], None, 0, want, None, 0)
