"""PCM output of the codec: on-device resampling to 8-48 kHz and 16-bit samples
(mp_hip_codec_decode_pcm, mp_hip_codec_stream_decode_pcm; definition in include/magpie_hip.h).

_table / _resample64 restate that definition in float64 with numpy alone. The f32 bar: the
accumulation error is at most (NT + 2) 2^-24 sum|h| max|x| and the coefficients' rounding at most
NT 2^-24 max|h|; with |x| <= 1 (the codec's tanh), sum|h| < 1.97 and NT <= 90 that is 1.2e-5, under
the project's f32 bar of 2e-5.
"""
import os
import struct
import subprocess
from math import ceil, gcd

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
F32, S16 = 0, 1


def _table(rate):
    g = gcd(rate, 22050)
    L, M = rate // g, 22050 // g
    if L == M:
        return L, M, np.ones((1, 1))
    s = max(1.0, M / L)
    NT = 2 * ceil(16 * s)
    C, fc = NT // 2, 0.9 / s
    d = np.arange(NT)[None, :] + np.arange(L)[:, None] / L - C
    w = np.i0(9.0 * np.sqrt(np.clip(1 - (d / C) ** 2, 0, None))) / np.i0(9.0)
    h = np.where(np.abs(d) < C, fc * np.sinc(fc * d) * w, 0.0)
    return L, M, h / h.sum(1, keepdims=True)


def _resample64(x, rate):
    L, M, h = _table(rate)
    NT = h.shape[1]
    n = np.arange(-(-len(x) * L // M), dtype=np.int64)
    xp = np.concatenate([np.zeros(NT - 1), x.astype(np.float64)])
    return (h[n * M % L] * xp[(n * M // L + NT - 1)[:, None] - np.arange(NT)[None, :]]).sum(1)


def _count(samples, rate):
    g = gcd(rate, 22050)
    return -(-samples * (rate // g) // (22050 // g))


@pytest.fixture(scope="module")
def ma():
    import magpie_amd
    if magpie_amd.device_count() < 1:
        pytest.fail("no HIP device visible")
    return magpie_amd


@pytest.fixture(scope="module")
def codec(ma, codec_model):
    c = ma.Codec(codec_model)
    yield c
    c.close()


@pytest.fixture(scope="module")
def codes():
    return np.random.default_rng(7).integers(0, 2016, (2, 8, 9)).astype(np.int32)  # two lanes' 9 frames


@pytest.mark.parametrize("rate", [8000, 16000, 22050, 24000, 44100, 48000])
def test_against_f64(ma, codec, codes, rate):
    x = codec.decode(codes[0, :, :3])
    y = codec.decode_pcm(codes[0, :, :3], rate, F32)
    assert y.dtype == np.float32 and len(y) == _count(3 * 1024, rate) == ma.pcm_samples(3, rate)
    if rate == 22050:
        assert y.tobytes() == x.tobytes()
        return
    err = float(np.abs(y - _resample64(x, rate)).max())
    print(f"{rate} Hz: max abs err vs f64 {err:.3g} (max |x| {np.abs(x).max():.3f})")
    assert err < 2e-5


@pytest.mark.parametrize("fmt", [F32, S16])
@pytest.mark.parametrize("rate", [8000, 48000])
def test_chunks_equal_one_shot(codec, codes, rate, fmt):
    sizes = [[1, 4, 3, 1], [4, 1, 1, 3]]
    s = codec.stream(2)
    at, got, first = [0, 0], [[], []], None
    for a, b in zip(*sizes):
        out = s.decode_pcm([codes[0][:, at[0]:at[0] + a], codes[1][:, at[1]:at[1] + b]], [a, b], rate, fmt)
        first = out if first is None else first
        for q, n in enumerate((a, b)):
            assert len(out[q]) == _count((at[q] + n) * 1024, rate) - _count(at[q] * 1024, rate)
            got[q].append(out[q])
            at[q] += n
    for q in range(2):
        assert np.concatenate(got[q]).tobytes() == codec.decode_pcm(codes[q], rate, fmt).tobytes()
    s.reset(1)
    again = s.decode_pcm([codes[1][:, :4]], [4], rate, fmt, lanes=[1])
    assert again[0].tobytes() == first[1].tobytes()
    s.close()


@pytest.mark.parametrize("rate", [22050, 16000])
def test_s16_is_the_reference_conversion(codec, codes, rate):
    f = codec.decode_pcm(codes[0], rate, F32)
    s = codec.decode_pcm(codes[0], rate, S16)
    assert s.dtype == np.int16
    assert np.array_equal(s, np.trunc(np.clip(f, -1, 1) * np.float32(32767)).astype(np.int16))
    # No input of the synthetic codec saturates (observed: [-0.595, 0.579] at 22 050 Hz, [-0.535, 0.562]
    # at 16 000 Hz), so the clamp itself is not reached here: both signs and over half of full scale are.
    print(f"{rate} Hz: f32 range [{f.min():.4f}, {f.max():.4f}], s16 range [{s.min()}, {s.max()}]")
    assert f.min() < -0.5 and 0.5 < f.max() and np.abs(f).max() < 1.0


def test_refusals(ma, codec, codes):
    good = codec.decode_pcm(codes[0, :, :2], 16000, S16)
    for kw, err in [(dict(rate=11025, fmt=S16), "MP_ERR_ARG"), (dict(rate=16000, fmt=2), "MP_ERR_ARG"),
                    (dict(rate=16000, fmt=S16, cap=len(good) - 1), "MP_ERR_ARG.*" + str(len(good)))]:
        with pytest.raises(ma.MagpieError, match=err):
            codec.decode_pcm(codes[0, :, :2], **kw)
        assert np.array_equal(codec.decode_pcm(codes[0, :, :2], 16000, S16), good)
    s = codec.stream(1)
    a = s.decode_pcm([codes[0, :, :2]], [2], 16000, S16)[0]
    with pytest.raises(ma.MagpieError, match="MP_ERR_STATE"):
        s.decode_pcm([codes[0, :, 2:4]], [2], 8000, S16)
    b = s.decode_pcm([codes[0, :, 2:4]], [2], 16000, S16)[0]  # the refused call advanced nothing
    assert np.array_equal(np.concatenate([a, b]), codec.decode_pcm(codes[0, :, :4], 16000, S16))
    s.reset(-1)
    assert len(s.decode_pcm([codes[0, :, :2]], [2], 8000, S16)[0]) == ma.pcm_samples(2, 8000)
    s.close()


def test_cli_sample_rate(ma, small_model, codec_model, tmp_path):
    exe = os.path.join(os.path.dirname(ma.LIB_PATH), "..", "bin", "magpie-tts")
    raw = {}
    for name, extra in [("plain", []), ("r22", ["--sample-rate", "22050"]), ("r16", ["--sample-rate", "16000"])]:
        out = str(tmp_path / (name + ".wav"))
        r = subprocess.run([exe, "-m", small_model, "-c", codec_model, "-t", "Hello, world!", "-o", out, "--temp", "0",
                            "-q", *extra], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        raw[name] = open(out, "rb").read()
    assert raw["r22"] == raw["plain"]
    rate, brate = struct.unpack("<II", raw["r16"][24:32])
    frames = (len(raw["plain"]) - 44) // 2 // 1024
    assert (rate, brate) == (16000, 32000) and len(raw["r16"]) == 44 + 2 * ma.pcm_samples(frames, 16000)
