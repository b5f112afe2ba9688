"""Speaking-rate control: the WSOLA time stretch in front of the resampler
(mp_hip_codec_decode_pcm_speed; definition in include/magpie_hip.h, speaking rate).

_stretch64 restates that definition in float64 with numpy alone, over the f32 waveform the same
device decoded. The output's bar, 4 ulp of max|x|: w and w2 are each rounded to f32 once (2^-24
relative each), the product w2 x once and the fma once, each at most half an ulp of a value no
larger than max|x|. The starts are compared where the f64 choice is no near-tie: at every segment
the best score must lead the runner-up by more than 1e-4 sqrt(sum x[r + i]^2), far above what a
512-term f32 sum can move a score and far below the gaps of this waveform. SEED holds that at all
four speeds, by 40 bars and more (found with the oracle's codec on the CPU). Most seeds do not: at
50 % the last segment's template x[p_22 + 512 ..] lies wholly in the zero padding behind the input
whenever segment 22 chose d >= 0, and every candidate then scores 0.
"""
import numpy as np
import pytest

from test_codec_pcm_gpu import _resample64

pytestmark = pytest.mark.gpu
F32, S16 = 0, 1
H, D, SEED, FRAMES = 512, 256, 138, 6


def _stretch64(x, speed_pct):
    """(starts p_m, y [Ls], the least lead of a best score over its runner-up in units of the bar)"""
    Lin = len(x)
    Ls = -(-Lin * 100 // speed_pct)
    M = -(-Ls // H)
    PAD = D + 2 * H  # zeros in front (c >= 0 is checked besides) and behind: x[j] = 0 outside [0, Lin)
    xp = np.concatenate([np.zeros(PAD), x.astype(np.float64), np.zeros(4 * PAD)])
    i = np.arange(H)
    w = np.sin(np.pi * (i + 0.5) / (2 * H)) ** 2
    p, y, lead = [0], [xp[PAD:PAD + H]], np.inf
    for m in range(1, M):
        r, a = p[-1] + H, m * H * speed_pct // 100
        tmpl = xp[PAD + r:PAD + r + H]
        c = a + np.arange(-D, D + 1)
        win = np.lib.stride_tricks.sliding_window_view(xp[PAD + c[0]:PAD + c[-1] + H], H)
        score = (win @ tmpl) / np.sqrt((win * win).sum(1) + np.float64(np.float32(1e-9)))
        score[c < 0] = -np.inf
        k = int(np.argmax(score))  # the first maximum
        gap, bar = score[k] - np.delete(score, k).max(), 1e-4 * np.sqrt((tmpl * tmpl).sum())
        lead = min(lead, gap / bar if bar > 0 else 0.0)
        p.append(int(c[k]))
        y.append(w * xp[PAD + p[-1]:PAD + p[-1] + H] + (1 - w) * tmpl)
    return np.array(p, np.int32), np.concatenate(y)[:Ls], lead


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
    return np.random.default_rng(SEED).integers(0, 2016, (8, FRAMES)).astype(np.int32)


@pytest.fixture(scope="module")
def x(codec, codes):
    return codec.decode(codes)


@pytest.fixture(scope="module")
def ref(x):
    return {s: _stretch64(x, s) for s in (50, 80, 125, 200)}


@pytest.mark.parametrize("speed_pct", [50, 80, 125, 200])
def test_against_f64(ma, codec, codes, x, ref, speed_pct):
    p64, y64, lead = ref[speed_pct]
    print(f"speed {speed_pct} %: {len(p64)} segments, least lead {lead:.3g} bars")
    assert lead > 1.0  # on the reference alone: every segment's choice is clear
    y, p = codec.decode_pcm(codes, 22050, F32, speed_pct=speed_pct, return_starts=True)
    assert len(y) == len(y64) == ma.tsm_samples(FRAMES, speed_pct, 22050)
    assert np.array_equal(p, p64)
    err, bar = float(np.abs(y - y64).max()), 4 * float(np.spacing(np.abs(x).max()))
    print(f"speed {speed_pct} %: max abs err vs f64 {err:.3g}, bar {bar:.3g} (max |x| {np.abs(x).max():.3f})")
    assert err <= bar


@pytest.mark.parametrize("fmt", [F32, S16])
def test_speed_100_is_decode_pcm(codec, codes, fmt):
    y, p = codec.decode_pcm(codes, 16000, fmt, speed_pct=100, return_starts=True)  # the speed entry point
    assert y.tobytes() == codec.decode_pcm(codes, 16000, fmt).tobytes() and len(p) == 0


def test_stretch_then_resample(ma, codec, codes, ref):
    y64 = _resample64(ref[125][1], 16000)
    s = codec.decode_pcm(codes, 16000, S16, speed_pct=125)
    assert s.dtype == np.int16 and len(s) == len(y64) == ma.tsm_samples(FRAMES, 125, 16000)
    assert np.abs(s - np.trunc(np.clip(y64, -1, 1) * 32767)).max() <= 1


def test_refusals(ma, codec, codes):
    good = codec.decode_pcm(codes, 16000, S16)
    n = ma.tsm_samples(FRAMES, 125, 16000)
    for kw, err in [(dict(speed_pct=49), "MP_ERR_ARG"), (dict(speed_pct=201), "MP_ERR_ARG"),
                    (dict(speed_pct=125, cap=n - 1), "MP_ERR_ARG.*" + str(n))]:
        with pytest.raises(ma.MagpieError, match=err):
            codec.decode_pcm(codes, 16000, S16, **kw)
        assert np.array_equal(codec.decode_pcm(codes, 16000, S16), good)
    assert ma.tsm_samples(FRAMES, 49, 16000) < 0 and ma.tsm_samples(FRAMES, 201, 16000) < 0
