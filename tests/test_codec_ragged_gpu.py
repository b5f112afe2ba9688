"""Ragged stream decode (mp_hip_codec_stream_decode_ragged, CodecStream.decode_ragged).

One call carries one chunk per lane, every lane's of its own length; each lane's chunks,
concatenated, are still bit for bit the one-shot Codec.decode of its frames, whatever the
other lanes of the same call do. A 1-frame lane beside a 32-frame lane ends, on every stage,
in a time tile that is not the launch's last one (stage 0: 8 rows of 256; the post conv:
1 024 samples of 32 768), and a 1-frame chunk is shorter than every tail, so it rolls them.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu_codec(codec_model):
    import magpie_amd as ma
    if ma.device_count() < 1:
        pytest.fail("no HIP device visible")
    c = ma.Codec(codec_model)
    yield c
    c.close()


def _codes(seed, F):
    return np.random.default_rng(seed).integers(0, 2016, (8, F)).astype(np.int32)


class Lanes:
    """Per-lane code sequences fed chunk by chunk; what came back, per lane."""

    def __init__(self, stream, codes):
        self.s, self.codes = stream, codes
        self.at = {b: 0 for b in codes}
        self.got = {b: [] for b in codes}

    def _padded(self, lanes, sizes, garbage):
        F = max(sizes)
        # rows behind a lane's own frames are "ignored": fill them with valid but unrelated codes
        arr = (np.random.default_rng(garbage).integers(0, 2016, (len(lanes), 8, F)).astype(np.int32))
        for q, (b, n) in enumerate(zip(lanes, sizes)):
            arr[q, :, :n] = self.codes[b][:, self.at[b]:self.at[b] + n]
        return arr

    def ragged(self, lanes, sizes, garbage=99):
        out = self.s.decode_ragged(self._padded(lanes, sizes, garbage), sizes, lanes=lanes)
        for q, (b, n) in enumerate(zip(lanes, sizes)):
            assert out[q].shape == (n * 1024,)
            self.got[b].append(out[q])
            self.at[b] += n

    def uniform(self, lanes, n):
        out = self.s.decode(self._padded(lanes, [n] * len(lanes), 0), lanes=lanes)
        for q, b in enumerate(lanes):
            self.got[b].append(out[q])
            self.at[b] += n

    def check(self, codec, lanes=None):
        for b in (self.codes if lanes is None else lanes):
            assert self.at[b] == self.codes[b].shape[1], f"lane {b}: test fed {self.at[b]} frames"
            np.testing.assert_array_equal(np.concatenate(self.got[b]), codec.decode(self.codes[b]), err_msg=f"lane {b}")


CALLS = [(1, 32, 3), (32, 1, 5), (1, 1, 1), (2, 4, 32)]


def test_three_lanes_four_ragged_calls(gpu_codec):
    totals = [sum(c[b] for c in CALLS) for b in range(3)]
    assert min(totals) >= 34  # beyond the 26 frames a frame's influence reaches
    s = gpu_codec.stream(lanes=3)
    L = Lanes(s, {b: _codes(100 + b, totals[b]) for b in range(3)})
    for k, sizes in enumerate(CALLS):
        L.ragged([0, 1, 2], list(sizes), garbage=200 + k)
    s.close()
    L.check(gpu_codec)


def test_equal_lengths_give_the_uniform_call(gpu_codec):
    codes = np.stack([_codes(110 + b, 9) for b in range(3)])
    s1, s2 = gpu_codec.stream(lanes=3), gpu_codec.stream(lanes=3)
    for a, n in ((0, 5), (5, 1), (6, 3)):
        uni = s1.decode(codes[:, :, a:a + n])
        rag = s2.decode_ragged(codes[:, :, a:a + n], [n] * 3)
        for q in range(3):
            np.testing.assert_array_equal(rag[q], uni[q])
    s1.close()
    s2.close()


def test_ragged_and_uniform_interleaved_with_reset_and_lane_order(gpu_codec):
    s = gpu_codec.stream(lanes=3)
    L = Lanes(s, {0: _codes(120, 2 + 4 + 3 + 7 + 1), 1: _codes(121, 5 + 4), 2: _codes(122, 1 + 4 + 6 + 2 + 3)})
    L.ragged([2, 0, 1], [1, 2, 5])        # lanes in non-ascending order
    L.uniform([1, 2, 0], 4)
    L.check(gpu_codec, lanes=[1])          # lane 1's first utterance is complete: 9 frames
    s.reset(1)
    L.codes[1], L.at[1], L.got[1] = _codes(123, 3 + 1 + 2), 0, []
    L.ragged([1, 0, 2], [3, 3, 6])
    L.ragged([0, 2], [7, 2])
    L.uniform([2], 3)
    L.ragged([0, 1], [1, 1])
    L.uniform([1], 2)
    s.close()
    L.check(gpu_codec)


def test_refused_calls_advance_nothing(gpu_codec):
    import magpie_amd as ma
    s = gpu_codec.stream(lanes=2)
    L = Lanes(s, {0: _codes(130, 3 + 4), 1: _codes(131, 1 + 2)})
    L.ragged([0, 1], [3, 1])
    bad = np.random.default_rng(5).integers(0, 2016, (2, 8, 4)).astype(np.int32)
    with pytest.raises(ma.MagpieError, match="MP_ERR_ARG"):
        s.decode_ragged(bad, [4, 0], lanes=[0, 1])
    with pytest.raises(ma.MagpieError, match="MP_ERR_ARG"):
        s.decode_ragged(bad, [5, 2], lanes=[0, 1])
    with pytest.raises(ma.MagpieError, match="MP_ERR_ARG.*twice"):
        s.decode_ragged(bad, [4, 2], lanes=[1, 1])
    with pytest.raises(ma.MagpieError, match="MP_ERR_ARG.*out of range"):
        s.decode_ragged(bad, [4, 2], lanes=[0, 2])
    L.ragged([0, 1], [4, 2])
    s.close()
    L.check(gpu_codec)
