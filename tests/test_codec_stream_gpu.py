"""Stateful streaming decode of the nano-codec (mp_hip_codec_stream_*, Codec.stream).

Consecutive chunks of one utterance decoded on one stream lane give, bit for bit, the
samples one Codec.decode of all the utterance's frames gives ("one-shot", the default
path: fused residual blocks). A lane carries each causal conv's last (ks - 1) * dilation
operand rows, each transposed conv's last input step and the pre-conv's last 6 frames of
codes; the deepest tail is 50 rows, a frame is 8 steps on the first stage, so single-frame
chunks roll every tail (chunk shorter than the tail) before they replace it.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WAVE_TOL = 2e-3  # tests/test_codec_gpu.py


@pytest.fixture(scope="module")
def gpu_codec(codec_model):
    import magpie_amd as ma
    if ma.device_count() < 1:
        pytest.fail("no HIP device visible")
    c = ma.Codec(codec_model)
    yield c
    c.close()


def _codes(seed, F, n=None):
    shape = (8, F) if n is None else (n, 8, F)
    return np.random.default_rng(seed).integers(0, 2016, shape).astype(np.int32)


def _stream(s, codes, sizes, lane=0):
    """codes [8][F] through lane `lane` in chunks of `sizes`, concatenated."""
    out, f = [], 0
    for n in sizes:
        out.append(s.decode(codes[None, :, f:f + n], lanes=[lane])[0])
        f += n
    assert f == codes.shape[1]
    return np.concatenate(out)


def test_single_frame_chunks_equal_one_shot(gpu_codec, oracle, codec_model):
    F = 13  # 13 x 8 steps > the deepest tail (50 rows): the roll with T < pad on every stage
    codes = _codes(21, F)
    one = gpu_codec.decode(codes)
    s = gpu_codec.stream()
    got = _stream(s, codes, [1] * F)
    s.close()
    np.testing.assert_array_equal(got, one)
    cpu = oracle.Codec(codec_model)
    o = cpu.decode(codes, f16_operands=True)
    cpu.close()
    e_stream, e_one = np.abs(got - o).max(), np.abs(one - o).max()
    print(f"max abs error against the oracle's one-shot: stream {e_stream:.2e}, one-shot {e_one:.2e}")
    assert e_stream < WAVE_TOL and e_one < WAVE_TOL


def test_mixed_chunk_sizes_equal_one_shot(gpu_codec):
    sizes = [3, 1, 32, 4, 2]  # 42 frames: beyond the 26 frames a frame's influence reaches
    codes = _codes(22, sum(sizes))
    s = gpu_codec.stream()
    got = _stream(s, codes, sizes)
    s.close()
    np.testing.assert_array_equal(got, gpu_codec.decode(codes))


@pytest.mark.parametrize("switches", [{}, {"MAGPIE_CODEC_UNFUSED": "1", "MAGPIE_CODEC_RL": "0"}], ids=["default", "unfused"])
def test_first_chunk_equals_stateless_decode(gpu_codec, monkeypatch, switches):
    """The two arms of the codec's one launch sequence against each other: a first chunk on a
    fresh lane (zero state: the causal padding) is Codec.decode of the same codes, bit for bit,
    with the stateless arm on its fused residual blocks (the default switches) and on the
    two-launch blocks the stream arm always runs. F = 1 keeps every stage below the wide-tile
    thresholds (conv_mfma_kernel everywhere, T shorter than the tails); F = 32 reaches
    conv2_kernel on every stage. Then one ragged call of 3 lanes after a reset."""
    for k, v in switches.items():
        monkeypatch.setenv(k, v)
    s = gpu_codec.stream(lanes=3)
    for lane, F in enumerate((1, 4, 32)):  # each on a lane nothing has used
        codes = _codes(80 + F, F)
        np.testing.assert_array_equal(s.decode(codes[None], lanes=[lane])[0], gpu_codec.decode(codes), err_msg=f"F = {F}")
    lens = (4, 1, 3)
    rows = [_codes(90 + q, n) for q, n in enumerate(lens)]
    s.reset()
    got = s.decode_ragged(rows, lens)
    s.close()
    for q, row in enumerate(rows):
        np.testing.assert_array_equal(got[q], gpu_codec.decode(row), err_msg=f"lane {q}: {lens[q]} of 4 frames")


def test_lanes_interleaved_reordered_and_reset(gpu_codec):
    sizes = {0: [2, 5, 1, 3], 1: [4, 1, 2], 2: [1, 5, 3, 2]}
    codes = {b: _codes(30 + b, sum(sizes[b])) for b in sizes}
    new1 = _codes(40, 6)
    s = gpu_codec.stream(lanes=3)
    got = {b: [] for b in sizes}
    at = {b: 0 for b in sizes}

    def step(b, k):
        n = sizes[b][k]
        got[b].append(s.decode(codes[b][None, :, at[b]:at[b] + n], lanes=[b])[0])
        at[b] += n

    # call by call: lane 0, 1, 2 in turn ...
    for b in (0, 1, 2):
        step(b, 0)
    # ... one call carrying lanes [2, 0], in that order (both chunks 5 frames)
    pair = s.decode(np.stack([codes[2][:, 1:6], codes[0][:, 2:7]]), lanes=[2, 0])
    got[2].append(pair[0]); at[2] += 5
    got[0].append(pair[1]); at[0] += 5
    step(1, 1)
    # lane 1 starts over mid-way with new codes; lanes 0 and 2 go on
    s.reset(1)
    fresh = [s.decode(new1[None, :, 0:2], lanes=[1])[0]]
    step(0, 2)
    step(2, 2)
    fresh.append(s.decode(new1[None, :, 2:6], lanes=[1])[0])
    step(0, 3)
    step(2, 3)
    s.close()
    for b in (0, 2):
        np.testing.assert_array_equal(np.concatenate(got[b]), gpu_codec.decode(codes[b]), err_msg=f"lane {b}")
    # lane 1 before the reset: the one-shot of the 5 frames it was given
    np.testing.assert_array_equal(np.concatenate(got[1]), gpu_codec.decode(codes[1][:, :5]))
    np.testing.assert_array_equal(np.concatenate(fresh), gpu_codec.decode(new1))


def test_sixteen_lanes_two_32_frame_chunks(gpu_codec):
    codes = _codes(50, 64, n=16)
    s = gpu_codec.stream(lanes=16)
    a = s.decode(codes[:, :, :32])
    b = s.decode(codes[:, :, 32:])
    s.close()
    for lane in (0, 7, 15):
        np.testing.assert_array_equal(np.concatenate([a[lane], b[lane]]), gpu_codec.decode(codes[lane]), err_msg=f"lane {lane}")


def test_stream_use_leaves_stateless_decode_unchanged(gpu_codec):
    fixed = _codes(60, 4, n=3)
    before = gpu_codec.decode_chunks(fixed)
    s = gpu_codec.stream(lanes=2)
    s.decode(_codes(61, 5, n=2))
    s.decode(_codes(62, 1, n=2))
    after_open = gpu_codec.decode_chunks(fixed)
    s.close()
    np.testing.assert_array_equal(before, after_open)
    np.testing.assert_array_equal(before, gpu_codec.decode_chunks(fixed))


def test_refused_calls_advance_nothing(gpu_codec):
    import magpie_amd as ma
    codes = _codes(70, 9)
    s = gpu_codec.stream(lanes=2)
    got = [s.decode(codes[None, :, 0:4], lanes=[0])[0]]
    two = np.stack([codes[:, 4:6], codes[:, 4:6]])
    with pytest.raises(ma.MagpieError, match="MP_ERR_ARG.*twice"):
        s.decode(two, lanes=[0, 0])
    with pytest.raises(ma.MagpieError, match="MP_ERR_ARG.*out of range"):
        s.decode(two, lanes=[0, 2])
    with pytest.raises(ma.MagpieError, match="MP_ERR_ARG.*out of range"):
        s.decode(two[:1], lanes=[-1])
    with pytest.raises(ma.MagpieError, match="MP_ERR_ARG"):
        s.decode(np.zeros((1, 8, 0), np.int32), lanes=[0])
    got.append(s.decode(codes[None, :, 4:9], lanes=[0])[0])
    s.close()
    np.testing.assert_array_equal(np.concatenate(got), gpu_codec.decode(codes))
