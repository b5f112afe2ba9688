"""Streaming synthesis with the continuous codec (MP_STREAM_CODEC_CONTINUOUS).

mp_hip_decode_stream decodes utterance b's chunks on lane b of a stateful codec stream, so
the audio an utterance's callbacks receive is, concatenated and bit for bit, one
Codec.decode of the utterance's frames; codes, chunk sizes, callback order, the EOS frame
and the stop semantics are the stateless run's. The CLI's --continuous-codec does the same
for its 32-frame chunk loop and, with --stream, per sentence.
"""
import os
import struct
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TEXT = "Hello, world! The first voice, 21st of May."


@pytest.fixture(scope="module")
def ma():
    import magpie_amd
    if magpie_amd.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    return magpie_amd


@pytest.fixture(scope="module")
def codec(ma, codec_model):
    c = ma.Codec(codec_model)
    yield c
    c.close()


def _collect(B):
    chunks = {b: [] for b in range(B)}

    def on_audio(utt, samples):
        chunks[utt].append(samples)
        return True
    return chunks, on_audio


def test_continuous_stream_equals_one_shot_per_utterance(ma, small_model, codec):
    toks = [ma.synthetic_tokens(8 + 3 * i, seed=700 + i) for i in range(3)]
    kw = dict(speakers=[0, 1, 2], max_dec_steps=10, frames_per_chunk=4, ignore_eos=True)
    dev = ma.Device(small_model)
    ch_s, cb_s = _collect(3)
    codes_s, total_s, _ = dev.synthesize_stream(codec, toks, cb_s, **kw)
    ch_c, cb_c = _collect(3)
    codes_c, total_c, _ = dev.synthesize_stream(codec, toks, cb_c, continuous=True, **kw)
    assert total_c == total_s == 3 * 10 * 1024
    for b in range(3):
        assert np.array_equal(codes_c[b], codes_s[b])
        assert [len(c) for c in ch_c[b]] == [4096, 4096, 2048]
        np.testing.assert_array_equal(np.concatenate(ch_c[b]), codec.decode(codes_c[b].T), err_msg=f"utterance {b}")
        # the first chunk has no past in either mode; the later stateless chunks are not the one-shot's
        assert np.array_equal(ch_c[b][0], ch_s[b][0]) and not np.array_equal(ch_c[b][1], ch_s[b][1])

    # a callback that stops utterance 0 after its first chunk leaves the others exact
    got = {b: [] for b in range(3)}

    def stop0(utt, audio):
        got[utt].append(audio)
        return utt != 0

    codes_x, total_x, _ = dev.synthesize_stream(codec, toks, stop0, continuous=True, **kw)
    assert len(got[0]) == 1 and len(codes_x[0]) == 4 and total_x == (4 + 10 + 10) * 1024
    np.testing.assert_array_equal(got[0][0], ch_c[0][0])
    for b in (1, 2):
        np.testing.assert_array_equal(np.concatenate(got[b]), codec.decode(codes_x[b].T), err_msg=f"utterance {b}")

    # and the default is the stateless stream again
    ch_d, cb_d = _collect(3)
    dev.synthesize_stream(codec, toks, cb_d, **kw)
    dev.close()
    for b in range(3):
        assert all(np.array_equal(x, y) for x, y in zip(ch_d[b], ch_s[b]))


def test_continuous_stream_with_eos_frame(ma, eos_model, codec):
    toks = [ma.synthetic_tokens(16, seed=7), ma.synthetic_tokens(9, seed=8)]
    dev = ma.Device(eos_model)
    ch_s, cb_s = _collect(2)
    codes_s, _, _ = dev.synthesize_stream(codec, toks, cb_s, max_dec_steps=64, frames_per_chunk=4)
    ch_c, cb_c = _collect(2)
    codes_c, total, _ = dev.synthesize_stream(codec, toks, cb_c, max_dec_steps=64, frames_per_chunk=4, continuous=True)
    dev.close()
    assert total == 2 * 5 * 1024
    for b in range(2):
        assert np.array_equal(codes_c[b], codes_s[b]) and len(codes_c[b]) == 5
        assert [len(c) for c in ch_c[b]] == [4 * 1024, 1 * 1024]  # 4 frames + the EOS frame
        np.testing.assert_array_equal(np.concatenate(ch_c[b]), codec.decode(codes_c[b].T), err_msg=f"utterance {b}")


# ---- CLI (the WAV rules of tests/test_cli_gpu.py)
def _read_wav(path):
    raw = open(path, "rb").read()
    assert raw[:4] == b"RIFF" and raw[8:16] == b"WAVEfmt " and raw[36:40] == b"data"
    (n,) = struct.unpack("<I", raw[40:44])
    assert len(raw) == 44 + n
    return np.frombuffer(raw[44:], np.int16)


def _pcm(audio):
    return (np.clip(audio, -1.0, 1.0) * np.float32(32767.0)).astype(np.int16)  # truncation toward zero


def _cli(ma, *args):
    exe = os.path.join(os.path.dirname(ma.LIB_PATH), "..", "bin", "magpie-tts")
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return r


def test_cli_continuous_codec(ma, small_model, codec_model, codec, tmp_path):
    out = str(tmp_path / "a.wav")
    _cli(ma, "-m", small_model, "-c", codec_model, "-t", TEXT, "-o", out, "--temp", "0", "--continuous-codec", "-q")
    wav = _read_wav(out)
    tk = ma.Tokenizer(small_model)
    dev = ma.Device(small_model)
    codes = dev.synthesize([tk(TEXT)], max_dec_steps=500).codes[0]
    assert len(wav) == len(codes) * 1024
    assert np.array_equal(wav, _pcm(codec.decode(codes.T)))  # one decode of all the frames, not 32-frame chunks

    out = str(tmp_path / "s.wav")
    _cli(ma, "-m", small_model, "-c", codec_model, "-t", TEXT, "-o", out, "--stream", "--continuous-codec", "--temp", "0.7",
         "-q")
    wav = _read_wav(out)
    parts = []
    for i, s in enumerate(ma.split_sentences(TEXT)):
        codes_s, _, _ = dev.synthesize_stream(codec, [tk(s)], lambda u, a: True, speakers=[0], max_dec_steps=500,
                                              temperature=0.7, top_k=80, seed=0, frames_per_chunk=4, stream_base=i)
        parts.append(codec.decode(codes_s[0].T))  # each sentence's one-shot decode
    dev.close()
    assert np.array_equal(wav, _pcm(np.concatenate(parts)))
