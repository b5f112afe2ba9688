"""What the stateful codec stream rests on, checked without a GPU.

The nano-codec decoder is strictly causal (every conv is left-padded, the transposed convs
reach one input step back), so the decode of a prefix is the prefix of the decode, exactly;
and a stateless decode of 4-frame chunks, each as if nothing preceded it, is a different
signal from the one-shot decode. Hence a chunked decode that carries each conv's left
context is the one-shot decode, and one that does not is audibly not.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WAVE_TOL = 2e-3  # tests/test_codec_gpu.py

NEW_ENTRY_POINTS = ["mp_hip_codec_stream_create", "mp_hip_codec_stream_decode", "mp_hip_codec_stream_reset",
                    "mp_hip_codec_stream_free", "mp_hip_set_stream_codec_mode"]


def test_oracle_codec_is_causal_and_stateless_chunks_are_not_the_signal(oracle, codec_model):
    F = 30
    codes = np.random.default_rng(5).integers(0, 2016, (8, F)).astype(np.int32)
    cpu = oracle.Codec(codec_model)
    kw = dict(f16_operands=True, resinit=True)
    one = cpu.decode(codes, **kw)
    for k in (1, 13):
        np.testing.assert_array_equal(cpu.decode(codes[:, :k], **kw), one[:k * 1024], err_msg=f"prefix {k}")
    chunked = np.concatenate([cpu.decode(codes[:, f:f + 4], **kw) for f in range(0, F, 4)])
    cpu.close()
    d = chunked - one
    rms, sig = float(np.sqrt(np.mean(d * d))), float(np.sqrt(np.mean(one * one)))
    print(f"stateless 4-frame chunks against one-shot, F = {F}: rms difference {rms:.3f} (signal rms {sig:.3f}), "
          f"max abs {np.abs(d).max():.2f}")  # 0.16 rms at F = 40
    assert rms > WAVE_TOL


def test_header_declares_the_stream_entry_points(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "no C compiler"
    src = tmp_path / "abi.c"
    uses = "\n".join(f"    (void)&{name};" for name in NEW_ENTRY_POINTS)
    src.write_text('#include "magpie_hip.h"\n'
                   "int main(void) {\n"
                   "    mp_codec_stream *s = 0;\n"
                   "    int modes[2] = {MP_STREAM_CODEC_STATELESS, MP_STREAM_CODEC_CONTINUOUS};\n"
                   f"{uses}\n"
                   "    return s != 0 || modes[0] == modes[1];\n"
                   "}\n")
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(REPO, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
