"""magpie-tts --cfg-scale (classifier-free guidance through the drop-in API's
magpie_context::cfg_scale): scale 1 is the plain run, sample for sample; 2.5 is not."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

TEXT = "Hello, world! The first voice, 21st of May."


@pytest.fixture(scope="module")
def ma():
    import magpie_amd
    if magpie_amd.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    return magpie_amd


def _cli(ma, *args):
    exe = os.path.join(os.path.dirname(ma.LIB_PATH), "..", "bin", "magpie-tts")
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return r


def test_cli_cfg_scale(ma, small_model, codec_model, tmp_path):
    base = ["-m", small_model, "-c", codec_model, "-t", TEXT, "--temp", "0", "-q"]
    wavs = {}
    for name, extra in (("plain", []), ("one", ["--cfg-scale", "1"]), ("guided", ["--cfg-scale", "2.5"])):
        out = str(tmp_path / f"{name}.wav")
        _cli(ma, *base, "-o", out, *extra)
        wavs[name] = open(out, "rb").read()
        assert len(wavs[name]) > 44 + 2 * 1024
    assert wavs["one"] == wavs["plain"]
    assert wavs["guided"] != wavs["plain"]
