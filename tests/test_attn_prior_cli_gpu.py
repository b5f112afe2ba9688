"""magpie-tts --attn-prior-* (the attention prior through magpie_context): epsilon 1 is the plain
run, sample for sample; 0.1 with no lookahead is not; a bad epsilon fails."""
import pytest

from test_cfg_cli_gpu import TEXT, _cli, ma  # noqa: F401

pytestmark = pytest.mark.gpu


def test_cli_attn_prior(ma, small_model, codec_model, tmp_path):  # noqa: F811
    base = ["-m", small_model, "-c", codec_model, "-t", TEXT, "--temp", "0", "-q"]
    wavs = {}
    for name, extra in (("plain", []), ("one", ["--attn-prior-eps", "1"]),
                        ("prior", ["--attn-prior-eps", "0.1", "--attn-prior-lookahead", "0", "--attn-prior-start", "1"])):
        out = str(tmp_path / f"{name}.wav")
        _cli(ma, *base, "-o", out, *extra)
        wavs[name] = open(out, "rb").read()
    assert wavs["one"] == wavs["plain"] and wavs["prior"] != wavs["plain"]
    with pytest.raises(AssertionError):
        _cli(ma, *base, "-o", str(tmp_path / "bad.wav"), "--attn-prior-eps", "2")
