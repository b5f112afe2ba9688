"""The f32 family's decode kernels take their entry path's scalars as leading kernel
arguments (mp_decode.hip, gemv_kernel's note; tests/test_kernarg_preload_cpu.py reads
the built code). A mis-ordered or mis-typed leading argument shows as a wrong decode
at the shapes run here: the 2-layer model, a T = 24 text, 9 greedy frames at batch 1
(lt_front, lt_ffn2, the LT head's merge prologue) and at batch 3 (4 padded slots: the
other LT launch list, lt_kvo / lt_ffn2<4> / lt_merge), each
 - replayed from the captured graph,
 - launched eagerly (MAGPIE_EAGER=1, in a fresh child process),
 - with the direct cross-attention form forced (oproj, xq and xa_dir instead of oproj_xa).
Every run's codes equal the oracle's and its hidden states are within the f32 bar."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HIDDEN_TOL = 2e-5  # f32 vs the acc64 oracle (tests/test_decode_gpu.py)
STEPS, T, SEED = 9, 24, 1000
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ma():
    import magpie_amd
    if magpie_amd.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    return magpie_amd


def _tokens(ma, B):
    return [ma.synthetic_tokens(T, seed=SEED + b) for b in range(B)]


@pytest.fixture(scope="module")
def reference(ma, oracle, small_model):
    """the oracle's (codes, hidden) of the three utterances, each run alone; read-only"""
    om = oracle.Model(small_model)
    out = []
    for b, tok in enumerate(_tokens(ma, 3)):
        o = om.synthesize(tok, speaker=b % 5, max_steps=STEPS, ignore_eos=True, trace=True)
        codes, hidden = np.asarray(o["codes"]), np.asarray(o["hidden"])
        assert codes.shape == (STEPS, 8)
        codes.setflags(write=False)
        hidden.setflags(write=False)
        out.append((codes, hidden))
    om.close()
    return out


def _check(codes, hidden, reference, what):
    for b in range(len(codes)):
        oc, oh = reference[b]
        assert np.array_equal(np.asarray(codes[b]), oc), f"{what}, slot {b}: codes differ from the oracle's"
        err = float(np.abs(np.asarray(hidden[b])[:STEPS + 1] - oh[:STEPS + 1]).max())
        print(f"{what}, slot {b}: hidden max abs err {err:.3g}")
        assert err < HIDDEN_TOL, f"{what}, slot {b}: hidden max abs err {err}"


def _run(ma, path, B, xa="auto"):
    dev = ma.Device(path, weights="f32", xa=xa)
    r = dev.synthesize(_tokens(ma, B), speakers=[b % 5 for b in range(B)], max_dec_steps=STEPS, ignore_eos=True,
                       trace=True)
    dev.close()
    return [r.codes[b] for b in range(B)], [r.hidden[b] for b in range(B)]


@pytest.mark.parametrize("B", [1, 3])
def test_graph_decode_matches_oracle(ma, small_model, reference, B):
    codes, hidden = _run(ma, small_model, B)
    _check(codes, hidden, reference, f"graph B={B}")


@pytest.mark.parametrize("B", [1, 3])
def test_direct_xa_decode_matches_oracle(ma, small_model, reference, B):
    codes, hidden = _run(ma, small_model, B, xa="direct")
    _check(codes, hidden, reference, f"direct XA B={B}")


CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import magpie_amd as ma
path, out, steps, T, seed = sys.argv[2], sys.argv[3], int(sys.argv[4]), int(sys.argv[5]), int(sys.argv[6])
res = {}
for B in (1, 3):
    dev = ma.Device(path, weights="f32")
    toks = [ma.synthetic_tokens(T, seed=seed + b) for b in range(B)]
    r = dev.synthesize(toks, speakers=[b % 5 for b in range(B)], max_dec_steps=steps, ignore_eos=True, trace=True)
    dev.close()
    for b in range(B):
        res[f"codes_{B}_{b}"] = np.asarray(r.codes[b])
        res[f"hidden_{B}_{b}"] = np.asarray(r.hidden[b])
np.savez(out, **res)
"""


def test_eager_decode_matches_oracle(ma, small_model, reference, tmp_path):
    out = str(tmp_path / "eager.npz")
    env = dict(os.environ, MAGPIE_EAGER="1")
    p = subprocess.run([sys.executable, "-c", CHILD, os.path.join(REPO, "magpie-tts.cpp_amd"), small_model, out,
                        str(STEPS), str(T), str(SEED)], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-3000:]
    z = np.load(out)
    for B in (1, 3):
        _check([z[f"codes_{B}_{b}"] for b in range(B)], [z[f"hidden_{B}_{b}"] for b in range(B)], reference,
               f"eager B={B}")
