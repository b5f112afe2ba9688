"""The text-length edges of the preamble and the decode step's cross-attention: the case
table shared by test_text_edges_cpu.py (the oracle's preconditions) and
test_text_edges_gpu.py (the kernels against the oracle).

The text length T decides the path in most of the preamble and in the decode's XA:
  1, 2, 3, 4, 5, 7, 9     whole empty key splits of the reassociated XA (XA_SPLITS = 4 chunks of
                          ceil(T / 4) keys: T < 4, T = 5, T = 9) and, to T = 12, waves with no key;
                          M = 1 is a single partial GEMM tile
  15, 16, 17              one full round of the reassociated XA's 4 waves x 4 keys, +- 1
  63, 64, 65              a 64 x 64 GEMM row tile and a 64-key round of the direct text attention
                          and of the encoder's causal attention, +- 1
  127, 128, 129           two tiles / rounds, +- 1
  160, 161                AUTO's switch from the reassociated to the direct form (MP_XA_DIRECT_T)
  255, 256, 257           four tiles, +- 1: the direct form's value rows past the 4 x 16 prefetched
  1023, 1024              the limit (TMAX_LIMIT: the 4 KB LDS score buffers full); from M = 321 the
                          FFN-up GEMM and from M = 449 the QKV GEMM run their splits inside each
                          workgroup (PRE_INWG_TILES)
Every case: the 2-layer small model, 8 greedy decode steps with EOS ignored, traced.
"""
import numpy as np

# the bars are the existing ones, from where they are derived
from parity import TIE_EPS
from test_decode_gpu import (BF16_HIDDEN_REL, BF16_HIDDEN_TOL, BF16_TIE_EPS, HIDDEN_TOL, Q8_BARS,  # noqa: F401
                             Q8_TIE_EPS)

ENC_TOL = 2e-5  # test_decode_gpu.py::test_encode_text_alone_leaves_batch_untouched

EDGES = (1, 2, 3, 4, 5, 7, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129, 160, 161, 255, 256, 257, 1023, 1024)
STEPS = 8
# the oracle's smallest top-1/top-2 margin over a case's 64 decisions must be this wide: the GPU
# tests then demand identical codes over all 8 frames, with no near-tie exit
MIN_MARGIN = 2 * TIE_EPS
# the last token replaced must move the hidden state after the BOS step by this much, so a kernel
# that drops or clamps away the last key misses the hidden bar
SENSITIVE_T = (2, 5, 17, 65, 161, 257, 1024)
MIN_SENSITIVITY = 50 * HIDDEN_TOL
# the oracle accumulating in f32 instead of f64: what the 2e-5 bars rest on
SPREAD_T = (1, 65, 257, 1024)
MAX_SPREAD = 1e-5

# The ragged XA K/V layer group: G = min(L, floor(4 max(T, 110) / T)) layers share one LN launch
# and one batched GEMM (run_preamble). 5 decoder layers: T = 88 gives G = 5 (one group), T = 89
# G = 4 (4 + 1, a ragged last group), T = 111 G = 4 past the 110-row context.
GROUP_MODEL = dict(dec_layers=5, enc_layers=2)
GROUP_MODEL_FILE = "magpie_l5e2_k32.gguf"
GROUP_T = (88, 89, 111)
GROUP_BATCH = (89, 30)

# Other weight families, short texts, teacher forced: (weights, model fixture, oracle weight
# mode, T, hidden bar). A case is listed only where the last token moves the BOS-step hidden state
# of the matching oracle mode by >= 3 x its bar (test_text_edges_cpu.py), so the test can fail.
# Measured (x the bar): bf16 84, 33, 10, 3.5 and f16 84, 33, 10, 3.7 at T = 1, 2, 3, 5; Q8_0 252,
# 99, 11 at T = 1, 2, 5. Q8_0 at T = 65 moves by 2.88e-2, 2.9 x its 1e-2 bar: not listed (the long
# edges of the attention body the Q8_0 kernels share are carried by the f32 cases).
FAMILY_MIN_SENSITIVITY = 3
FAMILY_CASES = (
    [("bf16", "small_model", 1, T, BF16_HIDDEN_TOL) for T in (1, 2, 3, 5)]
    + [("f16", "f16_model", 3, T, BF16_HIDDEN_TOL) for T in (1, 2, 3, 5)]
    + [("q8", "q8_model", 2, T, Q8_BARS["small"][0]) for T in (1, 2, 5)]
)


def tokens(ma, T):
    return ma.synthetic_tokens(T, seed=9000 + T)


def speaker(T):
    return T % 5


def last_token_replaced(tok):
    t = np.array(tok, np.int32)
    t[-1] = (t[-1] + 17) % 90 + 1
    return t


def group_model(ma):
    """the 5-layer model, written into $MAGPIE_CACHE as conftest.py's models are"""
    import os
    cache = os.environ.get("MAGPIE_CACHE", "/tmp/magpie_amd_cache")
    os.makedirs(cache, exist_ok=True)
    return ma.synth_gguf(os.path.join(cache, GROUP_MODEL_FILE), lt_head_scale=ma.DECISIVE, **GROUP_MODEL)


class OracleRuns:
    """One oracle.Model and its results, each computed once: run(T) is the case of length T
    (STEPS greedy frames, traced), encode(T) its encoder output."""

    def __init__(self, ma, oracle, path, weight_mode=0):
        self.ma = ma
        self.om = oracle.Model(path)
        if weight_mode:
            self.om.set_weight_mode(weight_mode)
        self._runs, self._enc = {}, {}

    def run(self, T):
        if T not in self._runs:
            o = self.om.synthesize(tokens(self.ma, T), speaker=speaker(T), max_steps=STEPS, ignore_eos=True, trace=True)
            assert o["n_frames"] == STEPS and np.isfinite(o["hidden"]).all(), f"T = {T}: the oracle's own run"
            for v in o.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
            self._runs[T] = o
        return self._runs[T]

    def encode(self, T):
        if T not in self._enc:
            e = self.om.encode(tokens(self.ma, T))
            e.setflags(write=False)
            self._enc[T] = e
        return self._enc[T]

    def bos_hidden(self, tok, spk):
        """the hidden state after the BOS step alone (one frame) of any text"""
        return self.om.synthesize(tok, speaker=spk, max_steps=1, ignore_eos=True, trace=True)["hidden"][0]

    def close(self):
        self.om.close()
