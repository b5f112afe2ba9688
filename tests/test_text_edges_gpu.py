"""Every text-length edge of the preamble and the decode step's cross-attention against the
oracle (the case table and what each length is the edge of: tests/text_edges.py; the
preconditions that keep these tests from passing vacuously: tests/test_text_edges_cpu.py).

The bars are the existing ones (test_decode_gpu.py): identical codes over all 8 frames (every
case's smallest oracle margin is >= 2 x TIE_EPS, so there is no near-tie exit) and hidden states
and encoder output within 2e-5 of the acc64 oracle, whose own f32-accumulating mode differs from
it by at most 3.4e-6 (hidden) and 7.7e-6 (encoder). One Device per model, weight mode and XA
form and one oracle.Model per model and weight mode serve the whole module; every single run
and every oracle result is computed once and left unchanged.

Measured on an MI355X (max abs err, units of 1e-6; every code identical):
  T         1    2    3    4    5    7    9    15   16   17   63   64   65   127  128  129
  reassoc   1.92 1.91 1.55 1.82 1.67 1.79 1.49 1.25 1.31 1.43 1.19 1.19 1.19 1.31 1.19 0.95
  direct    1.91 1.67 1.43 1.76 1.43 1.55 1.52 1.31 1.19 1.23 1.19 1.19 1.19 1.19 1.31 1.43
  encoder   1.73 1.91 1.79 2.38 2.26 2.71 2.50 2.62 2.38 2.44 3.10 2.92 2.68 2.80 2.98 2.62
  T         160  161  255  256  257  1023 1024
  reassoc   1.22 1.07 1.13 1.01 1.19 1.31 0.95
  direct    1.19 1.19 0.95 1.04 1.07 1.43 0.95
  encoder   2.86 2.74 3.14 2.77 3.10 2.92 3.22
5-layer model (T = 88, 89, 111): 1.19, 1.43, 1.31. bf16 / F16 / Q8_0 short texts: at most 7.2e-3,
1.8e-3 and 2.4e-3 against bars of 3e-2, 3e-2 and 1e-2.

The tests stand in the order a first run should meet them: the refused lengths (nothing is
launched), then the edges in ascending T, then batches, the layer groups, the other weight
families and the slot pool.
"""
import numpy as np
import pytest

import text_edges as te
from parity import compare_codes, compare_forced
from test_decode_gpu import _check_hidden_b16, _check_hidden_q8

pytestmark = pytest.mark.gpu

FORMS = ("reassoc", "direct")


@pytest.fixture(scope="module")
def ma():
    import magpie_amd
    if magpie_amd.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    return magpie_amd


class GpuRuns:
    """The Devices of one model and weight mode (one per XA form, opened on first use) and the
    single runs of the cases, each computed once."""

    def __init__(self, ma, path, weights="f32"):
        self.ma, self.path, self.weights = ma, path, weights
        self._dev, self._single = {}, {}

    def dev(self, xa):
        if xa not in self._dev:
            self._dev[xa] = self.ma.Device(self.path, weights=self.weights, xa=xa)
        return self._dev[xa]

    def synthesize(self, xa, lens):
        return self.dev(xa).synthesize([te.tokens(self.ma, T) for T in lens], speakers=[te.speaker(T) for T in lens],
                                       max_dec_steps=te.STEPS, ignore_eos=True, trace=True)

    def single(self, xa, T):
        if (xa, T) not in self._single:
            r = self.synthesize(xa, [T])
            r.codes[0].setflags(write=False)
            r.hidden.setflags(write=False)
            self._single[(xa, T)] = r
        return self._single[(xa, T)]

    def close(self):
        for d in self._dev.values():
            d.close()


@pytest.fixture(scope="module")
def gpu(ma, small_model):
    g = GpuRuns(ma, small_model)
    yield g
    g.close()


@pytest.fixture(scope="module")
def orc(ma, oracle, small_model):
    r = te.OracleRuns(ma, oracle, small_model)
    yield r
    r.close()


def _against_oracle(codes, hidden, o, what):
    """identical codes over all 8 frames and all 9 hidden rows within the f32 bar"""
    res = compare_codes(codes, o["codes"], o["margins"], min_frames=te.STEPS)
    err = float(np.abs(hidden[:te.STEPS + 1] - o["hidden"][:te.STEPS + 1]).max())
    print(f"{what}: hidden max abs err {err:.3g} vs the oracle")
    assert res["identical"], what
    assert err < te.HIDDEN_TOL, f"{what}: hidden max abs err {err}"
    return err


def _equals_single(rb, b, rs, what):
    assert np.array_equal(rb.codes[b], rs.codes[0]), f"{what}: codes"
    assert np.array_equal(rb.hidden[b], rs.hidden[0]), f"{what}: hidden"


# ---------------------------------------------------------------- refused lengths
def test_refused_lengths_leave_the_device_usable(ma, gpu, orc):
    """One token past TMAX_LIMIT = 1024 and an empty text are refused by the argument checks
    (check_utterances, mp_hip_encode_text: before anything is launched), alone or beside a good
    utterance; after each refusal the same Device runs the T = 5 case and matches the oracle."""
    dev = gpu.dev("auto")
    good, long_ = te.tokens(ma, 5), te.tokens(ma, te.EDGES[-1] + 1)
    assert len(long_) == 1025
    kw = dict(max_dec_steps=te.STEPS, ignore_eos=True, trace=True)
    refused = [
        ("synthesize, 1025 tokens", lambda: dev.synthesize([long_], speakers=[0], **kw), "too many text tokens"),
        ("synthesize, 1025 tokens beside 5", lambda: dev.synthesize([good, long_], speakers=[0, 0], **kw),
         "too many text tokens"),
        ("encode_text, 1025 tokens", lambda: dev.encode_text(long_), "too many text tokens"),
        ("synthesize, empty text", lambda: dev.synthesize([[]], speakers=[0], **kw), None),
        ("synthesize, empty text beside 5", lambda: dev.synthesize([good, []], speakers=[0, 0], **kw), None),
        ("encode_text, empty text", lambda: dev.encode_text(np.zeros(0, np.int32)), None),
    ]
    for what, call, match in refused:
        with pytest.raises(ma.MagpieError, match=match):
            call()
        r = dev.synthesize([good], speakers=[te.speaker(5)], **kw)
        _against_oracle(r.codes[0], r.hidden[0], orc.run(5), f"T = 5 after the refused {what}")


# ---------------------------------------------------------------- every edge, f32
@pytest.mark.parametrize("T,xa", [(T, xa) for T in te.EDGES for xa in FORMS])
def test_f32_edge_matches_oracle(gpu, orc, T, xa):
    """f32, both XA forms forced, every edge: codes and hidden states against the oracle."""
    r = gpu.single(xa, T)
    assert r.n_frames[0] == te.STEPS
    _against_oracle(r.codes[0], r.hidden[0], orc.run(T), f"T = {T}, {xa}")


@pytest.mark.parametrize("T", te.EDGES)
def test_encoder_edge_matches_oracle(ma, gpu, orc, T):
    """The text encoder alone (mp_hip_encode_text: M = T rows, causal attention to nk = T)."""
    enc = gpu.dev("auto").encode_text(te.tokens(ma, T))
    err = float(np.abs(enc - orc.encode(T)).max())
    print(f"T = {T}: encoder max abs err {err:.3g} vs the oracle")
    assert err < te.ENC_TOL, err


@pytest.mark.parametrize("T,form", [(160, "reassoc"), (161, "direct")])
def test_auto_threshold(gpu, T, form):
    """AUTO keeps the reassociated form to MP_XA_DIRECT_T = 160 tokens and runs the direct form
    from 161: bit for bit the forced form, codes and hidden."""
    _equals_single(gpu.single("auto", T), 0, gpu.single(form, T), f"T = {T}: auto vs {form}")
    other = gpu.single("direct" if form == "reassoc" else "reassoc", T)
    assert not np.array_equal(gpu.single("auto", T).hidden, other.hidden)  # the forms do differ in rounding


# ---------------------------------------------------------------- ragged batches
@pytest.mark.parametrize("xa", FORMS)
def test_ragged_batch_across_tile_edges(gpu, orc, xa):
    """[65, 1, 64, 2]: a 65-token utterance directly before a one-token one (the conv taps of
    rows 0 and 1 of an utterance must not reach the previous utterance's last rows; M = 260
    crosses GEMM tiles inside utterances). Every slot equals its single run of the same form bit
    for bit; slots 0 and 1 also equal the oracle."""
    lens = (65, 1, 64, 2)
    rb = gpu.synthesize(xa, lens)
    for b, T in enumerate(lens):
        _equals_single(rb, b, gpu.single(xa, T), f"{xa}, slot {b} (T = {T})")
    for b in (0, 1):
        _against_oracle(rb.codes[b], rb.hidden[b], orc.run(lens[b]), f"{xa}, batch {list(lens)}, slot {b}")


def test_ragged_batch_one_token_beside_the_limit(gpu, orc):
    """[1, 1024], direct: the largest stride / length mismatch the API allows. Slot 0 equals the
    oracle; both slots equal their single runs (at M = 2048 every encoder GEMM runs its splits
    inside the workgroup, at M = 1 none does: the same bits)."""
    lens = (1, 1024)
    rb = gpu.synthesize("direct", lens)
    _against_oracle(rb.codes[0], rb.hidden[0], orc.run(1), f"direct, batch {list(lens)}, slot 0")
    for b, T in enumerate(lens):
        _equals_single(rb, b, gpu.single("direct", T), f"direct, slot {b} (T = {T})")


# ---------------------------------------------------------------- XA K/V layer groups
@pytest.fixture(scope="module")
def group_gpu(ma):
    g = GpuRuns(ma, te.group_model(ma))
    yield g
    g.close()


@pytest.fixture(scope="module")
def group_orc(ma, oracle):
    r = te.OracleRuns(ma, oracle, te.group_model(ma))
    yield r
    r.close()


@pytest.mark.parametrize("T", te.GROUP_T)
def test_xa_kv_layer_groups_match_oracle(group_gpu, group_orc, T):
    """5 decoder layers: T = 88 one group of 5, T = 89 groups of 4 + 1 (a ragged last group),
    T = 111 groups of 4 + 1 past the 110-row context; codes and hidden against the oracle."""
    r = group_gpu.single("auto", T)
    _against_oracle(r.codes[0], r.hidden[0], group_orc.run(T), f"5 layers, T = {T}")


def test_xa_kv_layer_groups_batch_equals_single(group_gpu):
    """[89, 30]: the batch's groups are 4 + 1 (Tmax = 89), the 30-token single run's one of 5."""
    rb = group_gpu.synthesize("auto", te.GROUP_BATCH)
    for b, T in enumerate(te.GROUP_BATCH):
        _equals_single(rb, b, group_gpu.single("auto", T), f"5 layers, slot {b} (T = {T})")


# ---------------------------------------------------------------- other weight families
@pytest.fixture(scope="module")
def families(ma, oracle, request):
    """(weights, model fixture, oracle weight mode) -> (GpuRuns, OracleRuns), opened on first use"""
    made = {}

    def get(weights, fixture, mode):
        if weights not in made:
            path = request.getfixturevalue(fixture)
            made[weights] = (GpuRuns(ma, path, weights=weights), te.OracleRuns(ma, oracle, path, weight_mode=mode))
        return made[weights]
    yield get
    for g, o in made.values():
        g.close()
        o.close()


@pytest.mark.parametrize("weights,fixture,mode,T,bar", te.FAMILY_CASES, ids=[f"{c[0]}-{c[3]}" for c in te.FAMILY_CASES])
def test_family_short_texts_teacher_forced(ma, families, weights, fixture, mode, T, bar):
    """bf16 / F16 / Q8_0 at the short edges (empty splits of the 16-bit families' fused XA, one
    clamped key in the Q8_0 kernels' direct attention): every decision teacher forced, the
    families' own hidden helpers and bars (test_decode_gpu.py)."""
    g, o = families(weights, fixture, mode)
    r = g.single("auto", T)
    assert r.n_frames[0] == te.STEPS
    forced = o.om.synthesize_forced(te.tokens(ma, T), r.codes[0], speaker=te.speaker(T), ignore_eos=True)
    if weights == "q8":
        res = compare_forced(r.codes[0], forced, tie_eps=te.Q8_TIE_EPS, max_ties=int(0.05 * te.STEPS * 8))
        assert te.Q8_BARS["small"][0] == bar
        _check_hidden_q8(r.hidden[0, :te.STEPS + 1], forced["hidden"], "small")
    else:
        res = compare_forced(r.codes[0], forced, tie_eps=te.BF16_TIE_EPS, max_ties=8)
        assert te.BF16_HIDDEN_TOL == bar
        _check_hidden_b16(r.hidden[0, :te.STEPS + 1], forced["hidden"])
    assert res["decisions"] == te.STEPS * 8


# ---------------------------------------------------------------- slot pool
@pytest.mark.parametrize("xa", FORMS)
def test_slot_refill_over_a_longer_predecessor(ma, gpu, xa):
    """2 slots, texts of 65, 64, 1, 2, 5, 63 tokens in that order: the one-token utterance takes
    the slot of the 65-token one, whose K / V (and K' / V') rows past T = 1 stay in place and
    must not be read. Every utterance's codes equal its single run of the same form."""
    lens = (65, 64, 1, 2, 5, 63)
    res = gpu.dev(xa).synthesize_queue([te.tokens(ma, T) for T in lens], [te.speaker(T) for T in lens], slots=2,
                                       max_dec_steps=te.STEPS, ignore_eos=True)
    assert res.slots == 2 and res.refills == len(lens) - 2
    for i, T in enumerate(lens):
        assert res.n_frames[i] == te.STEPS, (i, res.n_frames[i])
        assert np.array_equal(res.codes[i], gpu.single(xa, T).codes[0]), f"{xa}, utterance {i} (T = {T})"
