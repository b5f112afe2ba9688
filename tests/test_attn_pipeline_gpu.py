"""The attention tails keep their cached rows in flight ahead of the hand-off wait
(mp_sa.hpp, sa_part: two batches of SA_IF rounds issued at entry, a two-batch register
ring in the loop). A batch is 64 keys of a split, 256 keys over the 4 splits, so the
code takes another path wherever L = pos + 1 crosses a multiple of 256; the
cross-attention's rounds (mp_xa.hpp, xa_part) change at every 64 text tokens. Run here
on the 2-layer model, greedy with ignore_eos; the prefill context is 110 frames, so
step s attends over L = 111 + s keys:
 - L = 257 (step 146): the first key of a second batch, live in wave 0's first key
   group only; L = 321 (step 210): every wave has a second-batch key; L = 513 (step
   402): the first key of a third batch (the ring wraps);
 - f32 B = 1 over 410 steps against the oracle (codes equal, hidden within the f32 bar),
   asserted over steps [140, 160] and [395, 409] apart so a failure names its boundary,
   from the captured graph and launched eagerly (MAGPIE_EAGER=1, a fresh child process);
 - batch equals single, bit for bit, over 160 steps: f32 B = 3, bf16 B = 8 with the bf16
   cache (the KV16 tail), bf16 B = 16 (the standalone sa_attn_kernel);
 - the Q8_0 model at B = 1 over 160 steps (sa_attn_kernel, no hand-off), teacher forced
   against the oracle under tests/test_decode_gpu.py's small-Q8 bars;
 - texts of 64 (one XA round), 65 (chunk 17: only wave 0 has a second-round key), 100
   (every wave has two rounds) and 150 tokens (three rounds), 9 frames: f32 B = 1
   against the oracle, 150 also with the direct form, and 64 / 100 / 150 in one batch
   against their single runs, bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

from parity import compare_forced

pytestmark = pytest.mark.gpu

HIDDEN_TOL = 2e-5  # f32 vs the acc64 oracle (tests/test_kernarg_lead_gpu.py, tests/test_decode_gpu.py)
Q8_TIE_EPS, Q8_TIE_FRAC, Q8_BAR = 1e-1, 0.05, (1e-2, 3e-3)  # tests/test_decode_gpu.py: Q8_TIE_EPS, Q8_BARS["small"]
SA_STEPS, BATCH_STEPS, T, SEED = 410, 160, 24, 1000
SA_WINDOWS = ((140, 160), (395, 409))  # steps around L = 257 and L = 513, inclusive
XA_STEPS, XA_TS = 9, (64, 65, 100, 150)
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ma():
    import magpie_amd
    if magpie_amd.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    return magpie_amd


def _frozen(*arrays):
    out = [np.asarray(a) for a in arrays]
    for a in out:
        a.setflags(write=False)
    return tuple(out)


@pytest.fixture(scope="module")
def sa_reference(ma, oracle, small_model):
    """the oracle's (codes, hidden) over SA_STEPS steps of the T-token text; read-only"""
    om = oracle.Model(small_model)
    o = om.synthesize(ma.synthetic_tokens(T, seed=SEED), speaker=0, max_steps=SA_STEPS, ignore_eos=True, trace=True)
    om.close()
    assert np.asarray(o["codes"]).shape == (SA_STEPS, 8)
    return _frozen(o["codes"], o["hidden"])


@pytest.fixture(scope="module")
def xa_reference(ma, oracle, small_model):
    """{T: the oracle's (codes, hidden)} over XA_STEPS steps of the texts of XA_TS tokens; read-only"""
    om = oracle.Model(small_model)
    out = {}
    for i, t in enumerate(XA_TS):
        o = om.synthesize(ma.synthetic_tokens(t, seed=SEED + i), speaker=i % 5, max_steps=XA_STEPS, ignore_eos=True,
                          trace=True)
        out[t] = _frozen(o["codes"], o["hidden"])
    om.close()
    return out


def _check_sa(codes, hidden, ref, what):
    oc, oh = ref
    codes, hidden = np.asarray(codes), np.asarray(hidden)
    assert codes.shape == oc.shape, f"{what}: {codes.shape[0]} frames"
    err = np.abs(hidden[:SA_STEPS + 1] - oh[:SA_STEPS + 1]).max(axis=1)
    for lo, hi in SA_WINDOWS:
        e = float(err[lo:hi + 1].max())
        print(f"{what}, steps {lo}..{hi} (L = {111 + lo}..{111 + hi}): hidden max abs err {e:.3g}")
        assert np.array_equal(codes[lo:hi + 1], oc[lo:hi + 1]), f"{what}: codes differ from the oracle's in steps {lo}..{hi}"
        assert e < HIDDEN_TOL, f"{what}: hidden max abs err {e} in steps {lo}..{hi}"
    print(f"{what}, all {SA_STEPS} steps: hidden max abs err {float(err.max()):.3g} (step {int(err.argmax())})")
    assert np.array_equal(codes, oc), f"{what}: codes differ from the oracle's"
    assert err.max() < HIDDEN_TOL, f"{what}: hidden max abs err {err.max()} at step {int(err.argmax())}"


def test_sa_batch_boundaries_f32_match_oracle(ma, small_model, sa_reference):
    dev = ma.Device(small_model, weights="f32")
    r = dev.synthesize([ma.synthetic_tokens(T, seed=SEED)], speakers=[0], max_dec_steps=SA_STEPS, ignore_eos=True,
                       trace=True)
    dev.close()
    _check_sa(r.codes[0], r.hidden[0], sa_reference, "graph f32 B=1")


CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import magpie_amd as ma
path, out, steps, T, seed = sys.argv[2], sys.argv[3], int(sys.argv[4]), int(sys.argv[5]), int(sys.argv[6])
dev = ma.Device(path, weights="f32")
r = dev.synthesize([ma.synthetic_tokens(T, seed=seed)], speakers=[0], max_dec_steps=steps, ignore_eos=True, trace=True)
dev.close()
np.savez(out, codes=np.asarray(r.codes[0]), hidden=np.asarray(r.hidden[0]))
"""


def test_sa_batch_boundaries_f32_eager_match_oracle(ma, small_model, sa_reference, tmp_path):
    out = str(tmp_path / "eager.npz")
    env = dict(os.environ, MAGPIE_EAGER="1")
    p = subprocess.run([sys.executable, "-c", CHILD, os.path.join(REPO, "magpie-tts.cpp_amd"), small_model, out,
                        str(SA_STEPS), str(T), str(SEED)], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-3000:]
    z = np.load(out)
    _check_sa(z["codes"], z["hidden"], sa_reference, "eager f32 B=1")


@pytest.mark.parametrize("weights,kv,B", [("f32", "f32", 3), ("bf16", "bf16", 8), ("bf16", "f32", 16)])
def test_sa_batch_equals_single_across_boundary(ma, small_model, weights, kv, B):
    """steps 0..159: L = 111..270, over the first batch boundary in every slot"""
    toks = [ma.synthetic_tokens(T + b, seed=SEED + b) for b in range(B)]
    spk = [b % 5 for b in range(B)]
    kw = dict(max_dec_steps=BATCH_STEPS, ignore_eos=True, trace=True)
    dev = ma.Device(small_model, weights=weights, kv=kv)
    rb = dev.synthesize(toks, speakers=spk, **kw)
    assert (np.asarray(rb.n_frames) == BATCH_STEPS).all()
    for b in range(B):
        rs = dev.synthesize([toks[b]], speakers=[spk[b]], **kw)
        assert np.array_equal(rb.codes[b], rs.codes[0]), f"{weights} kv={kv} B={B}, slot {b}: codes differ from the single run's"
        assert np.array_equal(rb.hidden[b], rs.hidden[0]), f"{weights} kv={kv} B={B}, slot {b}: hidden differs from the single run's"
    dev.close()


def test_sa_batch_boundary_q8_matches_oracle(ma, oracle, q8_model):
    tok = ma.synthetic_tokens(T, seed=SEED)
    dev = ma.Device(q8_model, weights="q8")
    r = dev.synthesize([tok], speakers=[1], max_dec_steps=BATCH_STEPS, ignore_eos=True, trace=True)
    dev.close()
    om = oracle.Model(q8_model)
    om.set_weight_mode(2)
    o = om.synthesize_forced(tok, r.codes[0], speaker=1, ignore_eos=True)
    om.close()
    res = compare_forced(r.codes[0], o, tie_eps=Q8_TIE_EPS, max_ties=int(Q8_TIE_FRAC * BATCH_STEPS * 8))
    assert res["decisions"] == BATCH_STEPS * 8
    h, ho = np.asarray(r.hidden[0, :BATCH_STEPS + 1]), np.asarray(o["hidden"])
    nrm = np.linalg.norm(ho, axis=-1)
    live = nrm > 0  # the last trace row of a run that ends at max_dec_steps is unwritten on both sides
    err = float(np.abs(h - ho).max())
    rel = float((np.linalg.norm(h - ho, axis=-1)[live] / nrm[live]).max())
    print(f"Q8 B=1, {BATCH_STEPS} steps: {res}, hidden max abs err {err:.3g}, max relative L2 {rel:.3g}")
    assert err < Q8_BAR[0], f"hidden max abs err {err}"
    assert rel < Q8_BAR[1], f"hidden max relative L2 err {rel}"


def _run_xa(ma, path, ts, xa="auto"):
    idx = [XA_TS.index(t) for t in ts]
    dev = ma.Device(path, weights="f32", xa=xa)
    r = dev.synthesize([ma.synthetic_tokens(t, seed=SEED + i) for t, i in zip(ts, idx)], speakers=[i % 5 for i in idx],
                       max_dec_steps=XA_STEPS, ignore_eos=True, trace=True)
    dev.close()
    return r


def _check_xa(r, b, ref, what):
    oc, oh = ref
    assert np.array_equal(np.asarray(r.codes[b]), oc), f"{what}: codes differ from the oracle's"
    err = float(np.abs(np.asarray(r.hidden[b])[:XA_STEPS + 1] - oh[:XA_STEPS + 1]).max())
    print(f"{what}: hidden max abs err {err:.3g}")
    assert err < HIDDEN_TOL, f"{what}: hidden max abs err {err}"


@pytest.mark.parametrize("t", XA_TS)
def test_xa_round_edges_f32_match_oracle(ma, small_model, xa_reference, t):
    _check_xa(_run_xa(ma, small_model, [t]), 0, xa_reference[t], f"T={t}")


def test_xa_three_rounds_direct_form_matches_oracle(ma, small_model, xa_reference):
    _check_xa(_run_xa(ma, small_model, [150], xa="direct"), 0, xa_reference[150], "direct XA T=150")


def test_xa_round_edges_batch_equals_single(ma, small_model):
    ts = [64, 100, 150]
    rb = _run_xa(ma, small_model, ts)
    for b, t in enumerate(ts):
        rs = _run_xa(ma, small_model, [t])
        assert np.array_equal(rb.codes[b], rs.codes[0]), f"slot {b} (T={t}): codes differ from the single run's"
        assert np.array_equal(rb.hidden[b], rs.hidden[0]), f"slot {b} (T={t}): hidden differs from the single run's"
