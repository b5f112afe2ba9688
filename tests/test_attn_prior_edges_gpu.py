"""The attention prior's kernels at every edge (the case table, the restatement and what each
case is the edge of: tests/attn_prior_cases.py; the preconditions that keep these tests from
passing vacuously: tests/test_attn_prior_cpu.py).

  f32     against the numpy f64 restatement: codes identical on every frame, att[:steps]
          identical, hidden within HIDDEN_TOL = 2e-5 (text edges in both XA forms, window edges
          of xa_align_kernel, start_step, the 12-layer row staging against the stored fixture)
  bf16    teacher forced along the device's own codes and att: hidden within the bf16 bars, every
          code decision through parity.compare_forced, every vote the restated maximum or within
          ALIGN_TIE_BF16 of it (at most 1 frame in 12)
  guidance, one captured graph across settings and text lengths, streaming, the refusal of more
  than 12 masked layers
"""
import os

import numpy as np
import pytest

import attn_prior_cases as ap
from parity import compare_forced
from test_attn_prior_gpu import device, run, same_bits
from test_decode_gpu import BF16_TIE_EPS, HIDDEN_TOL, _check_hidden_b16

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ma():
    import magpie_amd
    if magpie_amd.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    return magpie_amd


@pytest.fixture(scope="module")
def model64(small_model):
    return ap.mi.Magpie(small_model)


@pytest.fixture(scope="module")
def gpu(ma, small_model):
    """one f32 Device per XA form, opened on first use, and their runs, each computed once"""
    devs, runs = {}, {}

    def get(xa, T, W, start, layers, steps, seed, prior=True):
        key = (xa, T, W, start, layers, steps, seed, prior)
        if key not in runs:
            if xa not in devs:
                devs[xa] = ma.Device(small_model, xa=xa)
            runs[key] = run(devs[xa], [ap.tokens(ma, T, seed)], (ap.EPS, W, start, layers) if prior else None, steps=steps,
                            ignore_eos=True)
        return runs[key]
    yield get
    for d in devs.values():
        d.close()


def _against(r, att, b, ref, what, tol=HIDDEN_TOL, hidden=None, want_hidden=None):
    """codes and att identical on every frame, the hidden trace within the f32 bar"""
    n = len(ref["codes"])
    assert int(r.n_frames[b]) == n and np.array_equal(r.codes[b], ref["codes"]), f"{what}: codes"
    assert np.array_equal(att[b, :n], ref["att"]), f"{what}: att {att[b, :n].tolist()} vs {ref['att'].tolist()}"
    got = r.hidden[b] if hidden is None else hidden
    want = ref["hidden"] if want_hidden is None else want_hidden
    err = float(np.abs(got[:len(want)].astype(np.float64) - want).max())
    print(f"{what}: hidden max abs err {err:.2e}")
    assert err < tol, f"{what}: hidden max abs err {err}"
    return err


# ---------------------------------------------------------------- f32: text edges
@pytest.mark.parametrize("T,W,seed,xa", [(T, W, s, xa) for T, W, s in ap.EDGES for xa in ap.FORMS])
def test_text_edge_matches_restatement(ma, gpu, model64, T, W, seed, xa):
    ref, _ = ap.reference(model64, ma, T, W, 0, 0, ap.EDGE_STEPS, seed)
    r, att = gpu(xa, T, W, 0, 0, ap.EDGE_STEPS, seed)
    _against(r, att, 0, ref, f"T {T} W {W} {xa}")


@pytest.mark.parametrize("T,form", [(160, "reassoc"), (161, "direct")])
def test_auto_threshold_with_prior(ma, gpu, model64, T, form):
    """AUTO with a prior keeps the reassociated form to 160 tokens and runs the direct one from
    161: bit for bit the forced form (test_text_edges_gpu.py::test_auto_threshold's rule)."""
    W, seed = next((W, s) for t, W, s in ap.EDGES if t == T)
    ra, aa = gpu("auto", T, W, 0, 0, ap.EDGE_STEPS, seed)
    _against(ra, aa, 0, ap.reference(model64, ma, T, W, 0, 0, ap.EDGE_STEPS, seed)[0], f"T {T} auto")
    rf, af = gpu(form, T, W, 0, 0, ap.EDGE_STEPS, seed)
    same_bits(ra, aa, 0, rf, af, 0)
    other = gpu("direct" if form == "reassoc" else "reassoc", T, W, 0, 0, ap.EDGE_STEPS, seed)[0]
    assert not np.array_equal(ra.hidden, other.hidden)  # the forms do differ in rounding


# ---------------------------------------------------------------- f32: window edges, start_step
@pytest.mark.parametrize("name,T,xa,W,start,steps,seed", ap.WINDOWS, ids=[c[0] for c in ap.WINDOWS])
def test_window_edge_matches_restatement(ma, gpu, model64, name, T, xa, W, start, steps, seed):
    ref, _ = ap.reference(model64, ma, T, W, start, 0, steps, seed)
    r, att = gpu(xa, T, W, start, 0, steps, seed)
    _against(r, att, 0, ref, f"{name}: T {T} W {W} start {start} {xa}")
    if start > steps:  # lp all zero throughout: the plain run bit for bit, the alignment still voted
        same_bits(r, None, 0, gpu(xa, T, W, start, 0, steps, seed, prior=False)[0], None, 0)


@pytest.mark.parametrize("T,xa,W", ap.TIED_CASES)
def test_equal_votes_take_the_first_position(ma, small_model, T, xa, W):
    """every window position holds the same avg, bit for bit (K = V = 0: test_attn_prior_cpu.py),
    across the four waves and a thread's several positions: a' is a itself on every frame"""
    with device(ma, ap.tied_model(small_model), xa=xa) as dev:
        r, att = run(dev, [ap.tokens(ma, T, ap.TIED_SEED)], (ap.EPS, W, 0, 0), steps=ap.TIED_STEPS, ignore_eos=True)
    assert int(r.n_frames[0]) == ap.TIED_STEPS
    assert not att[0, :ap.TIED_STEPS].any(), att[0, :ap.TIED_STEPS].tolist()


# ---------------------------------------------------------------- f32: 12 layers, the row staging
@pytest.fixture(scope="module")
def full_dev(ma, full_model):
    with device(ma, full_model) as dev:
        yield dev


@pytest.mark.parametrize("i", range(len(ap.FULL_CASES)), ids=[f"mask{c[0]:#x}" for c in ap.FULL_CASES])
def test_full_depth_row_staging(ma, full_dev, i):
    """Magpie-357M's 12 layers, T = 64: all 12 masked (three rows per wave), 0b11111 (wave 0
    takes rows 0 and 4), layers {3, 7, 10} (nm != l, wave 3 idle), layer 11 alone; against the
    stored restatement (tests/golden/make_attn_prior.py)."""
    g = np.load(ap.GOLD_FULL)
    mask, W = int(g[f"m{i}_mask"]), int(g[f"m{i}_W"])
    assert (mask, W) == ap.FULL_CASES[i][:2]
    ref = {k: g[f"m{i}_{k}"] for k in ("codes", "att", "hidden")}
    r, att = run(full_dev, [g[f"m{i}_tokens"]], (ap.EPS, W, 0, mask), steps=ap.FULL_STEPS, ignore_eos=True)
    _against(r, att, 0, ref, f"12 layers, mask {mask:#x}", want_hidden=ref["hidden"].astype(np.float64))


# ---------------------------------------------------------------- bf16
@pytest.fixture(scope="module")
def bf16_dev(ma, small_model):
    devs = {}

    def get(xa):
        if xa not in devs:
            devs[xa] = ma.Device(small_model, weights="bf16", xa=xa)
        return devs[xa]
    yield get
    for d in devs.values():
        d.close()


def _bf16_slot(ma, model64, r, att, b, tok, spk, W, what):
    n = ap.BF16_STEPS
    assert int(r.n_frames[b]) == n
    ref = ap.restate(model64, tok, spk, n, ap.EPS, W, forced=(r.codes[b], att[b, :n]), bf16=True, ignore_eos=True)
    _check_hidden_b16(r.hidden[b, :n].astype(np.float64), ref["hidden"])
    res = compare_forced(r.codes[b], ref, tie_eps=BF16_TIE_EPS, max_ties=ap.BF16_MAX_TIES)
    assert res["decisions"] == n * 8
    exact = 0
    for f in range(n):
        win, a = ref["avg"][f], int(ref["base"][f])
        got = int(att[b, f]) - a
        assert 0 <= got < len(win), f"{what}: frame {f}: att {att[b, f]} outside the window from {a}"
        gap = float(win.max() - win[got])
        assert gap <= ap.ALIGN_TIE_BF16, f"{what}: frame {f}: att {att[b, f]}, restated avg {gap:.3g} under the window's maximum"
        exact += int(att[b, f]) == int(ref["att"][f])
    print(f"{what}: {exact} of {n} votes are the restated first maximum")
    assert exact >= n - 1


@pytest.mark.parametrize("T,xa,W,seed", ap.BF16_CASES)
def test_bf16_teacher_forced(ma, bf16_dev, model64, T, xa, W, seed):
    tok = ap.tokens(ma, T, seed)
    r, att = run(bf16_dev(xa), [tok], (ap.EPS, W, 0, 0), steps=ap.BF16_STEPS, ignore_eos=True)
    _bf16_slot(ma, model64, r, att, 0, tok, 0, W, f"bf16 T {T} {xa}")


@pytest.mark.parametrize("B,slots", [(16, (0, 15)), (8, (7,))])
def test_bf16_merged_sa_batches(ma, bf16_dev, model64, B, slots):
    """the T = 70 case as slots 0 and 15 of a 16-slot batch and slot 7 of an 8-slot one (the
    merged-SA forms of gemm_b16_kernel<.., EPI_RESID_XAP>), each against the restatement"""
    T, xa, W, seed = ap.BF16_CASES[0]
    tok = ap.tokens(ma, T, seed)
    toks = [tok if b in slots else ap.tokens(ma, (5, 12, 33)[b % 3], 300 + b) for b in range(B)]
    r, att = run(bf16_dev(xa), toks, (ap.EPS, W, 0, 0), [0] * B, steps=ap.BF16_STEPS, ignore_eos=True)
    for b in slots:
        _bf16_slot(ma, model64, r, att, b, tok, 0, W, f"bf16 T {T} {xa}, slot {b} of {B}")


# ---------------------------------------------------------------- guidance
@pytest.mark.parametrize("lens", [(70,), (70, 5, 33)])
def test_guidance_with_prior_matches_restatement(ma, small_model, model64, lens):
    """scale 2.5, prior (0.1, 5, 0, 0): the prior and the vote belong to the conditional slot,
    the partner's lp stays zero; both branches' traces at test_cfg_gpu.py's bars"""
    toks = [ap.tokens(ma, T, ap.CFG_SEEDS[T]) for T in lens]
    with device(ma, small_model) as dev:
        dev.set_cfg(ap.CFG_SCALE)
        r, att = run(dev, toks, (ap.EPS, 5, 0, 0), steps=ap.CFG_STEPS, ignore_eos=True)
    for b, T in enumerate(lens):
        ref = ap.cfg_reference(model64, ma, T)
        _against(r, att, b, ref, f"guided T {T}, slot {b} of {len(lens)}")
        _against(r, att, b, ref, f"guided T {T}, slot {b} of {len(lens)}, partner", hidden=r.hidden_uncond[b],
                 want_hidden=ref["hidden_uncond"])


# ---------------------------------------------------------------- one graph, changing state
def _fresh(ma, small_model, toks, prior, steps=12, **kw):
    with device(ma, small_model, **kw) as dev:
        return run(dev, toks, prior, steps=steps, ignore_eos=True)


def test_one_graph_serves_changing_settings(ma, small_model):
    """(0.1, 5, 0, all), (0.3, 2, 1, layer 1), prior off, the first again, all at T = 70 on one
    Device: each equals a fresh device's run bit for bit (PriorCfg is read from device memory;
    reset_decode_state zeroes lp, att_pos and att_out)"""
    tok = [ap.tokens(ma, 70, 1)]
    settings = [(ap.EPS, 5, 0, 0), (0.3, 2, 1, 2), None, (ap.EPS, 5, 0, 0)]
    with device(ma, small_model) as dev:
        got = [run(dev, tok, s, steps=12, ignore_eos=True) for s in settings]
    want = [_fresh(ma, small_model, tok, s) for s in settings[:3]]
    for i, (r, a) in enumerate(got):
        same_bits(r, a, 0, *want[i % 3], 0)
    assert not np.array_equal(got[0][0].codes[0], got[1][0].codes[0])
    assert not np.array_equal(got[0][0].codes[0], got[2][0].codes[0])


def test_short_text_after_long_in_the_same_slot(ma, small_model):
    """T = 200 then T = 9 alone, and the batch [200, 9] then [9, 200] (one Tmax, so the buffers
    and the graph stay): stale lp / scores beyond the new T must not be read"""
    prior = (ap.EPS, 5, 0, 0)
    long_, short = ap.tokens(ma, 200, 6), ap.tokens(ma, 9, 0)
    with device(ma, small_model, xa="reassoc") as dev:
        run(dev, [long_], prior, steps=12, ignore_eos=True)
        r9, a9 = run(dev, [short], prior, steps=12, ignore_eos=True)
        run(dev, [long_, short], prior, [0, 0], steps=12, ignore_eos=True)
        rb, ab = run(dev, [short, long_], prior, [0, 0], steps=12, ignore_eos=True)
    w9 = _fresh(ma, small_model, [short], prior, xa="reassoc")
    w200 = _fresh(ma, small_model, [long_], prior, xa="reassoc")
    same_bits(r9, a9, 0, *w9, 0)
    same_bits(rb, ab, 0, *w9, 0)
    same_bits(rb, ab, 1, *w200, 0)


def test_batch_reordered_on_one_device(ma, small_model):
    """[70, 5, 12] then [5, 70, 12]: every slot equals its fresh single run"""
    prior = (ap.EPS, 5, 0, 0)
    toks = {T: ap.tokens(ma, T, 100 + T) for T in (70, 5, 12)}
    with device(ma, small_model) as dev:
        run(dev, [toks[70], toks[5], toks[12]], prior, [0, 0, 0], steps=12, ignore_eos=True)
        rb, ab = run(dev, [toks[5], toks[70], toks[12]], prior, [0, 0, 0], steps=12, ignore_eos=True)
    for b, T in enumerate((5, 70, 12)):
        same_bits(rb, ab, b, *_fresh(ma, small_model, [toks[T]], prior), 0)


# ---------------------------------------------------------------- streaming
@pytest.mark.parametrize("model,chunk", [("small_model", 4), ("small_model", 3), ("eos_model", 4), ("eos_model", 3)])
def test_streaming_decode_with_prior(ma, request, codec_model, model, chunk):
    """mp_hip_decode_stream with a prior: the codes delivered, n_frames and alignment() equal
    mp_hip_decode's of the same batch (begun as the streaming call begins it: the EOS frame
    emitted), bit for bit; on eos_model a slot stops inside a chunk"""
    toks = [ma.synthetic_tokens(40, seed=7), ma.synthetic_tokens(52, seed=9)]
    steps = 10
    codec = ma.Codec(codec_model)
    try:
        with device(ma, request.getfixturevalue(model)) as dev:
            dev.set_attn_prior(ap.EPS, 3, 0, 0)
            B = dev.begin(toks, [0, 1], max_dec_steps=steps, emit_eos_frame=True)
            want = dev.decode(B, steps)
            want_att = dev.alignment()
            codes, total, _ = dev.synthesize_stream(codec, toks, lambda u, s: True, speakers=[0, 1], max_dec_steps=steps,
                                                    frames_per_chunk=chunk)
            att = dev.alignment()
    finally:
        codec.close()
    nf = [len(c) for c in codes]
    print(f"{model}, {chunk}-frame chunks: frames {nf}")
    if model == "eos_model":  # a slot stops inside a chunk
        assert 0 < min(nf) < steps and min(nf) % chunk != 0
    assert total == sum(nf) * 1024
    for b in range(2):
        assert nf[b] == int(want.n_frames[b]) and np.array_equal(codes[b], want.codes[b])
        assert np.array_equal(att[b, :nf[b]], want_att[b, :nf[b]])
        assert np.all(np.diff(att[b, :nf[b]]) >= 0)


# ---------------------------------------------------------------- more than 12 masked layers
def test_thirteen_masked_layers_are_refused(ma):
    """dec_layers = 13: layers = 0 (all 13) is MP_ERR_UNSUPPORTED from begin and the device then
    reproduces its plain run; 12 of 13 with bit 12 set run (nm stops at 12 rows of the LDS table)"""
    cache = os.environ.get("MAGPIE_CACHE", "/tmp/magpie_amd_cache")
    os.makedirs(cache, exist_ok=True)
    path = ma.synth_gguf(os.path.join(cache, "magpie_l13e1_k32.gguf"), lt_head_scale=ma.DECISIVE, dec_layers=13, enc_layers=1)
    tok, T = ma.synthetic_tokens(24, seed=5), 24
    with device(ma, path) as dev:
        assert dev.model_info()["dec_layers"] == 13
        want, _ = run(dev, [tok], steps=8, ignore_eos=True)
        dev.set_attn_prior(ap.EPS, 5, 0, 0)
        with pytest.raises(ma.MagpieError, match="MP_ERR_UNSUPPORTED"):
            dev.begin([tok], max_dec_steps=8, ignore_eos=True, trace=True)
        got, _ = run(dev, [tok], steps=8, ignore_eos=True)
        same_bits(got, None, 0, want, None, 0)
        r, att = run(dev, [tok], (ap.EPS, 5, 0, 0x1FFE), steps=8, ignore_eos=True)
    a = att[0, :8]
    assert int(r.n_frames[0]) == 8 and a.min() >= 0 and a.max() <= T - 1 and np.all(np.diff(a) >= 0)
