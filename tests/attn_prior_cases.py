"""The attention prior (mp_hip_set_attn_prior, include/magpie_hip.h): the numpy f64 restatement,
the case table and the margins shared by test_attn_prior_gpu.py, test_attn_prior_cpu.py (the
reference's own preconditions) and test_attn_prior_edges_gpu.py (the kernels at every edge).

restate() is built from tests/golden/make_indep.py's Magpie and tests/golden/make_cfg.py's guided
pick with the semantics of include/magpie_hip.h. Every token seed below was chosen on the CPU
(test_attn_prior_cpu.py holds what it was chosen for): the reference's own code decisions and
alignment votes are no near-ties, the prior changes codes and alignment entries against the
plain run, and each named edge is visited by the reference's own `att`.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_cfg as mc  # noqa: E402
import make_indep as mi  # noqa: E402

EPS = 0.1
MIN_MARGIN, MIN_ALIGN_MARGIN = 1e-3, 1e-4  # make_cfg.py's MIN_MARGIN; the alignment's top-1 / top-2 gap
GOLD_FULL = os.path.join(HERE, "golden", "attn_prior_full.npz")
# Depth (tests/golden/make_attn_prior.py writes GOLD_FULL): (layer mask, W, token seed). Layer 11
# alone votes with W = 20, not 5: of seeds 0..199 at W = 5, 45 miss a margin and the other 155
# change codes but move no att entry against the prior-off run (one late layer's vote barely
# follows the codes in this synthetic model; W = 10 was tried for seeds 0..16 only, with the
# same outcome). At W = 20 the window stays inside wave 0 and the staging is the same one row.
FULL_T, FULL_STEPS = 64, 12
FULL_CASES = [(0xFFF, 5, 0), (0b11111, 5, 0), (1 << 3 | 1 << 7 | 1 << 10, 5, 1), (1 << 11, 20, 2)]


def tokens(ma, T, seed):
    return ma.synthetic_tokens(T, seed=seed)


# ---------------------------------------------------------------- the restatement
def bf16r(x):
    """f64 -> f32 -> bf16 (round to nearest even) -> f64, the rounding of the oracle's weight mode 1"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    u = (u + (np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1)))) & np.uint32(0xFFFF0000)
    return u.view(np.float32).astype(np.float64)


class _Proj:
    """x @ w.T of one restatement run. half: w and x rounded to bf16, products exact (the oracle's
    weight mode 1 projection). acc32: the sum accumulated in f32 (both operands cast to f32; the
    f64 sum otherwise). key names a weight whose rounded / cast copy is kept for the run."""

    def __init__(self, acc32):
        self.acc32, self._w = acc32, {}

    def __call__(self, x, w, half=False, key=None):
        if not half and not self.acc32:
            return x @ w.T
        if key is None or (key, half) not in self._w:
            wr = bf16r(w) if half else w
            wr = wr.astype(np.float32) if self.acc32 else wr
            if key is not None:
                self._w[(key, half)] = wr
        else:
            wr = self._w[(key, half)]
        xr = bf16r(x) if half else x
        if self.acc32:
            return (xr.astype(np.float32) @ wr.T).astype(np.float64)
        return xr @ wr.T


def _lt_pick(M, hiddens, scale, forbid_eos, force, bf16, P):
    """The frame's 8 picks from one hidden state (or the guided pair's two, mixed by `scale`):
    (codes, argmax, margins). force: the codes the next codebooks are conditioned on (teacher
    forcing; the picks returned are still this restatement's own). bf16: the LT's FFN and
    output heads as the oracle's weight mode 1 has them (in_proj and attention stay f32)."""
    seqs = [[M.lt_in_w @ h + M.lt_in_b] for h in hiddens]
    forbidden = mc._forbidden(forbid_eos)
    codes, amax, margins = [], [], []
    for cb in range(8):
        lg = []
        for seq in seqs:
            if bf16:
                x = np.array(seq) + M.lt_pos[:len(seq)]
                q, k, v = mi.qkv_split(mi.layer_norm(x, M.lt["ln1"]), M.lt["qkv"])
                x = mi.attend(q, k, v, 1, 0) @ M.lt["o"].T + x
                f = mi.gelu(P(mi.layer_norm(x, M.lt["ln2"]), M.lt["f1"][:, :, 0], True, "lt_f1"))
                y = P(f, M.lt["f2"][:, :, 0], True, "lt_f2") + x
                lg.append(P(y[-1], M.lt_out_w[cb], True, ("lt_out", cb)) + M.lt_out_b[cb])
            else:
                lg.append(M.lt_out_w[cb] @ M.lt_layer(np.array(seq))[-1] + M.lt_out_b[cb])
        mixed = lg[0].copy() if len(lg) == 1 else scale * lg[0] + (1.0 - scale) * lg[1]
        mixed[forbidden] = -np.inf
        am = int(np.argmax(mixed))
        top2 = np.sort(mixed)[-2:]
        codes.append(am)
        amax.append(am)
        margins.append(float(top2[1] - top2[0]))
        if cb < 7:
            nxt = M.lt_in_w @ M.audio_emb[cb][int(force[cb]) if force is not None else am] + M.lt_in_b
            for seq in seqs:
                seq.append(nxt)
    return codes, amax, margins


def encode(M, tokens):
    """Magpie.encode with every conv tap's weights laid out contiguously once per model (the same
    sums through the BLAS path: the strided taps make T = 1024 take half a minute)."""
    if not hasattr(M, "_taps"):
        M._taps = [{n: [np.ascontiguousarray(L[n][:, :, k].T) for k in range(L[n].shape[2])] for n in ("f1", "f2")}
                   for L in M.enc]
    T = len(tokens)
    x = M.text_emb[np.asarray(tokens)] + M.enc_pos[:T]
    for L, taps in zip(M.enc, M._taps):
        q, k, v = mi.qkv_split(mi.layer_norm(x, L["ln1"]), L["qkv"])
        x = mi.attend(q, k, v, mi.H, 0) @ L["o"].T + x
        h = mi.layer_norm(x, L["ln2"])
        for n in ("f1", "f2"):  # causal conv, left pad k - 1 (make_indep.conv_ffn)
            ks = len(taps[n])
            pad = np.concatenate([np.zeros((ks - 1, h.shape[1])), h], axis=0)
            h = sum(pad[tap:tap + T] @ taps[n][tap] for tap in range(ks))
            if n == "f1":
                h = mi.gelu(h)
        x = h + x
    return mi.layer_norm(x, M.enc_norm)


def restate(M, tokens, speaker, max_steps, eps=None, W=0, start=0, layers=0, forced=None, bf16=False, cfg_scale=None,
            ignore_eos=False, acc32=False, partner_is_cond=False):
    """Magpie.synthesize with the attention prior (eps None: plain; the alignment is still voted).

    forced=(codes, att): teacher forcing. Frame f + 1's input codes come from codes[f] and its
        `a` and `lp` from att[f] (att None: this run's own), not from this run's picks; the picks,
        the votes, the per-frame window `avg` and the margins returned are still its own. The
        codebooks inside a frame are conditioned on codes[f] too.
    bf16: the decode steps' qkv / o / ff1 / ff2 projections and the LT's FFN and output heads
        take bf16-rounded weights and bf16-rounded activations, as the oracle's weight mode 1
        (oracle/magpie_oracle.c: orc_set_weight_mode, matmul_sel, decoder_layer's M == 1 rows,
        lt_sample); the prefill, the cross-attention and the LT's in_proj / attention stay f32.
    cfg_scale: the guided pair of make_cfg.py (synthesize_cfg's text-free branch: XA K = V = 0,
        the context rows the decoder positions alone, its own SA cache, the conditional branch's
        input frames; lt_sample_pair's mixed pick). The prior and the vote belong to the
        conditional branch; the partner's lp stays zero. partner_is_cond: the partner's LT row
        replaced by the conditional one (what test_attn_prior_cpu.py holds the pick against).
    acc32: the projections' sums accumulated in f32 (what ALIGN_TIE_BF16 is measured from).
    """
    T = len(tokens)
    P = _Proj(acc32)
    mask = layers or (1 << M.n_dec) - 1
    enc = encode(M, tokens)
    kvs = [mi.layer_norm(enc, L["lnm"]) @ L["xkv"].T for L in M.dec]
    xk, xv = [kv[:, :mi.XA_D] for kv in kvs], [kv[:, mi.XA_D:] for kv in kvs]
    rows = mi.CTX_FRAMES + max_steps + 16
    # branch 0: the utterance; branch 1 (guided): its text-free partner
    tabs = [(xk, xv)]
    ctx = [M.baked[speaker].reshape(mi.CTX_FRAMES, mi.D) + M.dec_pos[:mi.CTX_FRAMES]]
    if cfg_scale is not None:
        tabs.append(([np.zeros((T, mi.XA_D)) for _ in M.dec], [np.zeros((T, mi.XA_D)) for _ in M.dec]))
        ctx.append(M.dec_pos[:mi.CTX_FRAMES].copy())
    caches = [[(np.zeros((rows, mi.D)), np.zeros((rows, mi.D))) for _ in range(M.n_dec)] for _ in tabs]
    for (k_, v_), x, cache in zip(tabs, ctx, caches):
        for l in range(M.n_dec):
            x = M.dec_layer(l, x, 0, cache, k_, v_)
    Lp = float(np.float32(np.log(float(np.float32(eps))))) if eps is not None else 0.0
    a, lp, pos, prev = 0, np.zeros(T), mi.CTX_FRAMES, [mi.AUDIO_BOS] * 8
    frames, hidden, hidden_u, att, margins, amargins, wins, bases = [], [], [], [], [], [], [], []
    for f in range(max_steps):
        x0 = (M.frame_embedding(prev) + M.dec_pos[pos])[None, :]
        avg = np.zeros(T)
        hs = []
        for br, ((k_, v_), cache) in enumerate(zip(tabs, caches)):
            x = x0.copy()
            for l, L in enumerate(M.dec):  # dec_layer, + lp inside the masked layers' softmax
                qkv = P(mi.layer_norm(x, L["ln1"]), L["qkv"], bf16, ("qkv", l))
                q, k, v = qkv[:, :mi.D], qkv[:, mi.D:2 * mi.D], qkv[:, 2 * mi.D:]
                cache[l][0][pos], cache[l][1][pos] = k[0], v[0]
                x = P(mi.attend(q, cache[l][0][:pos + 1], cache[l][1][:pos + 1], mi.H, pos), L["o"], bf16, ("o", l)) + x
                sc = P(P(mi.layer_norm(x, L["lnq"]), L["xq"], key=("xq", l)), k_[l]) / np.sqrt(mi.XA_D)
                if br == 0 and mask >> l & 1:
                    sc = sc + lp
                    avg = avg + mi.softmax(sc)[0]
                x = P(P(mi.softmax(sc), v_[l].T), L["xo"], key=("xo", l)) + x
                h = mi.gelu(P(mi.layer_norm(x, L["ln2"]), L["f1"][:, :, 0], bf16, ("f1", l)))
                x = P(h, L["f2"][:, :, 0], bf16, ("f2", l)) + x
            hs.append(mi.layer_norm(x[0], M.dec_norm))
        hidden.append(hs[0])
        if cfg_scale is not None:
            hidden_u.append(hs[1])
        win = avg[a:min(a + W, T - 1) + 1]
        a2 = a + int(np.argmax(win))
        att.append(a2)
        wins.append(win)
        bases.append(a)
        if len(win) >= 2:
            top = np.sort(win)
            amargins.append(top[-1] - top[-2])
        forbid = ignore_eos or f < 4
        force = forced[0][f] if forced is not None and f < len(forced[0]) else None
        if cfg_scale is None and force is None and not bf16:
            codes, mg, _ = M.lt_sample_all(hs[0], forbid_eos=forbid)
        elif cfg_scale is not None and force is None and not bf16 and not partner_is_cond:
            codes, _, mg = mc.lt_sample_pair(M, hs[0], hs[1], cfg_scale, forbid_eos=forbid)
        else:
            pair = hs if not partner_is_cond else [hs[0], hs[0]]
            codes, _, mg = _lt_pick(M, pair, cfg_scale, forbid, force, bf16, P)
        margins.append(mg)
        if forced is None and any(c == mi.AUDIO_EOS for c in codes):
            break
        frames.append(codes)
        if f + 1 >= max_steps:
            break
        prev, pos = codes, pos + 1  # the slot advances
        a = a2
        if forced is not None:
            prev = [int(c) for c in forced[0][f]]
            if forced[1] is not None:
                a = int(forced[1][f])
        t = np.arange(T)
        inside = (t >= max(a - 1, 0)) & (t <= min(a + W, T - 1))
        lp = np.where(inside | (f + 1 < start), 0.0, Lp)
    out = {"codes": np.array(frames, np.int32).reshape(-1, 8), "hidden": np.array(hidden), "att": np.array(att, np.int32),
           "margins": np.array(margins), "amargins": np.array(amargins), "avg": wins, "base": np.array(bases, np.int32)}
    if cfg_scale is not None:
        out["hidden_uncond"] = np.array(hidden_u)
    return out


# ---------------------------------------------------------------- the f32 cases
# Every case: the 2-layer small model, speaker 0, epsilon 0.1, greedy with EOS ignored, traced.
# A reference is one (T, W, start_step, layers, steps, token seed); the XA forms share it.
FORMS = ("reassoc", "direct")

# Text edges (tests/text_edges.py: what each length is the edge of), 8 frames, all layers, from
# frame 0: (T, W, seed). At W = 0 the window is the single position a, so `att` is 0 on every
# frame of any run (point 3 of the header comment) and only the codes can differ from the
# prior-off run; lp is L from key 1 on, which is what these lengths are listed for. At T = 1023
# and 1024 the attention over a thousand random keys is flat and few seeds let a 6-wide window
# move `att` with both margins held: 100, 102 and 103 are the first of 0..199 that do.
EDGE_STEPS = 8
EDGES = [(3, 0, 0), (4, 0, 0), (5, 0, 0), (9, 0, 0), (15, 1, 13), (16, 1, 3), (17, 1, 3), (63, 5, 3), (64, 5, 1), (65, 5, 3),
         (100, 5, 6), (127, 5, 1), (128, 5, 1), (129, 5, 1), (150, 5, 1), (160, 5, 7), (161, 5, 7), (255, 5, 0), (256, 5, 0),
         (257, 5, 0), (1023, 5, 103), (1024, 5, 103)]

# Window edges of xa_align_kernel and start_step, 12 frames, all layers:
# (name, T, XA form, W, start_step, steps, seed)
WINDOWS = [
    ("a_reaches_the_end", 12, "reassoc", 5, 0, 12, 17),       # a arrives at T - 1 and stays
    ("wide_window_64", 200, "reassoc", 64, 0, 12, 11),         # a winner 64 past a: wave 1
    ("wide_window_100", 200, "reassoc", 100, 0, 12, 2),      # winners in waves 1+
    ("strided_window", 1024, "direct", 300, 0, 12, 8),     # threads with two positions
    ("window_wider_than_the_text", 150, "reassoc", 300, 0, 12, 0),  # hi clipped at T - 1
    ("start_0", 70, "reassoc", 5, 0, 12, 1),
    ("start_3", 70, "reassoc", 5, 3, 12, 1),
    ("start_past_the_run", 70, "reassoc", 5, 20, 12, 0),  # lp zero throughout
]
STRIDED_WINNER_PAST_256 = True  # seed 8: the frame-2 winner lies 297 past a (a thread's second position wins)

_refs = {}


def _frozen(r):
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


def reference(M, ma, T, W, start, layers, steps, seed):
    """(the restatement with the prior, the prior-off run) of an f32 case, each computed once"""
    key = (id(M), T, W, start, layers, steps, seed)
    if key not in _refs:
        tok = tokens(ma, T, seed)
        _refs[key] = (_frozen(restate(M, tok, 0, steps, EPS, W, start, layers, ignore_eos=True)),
                      _frozen(restate(M, tok, 0, steps, None, W, start, layers, ignore_eos=True)), M)
    return _refs[key][:2]


# Guidance with the prior: scale 2.5, prior (0.1, 5, 0, 0), 8 frames; T -> token seed
CFG_SCALE, CFG_STEPS = 2.5, 8
CFG_SEEDS = {70: 2, 5: 0, 33: 2}


def cfg_reference(M, ma, T):
    key = (id(M), "cfg", T)
    if key not in _refs:
        _refs[key] = (_frozen(restate(M, tokens(ma, T, CFG_SEEDS[T]), 0, CFG_STEPS, EPS, 5, cfg_scale=CFG_SCALE, ignore_eos=True)), M)
    return _refs[key][0]


# bf16 (the oracle's weight mode 1), prior (0.1, W, 0, 0), 12 frames: (T, XA form, W, seed)
BF16_STEPS = 12
BF16_CASES = [(70, "reassoc", 5, 0), (200, "direct", 5, 0)]
BF16_MAX_TIES = 2  # 8 of 320 decisions, test_decode_gpu.py's share, of 96
# the bf16 restatement against oracle.Model(...).set_weight_mode(1), prior off, teacher forced:
# hidden states within 7.0e-5 (T = 70) and 4.6e-3 (T = 200: the oracle keeps f32 intermediates, so
# an activation's bf16 rounding can fall the other way) -- test_attn_prior_cpu.py; the bound is a
# fifth of BF16_HIDDEN_TOL = 3e-2
BF16_RESTATE_SPREAD = 6e-3
# the largest shift of any window avg entry between the bf16 restatement accumulating its
# projections in f32 and in f64 over BF16_CASES (measured 2.23e-6 at T = 70, 4.02e-6 at T = 200;
# recorded rounded up), and the bar under which a bf16 alignment vote counts as a near-tie: twice that
ALIGN_SHIFT_BF16 = 4.1e-6
ALIGN_TIE_BF16 = 2 * ALIGN_SHIFT_BF16


# Exact ties across waves: the small model with every cross_attention.kv_net zeroed (K = V = 0:
# every XA score is exactly 0, every softmax uniform), so all window positions hold the same
# avg, bit for bit, and "the first index of the maximum" is a itself on every frame. A window of
# 200 positions spans xa_align_kernel's four waves, one of 1024 gives every thread four
# positions: (T, XA form, W)
TIED_MODEL_FILE = "magpie_small_l2e1_k32_xkv0.gguf"
TIED_CASES = [(200, "reassoc", 199), (1024, "direct", 1023)]
TIED_STEPS, TIED_SEED = 8, 4


def tied_model(small_model):
    """written into $MAGPIE_CACHE beside the small model it is made from"""
    from gguf_raw import GgufRaw
    path = os.path.join(os.path.dirname(small_model), TIED_MODEL_FILE)
    if not os.path.exists(path):
        g = GgufRaw(small_model)
        buf = bytearray(g.buf)
        zeroed = 0
        for name, (ne, typ, off) in g.tensors.items():
            if name.endswith("cross_attention.kv_net.weight"):
                assert typ == 0
                n = 4 * int(np.prod(ne))
                buf[g.data + off:g.data + off + n] = bytes(n)
                zeroed += 1
        assert zeroed >= 1
        tmp = f"{path}.tmp{os.getpid()}"
        with open(tmp, "wb") as f:
            f.write(buf)
        os.replace(tmp, path)
    return path
