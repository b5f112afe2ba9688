#!/usr/bin/env python3
"""Classifier-free guidance restated in numpy f64 on the independent restatement of the
decode path (tests/golden/make_indep.py: Magpie), and the fixture it produces,
tests/golden/cfg_small.npz (tests/test_cfg_cpu.py keeps it honest, tests/test_cfg_gpu.py
holds the HIP path to it).

*** TEST INFRASTRUCTURE (build side only). ***

The semantics (include/magpie_hip.h, mp_hip_set_cfg), for one utterance and scale s:
  conditional branch    exactly Magpie.synthesize's decode of the utterance
  unconditional branch  the same decoder without text and speaker context: XA K = V = 0 over
                        the utterance's T text rows (an all-zero encoder output through the
                        bias-free kv_net), so every layer's cross-attention adds a zero vector;
                        the 110 context rows are decoder.position_embeddings[0..109] alone; its
                        own self-attention cache; its input frames are the conditional branch's
  every code            codebook cb of a frame is picked once, from
                        mixed = s * cond + (1 - s) * uncond over the 2024 logits, with the plain
                        decode's mask, first-max argmax, top-k draw and EOS rule; the picked code
                        is appended to both branches' LT sequences and feeds both branches' next
                        frame embedding
A greedy decision's margin is the top-1 / top-2 gap of the masked `mixed`; a sampled one's is
min(that gap, distance of u to the chosen interval), as orc_synthesize_ex defines it (the draw
from oracle.draw_u, the pick from oracle.sample_top_k on the f32-cast masked `mixed`).

Every stored case's smallest margin is asserted >= MIN_MARGIN = 1e-3 = 5 x parity.TIE_EPS: no
decision of the fixture is a near-tie, and the GPU test may demand every frame.

usage: python tests/golden/make_cfg.py   (writes tests/golden/cfg_small.npz)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "magpie-tts.cpp_amd"))

from make_indep import AUDIO_BOS, AUDIO_EOS, CTX_FRAMES, D, XA_D, Magpie, layer_norm  # noqa: E402

MIN_MARGIN = 1e-3

# (token seed, T, speaker, max_steps, scale, sampling or None)
# sampling = (temperature, top_k, draw seed, stream)
CASES = [
    (11, 12, 0, 16, 2.5, None),
    (13, 33, 3, 12, -0.5, None),
    (21, 20, 2, 5, 2.5, (0.7, 80, 539, 0)),  # 40 draws, each >= 1e-3 from its interval's ends: 1 seed in ~500
]


def _forbidden(forbid_eos):
    return [AUDIO_BOS] + list(range(AUDIO_BOS + 2, AUDIO_BOS + 8)) + ([AUDIO_EOS] if forbid_eos else [])


def lt_sample_pair(m, hidden_c, hidden_u, scale, forbid_eos, draw=None):
    """magpie_local_transformer_sample_all for a guided pair: (codes, argmax, margins).
    draw: None (greedy) or (temperature, top_k, cb -> u)."""
    seq_c = [m.lt_in_w @ hidden_c + m.lt_in_b]
    seq_u = [m.lt_in_w @ hidden_u + m.lt_in_b]
    codes, amax, margins = [], [], []
    forbidden = _forbidden(forbid_eos)
    for cb in range(8):
        lc = m.lt_out_w[cb] @ m.lt_layer(np.array(seq_c))[-1] + m.lt_out_b[cb]
        lu = m.lt_out_w[cb] @ m.lt_layer(np.array(seq_u))[-1] + m.lt_out_b[cb]
        mixed = scale * lc + (1.0 - scale) * lu
        mixed[forbidden] = -np.inf
        am = int(np.argmax(mixed))  # first maximal index
        top2 = np.sort(mixed)[-2:]
        mg = float(top2[1] - top2[0])
        code = am
        if draw is not None:
            from oracle import oracle as orc
            temperature, top_k, u_of = draw
            code, sm = orc.sample_top_k(mixed.astype(np.float32), temperature, top_k, u_of(cb))
            mg = min(mg, float(sm))
        codes.append(int(code))
        amax.append(am)
        margins.append(mg)
        if cb < 7:
            nxt = m.lt_in_w @ m.audio_emb[cb][code] + m.lt_in_b
            seq_c.append(nxt)
            seq_u.append(nxt)
    return codes, amax, margins


def synthesize_cfg(m, tokens, speaker, max_steps, scale, sampling=None, give_up_below=None):
    """Magpie.synthesize (graph reuse) for a guided utterance: codes, margins and both
    branches' hidden traces (BOS first). give_up_below: return None at the first frame with
    a smaller margin (a seed search abandons the candidate)."""
    tokens = np.asarray(tokens)
    T = len(tokens)
    enc = m.encode(tokens)
    xk, xv = [], []
    for L in m.dec:
        kv = layer_norm(enc, L["lnm"]) @ L["xkv"].T
        xk.append(kv[:, :XA_D])
        xv.append(kv[:, XA_D:])
    zk = [np.zeros((T, XA_D)) for _ in m.dec]  # the unconditional branch's XA tables
    zv = [np.zeros((T, XA_D)) for _ in m.dec]
    max_seq = CTX_FRAMES + max_steps + 16
    cache_c = [(np.zeros((max_seq, D)), np.zeros((max_seq, D))) for _ in range(m.n_dec)]
    cache_u = [(np.zeros((max_seq, D)), np.zeros((max_seq, D))) for _ in range(m.n_dec)]
    xc = m.baked[speaker].reshape(CTX_FRAMES, D) + m.dec_pos[:CTX_FRAMES]
    xu = m.dec_pos[:CTX_FRAMES].copy()
    for l in range(m.n_dec):
        xc = m.dec_layer(l, xc, 0, cache_c, xk, xv)
        xu = m.dec_layer(l, xu, 0, cache_u, zk, zv)
    pos = CTX_FRAMES
    frames, hid_c, hid_u, margins = [], [], [], []
    prev = [AUDIO_BOS] * 8
    for step in range(-1, max_steps):
        if step >= 0:
            draw = None
            if sampling is not None:
                from oracle import oracle as orc
                temperature, top_k, seed, stream = sampling
                draw = (temperature, top_k, lambda cb, s=step: orc.draw_u(seed, stream, s, cb))
            codes, amax, mg = lt_sample_pair(m, hid_c[-1], hid_u[-1], scale, forbid_eos=step < 4, draw=draw)
            margins.append(mg)
            if give_up_below is not None and min(mg) < give_up_below:
                return None
            # EOS if any codebook's sampled code or argmax is EOS (magpie.cpp:4340-4348)
            if any(c == AUDIO_EOS for c in codes) or any(a == AUDIO_EOS for a in amax):
                break
            frames.append(codes)
            if step + 1 >= max_steps:
                break
            prev = codes
        x = m.frame_embedding(prev) + m.dec_pos[pos]
        xc, xu = x[None, :].copy(), x[None, :].copy()
        for l in range(m.n_dec):
            xc = m.dec_layer(l, xc, pos, cache_c, xk, xv)
            xu = m.dec_layer(l, xu, pos, cache_u, zk, zv)
        hid_c.append(layer_norm(xc[0], m.dec_norm))
        hid_u.append(layer_norm(xu[0], m.dec_norm))
        pos += 1
    return {"codes": np.array(frames, np.int32).reshape(-1, 8), "margins": np.array(margins).reshape(-1, 8),
            "hidden": np.array(hid_c), "hidden_uncond": np.array(hid_u)}


def small_model_path():
    import magpie_amd as ma
    cache = os.environ.get("MAGPIE_CACHE", "/tmp/magpie_amd_cache")
    os.makedirs(cache, exist_ok=True)
    return ma.synth_gguf(os.path.join(cache, "magpie_small_l2e1_k32.gguf"), dec_layers=2, enc_layers=1,
                         lt_head_scale=ma.DECISIVE)


def main():
    import magpie_amd as ma
    m = Magpie(small_model_path())
    out = {}
    for i, (seed, T, spk, steps, scale, sampling) in enumerate(CASES):
        tok = ma.synthetic_tokens(T, seed=seed)
        r = synthesize_cfg(m, tok, spk, steps, scale, sampling)
        plain = m.synthesize(tok, spk, steps)["codes"]
        n = min(len(plain), len(r["codes"]))
        differ = float((plain[:n] != r["codes"][:n]).mean()) if n else 0.0
        mn = float(r["margins"].min())
        print(f"case {i}: T={T} speaker={spk} scale={scale} sampling={sampling}: {len(r['codes'])} frames, "
              f"min margin {mn:.2e}, {100 * differ:.0f} % of decisions differ from the plain run")
        assert mn >= MIN_MARGIN, f"case {i}: min margin {mn:.3g} < {MIN_MARGIN}: choose another seed"
        assert len(r["codes"]) >= min(8, steps)
        out[f"g{i}_tokens"] = tok
        out[f"g{i}_meta"] = np.array([spk, steps], np.int32)
        out[f"g{i}_scale"] = np.float64(scale)
        out[f"g{i}_sampling"] = np.array(sampling if sampling is not None else (0.0, 0, 0, 0), np.float64)
        out[f"g{i}_codes"] = r["codes"]
        out[f"g{i}_margins"] = r["margins"]
        out[f"g{i}_hidden"] = r["hidden"].astype(np.float32)
        out[f"g{i}_hidden_uncond"] = r["hidden_uncond"].astype(np.float32)
    np.savez_compressed(os.path.join(HERE, "cfg_small.npz"), **out)


if __name__ == "__main__":
    main()
