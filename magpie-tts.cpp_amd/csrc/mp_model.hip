// Weight loading of the MI355X decode path (mp_model.hpp): a GGUF's tensors into one f32
// arena, the weight mode's repacked copies, and the LT tables built at load time.
// Tensor names and mapping: create_tensors (magpie.cpp:572-672).
#include "mp_model.hpp"

#include <algorithm>
#include <cstring>

#include "mp_device.hpp"
#include "mp_gguf.hpp"
#include "mp_ops.hpp"
#include "mp_prefill_api.hpp"

namespace mp {
namespace {

#define HIPCHK(expr) MP_HIPCHK_TO(err, expr)

int fail(std::string &err, int code, const std::string &msg) {
    err = msg;
    return code;
}

// bf16 weight mode: the f32 weights rounded to bf16 fragments; F16 mode (an F16
// file): its f16 values (widened exactly at load) repacked as f16 fragments.
int pack_weights(Model &m, bool f16, hipStream_t stream, std::string &err) {
    const int L = m.dec_layers;
    const size_t per_layer = pk_elems(2304, 768) + pk_elems(768, 768) + pk_elems(3072, 768) + pk_elems(768, 3072);
    const size_t lt = pk_elems(768, 256) + pk_elems(256, 256) + pk_elems(1024, 256) + pk_elems(256, 1024) +
                      8 * pk_elems(2024, 256) + (f16 ? pk_elems(256, 768) : 0);
    unsigned short *cur = nullptr;  // one block, the tensors back to back
    HIPCHK(m.mem.bytes(&cur, (per_layer * L + lt) * 2));
    auto pack = [&](const float *W, int N, int K) -> const unsigned short * {
        unsigned short *dst = cur;
        cur += pk_elems(N, K);
        return pack_b16(W, N, K, dst, stream, f16) == hipSuccess ? dst : nullptr;
    };
    m.pk_qkv.assign(L, nullptr); m.pk_o.assign(L, nullptr); m.pk_ff1.assign(L, nullptr); m.pk_ff2.assign(L, nullptr);
    for (int l = 0; l < L; ++l) {
        m.pk_qkv[l] = pack(m.dec[l].qkv, 2304, 768);
        m.pk_o[l] = pack(m.dec[l].o, 768, 768);
        m.pk_ff1[l] = pack(m.dec[l].ff1, 3072, 768);
        m.pk_ff2[l] = pack(m.dec[l].ff2, 768, 3072);
        if (!m.pk_qkv[l] || !m.pk_o[l] || !m.pk_ff1[l] || !m.pk_ff2[l]) return fail(err, MP_ERR_HIP, "bf16 pack failed");
    }
    m.pk_lt_qkv = pack(m.lt_qkv, 768, 256);
    m.pk_lt_o = pack(m.lt_o, 256, 256);
    m.pk_lt_ff1 = pack(m.lt_ff1, 1024, 256);
    m.pk_lt_ff2 = pack(m.lt_ff2, 256, 1024);
    m.pk_lt_out = cur;
    for (int c = 0; c < 8; ++c)
        if (!pack(m.lt_out_w + (size_t)c * 2024 * 256, 2024, 256)) return fail(err, MP_ERR_HIP, "bf16 pack failed");
    if (!m.pk_lt_qkv || !m.pk_lt_o || !m.pk_lt_ff1 || !m.pk_lt_ff2) return fail(err, MP_ERR_HIP, "bf16 pack failed");
    m.pk_lt_in = f16 ? pack(m.lt_in_w, 256, 768) : nullptr;
    if (f16 && !m.pk_lt_in) return fail(err, MP_ERR_HIP, "f16 pack failed");
    HIPCHK(hipStreamSynchronize(stream));
    return MP_OK;
}

int load_tensors(Model &m, const Gguf &g, std::string &err) {
    // read_hparams (magpie.cpp:73-121): the reader's keys, struct defaults otherwise
    if (g.get_u32("magpie.d_model", 768) != 768 || g.get_u32("magpie.d_ffn", 3072) != 3072 ||
        g.get_u32("magpie.d_head", 64) != 64 || g.get_u32("magpie.dec_sa_heads", 12) != 12 ||
        g.get_u32("magpie.dec_xa_heads", 1) != 1 || g.get_u32("magpie.dec_xa_d_head", 128) != 128 ||
        g.get_u32("magpie.lt_dim", 256) != 256 || g.get_u32("magpie.lt_ffn_dim", 1024) != 1024 ||
        g.get_u32("magpie.num_codebooks", 8) != 8 || g.get_u32("magpie.vocab_per_cb", 2024) != 2024 ||
        g.get_u32("magpie.context_frames", 110) != 110 || g.get_u32("magpie.enc_heads", 12) != 12 ||
        g.get_u32("magpie.enc_kernel", 3) != 3 || g.get_u32("magpie.dec_kernel", 1) != 1 ||
        g.get_u32("magpie.lt_layers", 1) != 1 || g.get_u32("magpie.lt_heads", 1) != 1)
        return fail(err, MP_ERR_UNSUPPORTED, "model dimensions differ from Magpie-357M (kernels are specialised)");
    m.enc_layers = (int)g.get_u32("magpie.enc_layers", 6);
    m.dec_layers = (int)g.get_u32("magpie.dec_layers", 12);
    m.n_spk = (int)g.get_u32("magpie.num_speakers", 5);
    m.text_vocab = (int)g.get_u32("magpie.text_vocab_size", 2380);
    m.audio_bos = (int)g.get_u32("magpie.audio_bos_id", 2016);
    m.audio_eos = (int)g.get_u32("magpie.audio_eos_id", 2017);
    // the kernels' forbidden-token mask is the range [bos, bos + 7] minus eos, which is
    // the reference's explicit list (magpie.cpp:1133-1145) only when eos == bos + 1
    if (m.audio_eos != m.audio_bos + 1 || m.audio_bos < 0 || m.audio_bos + 8 > VCB)
        return fail(err, MP_ERR_UNSUPPORTED, "audio_eos_id must be audio_bos_id + 1 (forbidden-token layout)");
    m.max_dec_steps = (int)g.get_u32("magpie.max_dec_steps", 500);
    m.eps = (float)g.get_f32("magpie.eps", 1e-5);
    if (m.enc_layers < 1 || m.dec_layers < 1 || m.enc_layers > 64 || m.dec_layers > 64)
        return fail(err, MP_ERR_FORMAT, "bad layer counts");

    struct Want { std::string name; int64_t n; const float **dst; };
    std::vector<Want> want;
    auto need = [&](const std::string &name, int64_t n, const float **dst) { want.push_back({name, n, dst}); };
    const int64_t D = 768;
    need("text_embedding.weight", (int64_t)m.text_vocab * D, &m.text_emb);
    need("encoder.position_embeddings.weight", -1, &m.enc_pos);
    m.enc.assign(m.enc_layers, EncLayerW{});
    for (int l = 0; l < m.enc_layers; ++l) {
        const std::string p = "encoder.layers." + std::to_string(l) + ".";
        EncLayerW &L = m.enc[l];
        need(p + "norm_self.weight", D, &L.norm_self);
        need(p + "self_attention.qkv_net.weight", 3 * D * D, &L.qkv);
        need(p + "self_attention.o_net.weight", D * D, &L.o);
        need(p + "norm_pos_ff.weight", D, &L.norm_ff);
        need(p + "pos_ff.proj.conv.weight", 3072 * D * 3, &L.ff1);
        need(p + "pos_ff.o_net.conv.weight", 3072 * D * 3, &L.ff2);
    }
    need("encoder.norm_out.weight", D, &m.enc_norm_out);
    need("decoder.position_embeddings.weight", -1, &m.dec_pos);
    m.dec.assign(m.dec_layers, DecLayerW{});
    for (int l = 0; l < m.dec_layers; ++l) {
        const std::string p = "decoder.layers." + std::to_string(l) + ".";
        DecLayerW &L = m.dec[l];
        need(p + "norm_self.weight", D, &L.norm_self);
        need(p + "self_attention.qkv_net.weight", 3 * D * D, &L.qkv);
        need(p + "self_attention.o_net.weight", D * D, &L.o);
        need(p + "norm_xattn_query.weight", D, &L.norm_xq);
        need(p + "cross_attention.q_net.weight", 128 * D, &L.xq);
        need(p + "cross_attention.kv_net.weight", 256 * D, &L.xkv);
        need(p + "cross_attention.o_net.weight", D * 128, &L.xo);
        need(p + "norm_xattn_memory.weight", D, &L.norm_xmem);
        need(p + "norm_pos_ff.weight", D, &L.norm_ff);
        need(p + "pos_ff.proj.conv.weight", 3072 * D, &L.ff1);
        need(p + "pos_ff.o_net.conv.weight", 3072 * D, &L.ff2);
    }
    need("decoder.norm_out.weight", D, &m.dec_norm_out);
    need("baked_context_embedding.weight", -1, &m.baked);
    need("local_transformer_in_projection.weight", 256 * D, &m.lt_in_w);
    need("local_transformer_in_projection.bias", 256, &m.lt_in_b);
    need("local_transformer.position_embeddings.weight", -1, &m.lt_pos);
    need("local_transformer.layers.0.norm_self.weight", 256, &m.lt_norm_self);
    need("local_transformer.layers.0.self_attention.qkv_net.weight", 768 * 256, &m.lt_qkv);
    need("local_transformer.layers.0.self_attention.o_net.weight", 256 * 256, &m.lt_o);
    need("local_transformer.layers.0.norm_pos_ff.weight", 256, &m.lt_norm_ff);
    need("local_transformer.layers.0.pos_ff.proj.conv.weight", 1024 * 256, &m.lt_ff1);
    need("local_transformer.layers.0.pos_ff.o_net.conv.weight", 1024 * 256, &m.lt_ff2);
    // per-codebook tensors become one contiguous [8][...] array each so a kernel
    // can index them by a codebook read from device memory
    std::vector<std::string> grouped[3];
    for (int c = 0; c < 8; ++c) {
        grouped[0].push_back("audio_embeddings." + std::to_string(c) + ".weight");
        grouped[1].push_back("local_transformer_out_projections." + std::to_string(c) + ".weight");
        grouped[2].push_back("local_transformer_out_projections." + std::to_string(c) + ".bias");
    }
    const int64_t gsize[3] = {2024 * D, 2024 * 256, 2024};
    const float **gdst[3] = {&m.audio_emb, &m.lt_out_w, &m.lt_out_b};

    // size the arena
    auto align_up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    size_t total = 0;
    for (auto &w : want) {
        const GgufTensor *t = g.find(w.name);
        if (!t) return fail(err, MP_ERR_FORMAT, "missing tensor " + w.name);
        if (w.n >= 0 && t->nelements() != w.n) return fail(err, MP_ERR_FORMAT, "unexpected shape for " + w.name);
        total += align_up((size_t)t->nelements() * 4);
    }
    for (int k = 0; k < 3; ++k)
        for (auto &nm : grouped[k]) {
            const GgufTensor *t = g.find(nm);
            if (!t) return fail(err, MP_ERR_FORMAT, "missing tensor " + nm);
            if (t->nelements() != gsize[k]) return fail(err, MP_ERR_FORMAT, "unexpected shape for " + nm);
        }
    for (int k = 0; k < 3; ++k) total += align_up((size_t)gsize[k] * 8 * 4);
    {
        const GgufTensor *dp = g.find("decoder.position_embeddings.weight");
        const GgufTensor *bk = g.find("baked_context_embedding.weight");
        const GgufTensor *ep = g.find("encoder.position_embeddings.weight");
        const GgufTensor *lp = g.find("local_transformer.position_embeddings.weight");
        if (dp->ne[0] != D || bk->ne[0] != 110 * D || ep->ne[0] != D || lp->ne[0] != 256 || lp->ne[1] < 8)
            return fail(err, MP_ERR_FORMAT, "unexpected embedding table shapes");
        m.dec_pos_rows = (int)dp->ne[1];
        m.n_spk = (int)std::min<int64_t>(m.n_spk, bk->ne[1]);
    }
    char *arena = nullptr;
    HIPCHK(m.mem.bytes(&arena, total));
    m.arena_bytes = total;
    std::vector<float> host;
    size_t off = 0;
    std::vector<float> tmp;
    auto upload = [&](const GgufTensor *t, float *dst) -> int {
        host.resize((size_t)t->nelements());
        if (!g.to_f32(*t, host.data())) return fail(err, MP_ERR_FORMAT, "unsupported tensor type in " + t->name);
        if (t->n_dims == 3 && t->ne[0] == 3 && t->name.rfind("encoder.layers.", 0) == 0) {
            // causal k=3 conv weight [out][in][k] -> tap-major [out][k][in] (mp_prefill.hip loader)
            const int64_t K = 3, Cin = t->ne[1], Co = t->ne[2];
            tmp.resize(host.size());
            for (int64_t o = 0; o < Co; ++o)
                for (int64_t i = 0; i < Cin; ++i)
                    for (int64_t k = 0; k < K; ++k) tmp[(o * K + k) * Cin + i] = host[(o * Cin + i) * K + k];
            host.swap(tmp);
        }
        HIPCHK(hipMemcpy(dst, host.data(), host.size() * 4, hipMemcpyHostToDevice));
        return MP_OK;
    };
    for (auto &w : want) {
        const GgufTensor *t = g.find(w.name);
        float *dst = (float *)(arena + off);
        if (int rc = upload(t, dst)) return rc;
        *w.dst = dst;
        off += align_up((size_t)t->nelements() * 4);
    }
    for (int k = 0; k < 3; ++k) {
        float *base = (float *)(arena + off);
        for (int c = 0; c < 8; ++c)
            if (int rc = upload(g.find(grouped[k][c]), base + (size_t)c * gsize[k])) return rc;
        *gdst[k] = base;
        off += align_up((size_t)gsize[k] * 8 * 4);
    }
    // W_q^T per decoder layer (for the per-utterance K' = K W_q of the fused XA), one
    // allocation, layer l at l * 768 * 128 (the batched K' GEMM strides over it)
    m.xq_t.assign(m.dec_layers, nullptr);
    {
        std::vector<float> wq((size_t)128 * 768), wt((size_t)768 * 128);
        float *all = nullptr;
        HIPCHK(m.mem.bytes(&all, wt.size() * 4 * m.dec_layers));
        for (int l = 0; l < m.dec_layers; ++l) {
            HIPCHK(hipMemcpy(wq.data(), m.dec[l].xq, wq.size() * 4, hipMemcpyDeviceToHost));
            for (int j = 0; j < 128; ++j)
                for (int n = 0; n < 768; ++n) wt[(size_t)n * 128 + j] = wq[(size_t)j * 768 + n];
            m.xq_t[l] = all + (size_t)l * wt.size();
            HIPCHK(hipMemcpy(m.xq_t[l], wt.data(), wt.size() * 4, hipMemcpyHostToDevice));
        }
    }
    return MP_OK;
}

// f32 -> bf16 bits, round to nearest even (ggml_compute_fp32_to_bf16; finite weights)
unsigned short bf16_bits(float x) {
    unsigned u;
    memcpy(&u, &x, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((u >> 16) | 64);
    return (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

int build_vo_tables(Model &m, hipStream_t stream, std::string &err) {
    const size_t R = (size_t)7 * 2024;
    HIPCHK(m.mem.bytes(&m.lt_votab, R * 256 * 4));
    GemmP gp{};
    gp.A = m.lt_qkvtab + 512; gp.lda = 768; gp.W = m.lt_o; gp.C = m.lt_votab; gp.ldc = 256;
    gp.M = (int)R; gp.N = 256; gp.K = 256; gp.rows_per_utt = (int)R;
    HIPCHK(pre_gemm(gp, GE_STORE, stream));
    std::vector<float> qkv((size_t)768 * 256), o((size_t)256 * 256), kvo((size_t)512 * 256);
    HIPCHK(hipMemcpy(qkv.data(), m.lt_qkv, qkv.size() * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(o.data(), m.lt_o, o.size() * 4, hipMemcpyDeviceToHost));
    memcpy(kvo.data(), qkv.data() + (size_t)256 * 256, (size_t)256 * 256 * 4);  // W_k rows
    for (int n = 0; n < 256; ++n)
        for (int k = 0; k < 256; ++k) {
            double acc = 0.0;
            for (int j = 0; j < 256; ++j) acc += (double)o[(size_t)n * 256 + j] * qkv[(size_t)(512 + j) * 256 + k];
            kvo[(size_t)(256 + n) * 256 + k] = (float)acc;
        }
    HIPCHK(m.mem.bytes(&m.lt_kvo, kvo.size() * 4));
    HIPCHK(hipMemcpy(m.lt_kvo, kvo.data(), kvo.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(hipStreamSynchronize(stream));
    return MP_OK;
}

// P[c][v] = in_proj(audio_emb[c][v]) + b: the LT's per-codebook re-embedding
// (magpie.cpp:1274-1313) depends only on (c, v) -> one GEMM at load time (with
// ggml's Q8_0 arithmetic when in_proj is a Q8_0 tensor in Q8 mode).
int build_ptab(Model &m, hipStream_t stream, std::string &err) {
    const bool f16 = m.weight_mode == MP_WEIGHTS_F16;
    HIPCHK(m.mem.bytes(&m.lt_ptab, (size_t)8 * 2024 * 256 * 4));
    GemmP gp{};
    gp.A = m.audio_emb; gp.lda = 768; gp.W = m.lt_in_w; gp.Wq = m.lt_in8.q; gp.Wd = m.lt_in8.d; gp.bias = m.lt_in_b;
    gp.C = m.lt_ptab; gp.ldc = 256; gp.M = 8 * 2024; gp.N = 256; gp.K = 768; gp.rows_per_utt = 8 * 2024;
    gp.xround = f16 ? 2 : 0;  // F16 in_proj: the embedding row rounded to f16
    HIPCHK(pre_gemm(gp, GE_STORE, stream));
    // LT q|k|v of position c+1 for every code v of codebook c < 7: the rows PRO_LTARG_ATTN
    // gathers instead of running the q|k|v GEMV per codebook. The projection uses the
    // weights the decode-time GEMV would: f32 (also in the bf16 mode, whose LT attention is
    // f32: lt_table_attn; an F16 file's weights are already f16 values), or Q8_0 with
    // activations quantised per block.
    const size_t R = (size_t)7 * 2024;
    HIPCHK(m.mem.bytes(&m.lt_qkvtab, R * 768 * 4));
    {
        DevBlocks scratch;  // released before the layouts below are allocated
        float *rows = nullptr;
        HIPCHK(scratch.bytes(&rows, R * 256 * 4));
        HIPCHK(pre_lt_tab_rows(m.lt_ptab, m.lt_pos, m.lt_norm_self, m.eps, rows, f16 ? 2 : 0, stream));
        gp = GemmP{};
        gp.A = rows; gp.lda = 256; gp.W = m.lt_qkv; gp.Wq = m.lt_qkv8.q; gp.Wd = m.lt_qkv8.d;
        gp.C = m.lt_qkvtab; gp.ldc = 768; gp.M = (int)R; gp.N = 768; gp.K = 256; gp.rows_per_utt = (int)R;
        const hipError_t ge = pre_gemm(gp, GE_STORE, stream);
        const hipError_t se = hipStreamSynchronize(stream);  // rows is read until here, launched or not
        HIPCHK(ge);
        HIPCHK(se);
    }
    // the f32 FFN-down weights [256][1024] slice-major [P][256][1024 / P]
    auto ff2_slices = [&](int P, float **dst) -> int {
        const int U = 1024 / P;
        std::vector<float> w2((size_t)256 * 1024), w2s(w2.size());
        HIPCHK(hipMemcpy(w2.data(), m.lt_ff2, w2.size() * 4, hipMemcpyDeviceToHost));
        for (int p = 0; p < P; ++p)
            for (int n = 0; n < 256; ++n)
                memcpy(&w2s[((size_t)p * 256 + n) * U], &w2[(size_t)n * 1024 + p * U], U * 4);
        HIPCHK(m.mem.bytes(dst, w2s.size() * 4));
        HIPCHK(hipMemcpy(*dst, w2s.data(), w2s.size() * 4, hipMemcpyHostToDevice));
        return MP_OK;
    };
    if (int rc = ff2_slices(LT_FFN_P, &m.lt_ff2s)) return rc;
    if (m.weight_mode == MP_WEIGHTS_BF16) {
        std::vector<float> w1((size_t)1024 * 256), w2((size_t)256 * 1024);
        HIPCHK(hipMemcpy(w1.data(), m.lt_ff1, w1.size() * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(w2.data(), m.lt_ff2, w2.size() * 4, hipMemcpyDeviceToHost));
        constexpr int U = 1024 / LTS_P;
        std::vector<unsigned short> h1(w1.size()), h2(w2.size());
        for (size_t i = 0; i < w1.size(); ++i) h1[i] = bf16_bits(w1[i]);
        for (int q = 0; q < LTS_P; ++q)
            for (int n = 0; n < 256; ++n)
                for (int u = 0; u < U; ++u) h2[((size_t)q * 256 + n) * U + u] = bf16_bits(w2[(size_t)n * 1024 + q * U + u]);
        HIPCHK(m.mem.bytes(&m.lt_ff1h, h1.size() * 2));
        HIPCHK(hipMemcpy(m.lt_ff1h, h1.data(), h1.size() * 2, hipMemcpyHostToDevice));
        HIPCHK(m.mem.bytes(&m.lt_ff2h, h2.size() * 2));
        HIPCHK(hipMemcpy(m.lt_ff2h, h2.data(), h2.size() * 2, hipMemcpyHostToDevice));
    }
    if (m.weight_mode == MP_WEIGHTS_Q8)
        if (int rc = ff2_slices(LTQ_P, &m.lt_ff2q)) return rc;
    return lt_table_attn(m) ? build_vo_tables(m, stream, err) : MP_OK;
}

// Weight mode MP_WEIGHTS_Q8: upload every block-quantised tensor the decode path
// uses (scripts/convert_magpie_to_gguf.py:155-176 decides which: attention,
// cross-attention and LT projections), repacked to int8 [N][K] + fp16 scales
// [N][K/32] (34 B per 32 weights). Q8_0 blocks are copied; Q4_0 blocks
// (convert_magpie_to_gguf.py:107-138: q in 0..15, byte j = q_j | q_{j+16} << 4) become
// the int8 values q - 8 with the same scale, so the Q8_0 kernels compute exactly
// ggml's vec_dot_q4_0_q8_0: the integer dot of (q - 8) with the Q8_0-quantised
// activation times d_w * d_a. F32 tensors keep the f32 path.
int load_q8(Model &m, const Gguf &g, std::string &err) {
    struct Item { const GgufTensor *t; QW *dst; int group; };
    // a Q4_0 tensor's decode fragments stream its nibbles (MAGPIE_Q4_AS_Q8=1: as int8 q - 8,
    // the same integers at 34 B per 32 weights; both compute the same bits)
    const bool q4_nib = env_int("MAGPIE_Q4_AS_Q8", 0) == 0;
    std::vector<Item> items;
    auto want = [&](const std::string &name, QW *dst) {
        const GgufTensor *t = g.find(name);
        if (t && (t->type == 8 || t->type == 2) && t->ne[0] % 32 == 0) items.push_back({t, dst, -1});
    };
    for (int l = 0; l < m.enc_layers; ++l) {
        const std::string p = "encoder.layers." + std::to_string(l) + ".self_attention.";
        want(p + "qkv_net.weight", &m.enc[l].qkv8);
        want(p + "o_net.weight", &m.enc[l].o8);
    }
    for (int l = 0; l < m.dec_layers; ++l) {
        const std::string p = "decoder.layers." + std::to_string(l) + ".";
        want(p + "self_attention.qkv_net.weight", &m.dec[l].qkv8);
        want(p + "self_attention.o_net.weight", &m.dec[l].o8);
        want(p + "cross_attention.q_net.weight", &m.dec[l].xq8);
        want(p + "cross_attention.kv_net.weight", &m.dec[l].xkv8);
        want(p + "cross_attention.o_net.weight", &m.dec[l].xo8);
    }
    want("local_transformer_in_projection.weight", &m.lt_in8);
    want("local_transformer.layers.0.self_attention.qkv_net.weight", &m.lt_qkv8);
    want("local_transformer.layers.0.self_attention.o_net.weight", &m.lt_o8);
    int nout = 0;
    for (int c = 0; c < 8; ++c) {
        const GgufTensor *t = g.find("local_transformer_out_projections." + std::to_string(c) + ".weight");
        if (t && (t->type == 8 || t->type == 2)) { items.push_back({t, &m.lt_out8, c}); ++nout; }
    }
    if (nout != 0 && nout != 8) return fail(err, MP_ERR_UNSUPPORTED, "mixed quantised/F32 LT output projections");
    if (items.empty()) return fail(err, MP_ERR_UNSUPPORTED, "Q8 weight mode needs a GGUF with Q8_0 or Q4_0 tensors");
    // the reassociated XA (K' = K W_q, V' = W_o V) is an f32 identity: with Q8_0
    // q_net / o_net the activations must be quantised where ggml quantises them
    for (int l = 0; l < m.dec_layers; ++l)
        if ((bool)m.dec[l].xq8 != (bool)m.dec[l].xo8)
            return fail(err, MP_ERR_UNSUPPORTED, "cross-attention q_net / o_net must both be Q8_0 or both F32");
    auto align_up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    size_t total = 0;
    for (auto &it : items) {
        const size_t n = (size_t)it.t->nelements();
        total += align_up(n) + align_up(n / 32 * 2);
        if (it.dst == &m.lt_o8) total += align_up(n);  // the transposed copy
    }
    char *cur = nullptr;
    HIPCHK(m.mem.bytes(&cur, total));
    std::vector<signed char> hq;
    std::vector<unsigned short> hd;
    signed char *out_q = nullptr;
    unsigned short *out_d = nullptr;
    const size_t out_n = (size_t)2024 * 256;
    for (auto &it : items) {
        const size_t n = (size_t)it.t->nelements();
        const uint8_t *src = g.data(*it.t);
        hq.resize(n);
        hd.resize(n / 32);
        for (size_t b = 0; b < n / 32; ++b) {
            if (it.t->type == 8) {
                memcpy(&hd[b], src + b * 34, 2);
                memcpy(&hq[b * 32], src + b * 34 + 2, 32);
            } else {  // Q4_0
                const uint8_t *blk = src + b * 18;
                memcpy(&hd[b], blk, 2);
                for (int j = 0; j < 16; ++j) {
                    hq[b * 32 + j] = (signed char)((blk[2 + j] & 0x0F) - 8);
                    hq[b * 32 + j + 16] = (signed char)((blk[2 + j] >> 4) - 8);
                }
            }
        }
        signed char *dq;
        unsigned short *dd;
        if (it.group < 0) {
            dq = (signed char *)cur; cur += align_up(n);
            dd = (unsigned short *)cur; cur += align_up(n / 32 * 2);
            it.dst->q = dq; it.dst->d = dd;
            it.dst->nib = q4_nib && it.t->type == 2;
        } else {  // the 8 LT heads as one [8][2024][256] array (indexed by a device codebook)
            if (n != out_n) return fail(err, MP_ERR_FORMAT, "unexpected LT output projection shape");
            if (!out_q) {
                out_q = (signed char *)cur; cur += align_up(8 * n);
                out_d = (unsigned short *)cur; cur += align_up(8 * (n / 32) * 2);
            }
            dq = out_q + (size_t)it.group * n;
            dd = out_d + (size_t)it.group * (n / 32);
            it.dst->q = out_q; it.dst->d = out_d;
            if (it.group == 0) it.dst->nib = q4_nib && it.t->type == 2;
            else if (it.dst->nib != (int)(q4_nib && it.t->type == 2))
                return fail(err, MP_ERR_UNSUPPORTED, "mixed Q4_0 / Q8_0 LT output projections");
        }
        HIPCHK(hipMemcpy(dq, hq.data(), n, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(dd, hd.data(), n / 32 * 2, hipMemcpyHostToDevice));
        if (it.dst == &m.lt_o8) {  // chunk i of row r at [i][r]: thread r's 16 loads coalesce across the wave
            if (n != (size_t)256 * 256) return fail(err, MP_ERR_FORMAT, "unexpected LT o_net shape");
            std::vector<signed char> ht(n);
            for (int r = 0; r < 256; ++r)
                for (int i = 0; i < 16; ++i) memcpy(&ht[((size_t)i * 256 + r) * 16], &hq[(size_t)r * 256 + i * 16], 16);
            signed char *dt = (signed char *)cur;
            cur += align_up(n);
            HIPCHK(hipMemcpy(dt, ht.data(), n, hipMemcpyHostToDevice));
            m.lt_o8t = dt;
        }
    }
    // the decode projections once more in int8 MFMA fragment order
    struct Dec { QW *w; int N, K, heads; };
    std::vector<Dec> dec;
    bool all = true;
    auto add = [&](QW &w, int N, int K, int heads) {
        if (w) dec.push_back({&w, N, K, heads});
        else all = false;
    };
    for (int l = 0; l < m.dec_layers; ++l) {
        add(m.dec[l].qkv8, 2304, 768, 1);
        add(m.dec[l].o8, 768, 768, 1);
        add(m.dec[l].xq8, 128, 768, 1);
        if (!m.dec[l].xo8) all = false;
    }
    add(m.lt_in8, 256, 768, 1);
    add(m.lt_qkv8, 768, 256, 1);
    add(m.lt_o8, 256, 256, 1);
    add(m.lt_out8, 2024, 256, 8);
    size_t ptotal = 0;
    auto frag_bytes = [&](const Dec &d) { return align_up(d.w->nib ? q4p_qbytes(d.N, d.K) : q8p_qbytes(d.N, d.K)); };
    for (auto &d : dec) ptotal += d.heads * (frag_bytes(d) + align_up(q8p_dbytes(d.N, d.K)));
    char *pc = nullptr;
    if (ptotal) HIPCHK(m.mem.bytes(&pc, ptotal));
    for (auto &d : dec) {
        const size_t qb = frag_bytes(d), db = align_up(q8p_dbytes(d.N, d.K));
        signed char *oq = (signed char *)pc;
        pc += d.heads * qb;
        unsigned short *od = (unsigned short *)pc;
        pc += d.heads * db;
        for (int h = 0; h < d.heads; ++h) {
            const signed char *hq = d.w->q + (size_t)h * d.N * d.K;
            // the scales (and, for Q8_0, the int8 fragments) in fragment order
            HIPCHK(pack_q8(hq, d.w->d + (size_t)h * d.N * (d.K / 32), d.N, d.K,
                           d.w->nib ? nullptr : (unsigned char *)oq + h * qb,
                           (unsigned short *)((char *)od + h * db), nullptr));
            if (d.w->nib) HIPCHK(pack_q4(hq, d.N, d.K, (unsigned char *)oq + h * qb, nullptr));
        }
        d.w->pq = oq;
        d.w->pd = od;
        d.w->head_q = qb;
    }
    HIPCHK(hipDeviceSynchronize());
    m.q8_all = all;
    return MP_OK;
}

}  // namespace

int load_model(const char *path, int weight_mode, hipStream_t stream, Model &m, std::string &err) {
    Gguf g;
    if (!g.open(path, err)) return MP_ERR_IO;
    // cheap header checks before any upload
    const GgufTensor *t = g.find("decoder.layers.0.self_attention.qkv_net.weight");
    if (weight_mode == MP_WEIGHTS_Q8 && (!t || (t->type != 8 && t->type != 2)))
        return fail(err, MP_ERR_UNSUPPORTED, "Q8 weight mode needs a GGUF with Q8_0 or Q4_0 tensors");
    // every tensor the F16 mode streams as f16 must be stored F16 (the converter's
    // pattern set, convert_magpie_to_gguf.py:155-176, 311-327)
    if (weight_mode == MP_WEIGHTS_F16)
        for (const auto &kv : g.tensors()) {
            const std::string &n = kv.first;
            const bool proj = n.find(".self_attention.") != std::string::npos ||
                              n.find(".pos_ff.") != std::string::npos ||
                              n.find("local_transformer_out_projections.") == 0 ||
                              n == "local_transformer_in_projection.weight";
            if (proj && n.size() > 7 && n.compare(n.size() - 7, 7, ".weight") == 0 && kv.second.type != 1)
                return fail(err, MP_ERR_UNSUPPORTED, "F16 weight mode needs a GGUF with F16 projections (" + n + ")");
        }
    if (int rc = load_tensors(m, g, err)) return rc;
    if (h16_mode(weight_mode)) {
        if (int rc = pack_weights(m, weight_mode == MP_WEIGHTS_F16, stream, err)) return rc;
    } else if (weight_mode == MP_WEIGHTS_Q8) {
        if (int rc = load_q8(m, g, err)) return rc;
    }
    m.weight_mode = weight_mode;  // the load-time LT tables depend on it
    return build_ptab(m, stream, err);
}

}  // namespace mp
