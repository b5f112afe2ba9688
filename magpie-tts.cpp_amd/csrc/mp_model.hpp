// The resident weights of one Magpie model: the GGUF's tensors in one f32 arena, the weight
// mode's repacked copies (16-bit MFMA fragments, Q8_0 / Q4_0 blocks and fragments) and the
// LT tables built at load time. A Model owns its device memory (`mem`); every pointer in it
// is a view into that. A model is loaded into a fresh Model and replaced whole, never patched.
#pragma once
#include <string>
#include <vector>

#include "../../include/magpie_hip.h"
#include "mp_own.hpp"

namespace mp {

// the 16-bit MFMA family serves the bf16 and F16 weight modes
inline bool h16_mode(int weight_mode) { return weight_mode == MP_WEIGHTS_BF16 || weight_mode == MP_WEIGHTS_F16; }

// A Q8_0 tensor (weight mode MP_WEIGHTS_Q8): as stored, int8 [N][K] + fp16 scales
// [N][K/32] (the preamble GEMMs), and for the decode projections also in int8 MFMA
// fragment order (pq, pd: mp_decode_q8.hip)
struct QW {
    const signed char *q = nullptr;
    const unsigned short *d = nullptr;
    const signed char *pq = nullptr;
    const unsigned short *pd = nullptr;
    int nib = 0;        // a Q4_0 tensor: pq holds nibble fragments (pack_q4, 18 B per 32 weights)
    size_t head_q = 0;  // bytes between consecutive heads' fragments (the 8 LT output heads)
    explicit operator bool() const { return q != nullptr; }
};
// Size (elements) of one [N][K] matrix packed as 16-bit fragments: [ceil(N/16)][K/32][64][8].
inline size_t pk_elems(int N, int K) { return (size_t)((N + 15) / 16) * 16 * K; }
// bytes of a packed Q8_0 tensor: fragments and scales (Q4_0: half the fragment bytes)
inline size_t q8p_qbytes(int N, int K) { return (size_t)((N + 15) / 16) * (K / 64) * 1024; }
inline size_t q4p_qbytes(int N, int K) { return (size_t)((N + 15) / 16) * (K / 64) * 512; }
inline size_t q8p_dbytes(int N, int K) { return (size_t)((N + 15) / 16) * (K / 64) * 64; }
// stride between the 8 packed LT heads' scales, as load_q8 lays them out (fragments: QW::head_q)
inline size_t q8p_head_d() { return (q8p_dbytes(2024, 256) + 255) & ~(size_t)255; }

struct EncLayerW { const float *norm_self, *qkv, *o, *norm_ff, *ff1, *ff2; QW qkv8, o8; };
struct DecLayerW {
    const float *norm_self, *qkv, *o, *norm_xq, *xq, *xkv, *xo, *norm_xmem, *norm_ff, *ff1, *ff2;
    QW qkv8, o8, xq8, xkv8, xo8;
};

struct Model {
    DevBlocks mem;  // every device block below
    int enc_layers = 6, dec_layers = 12, n_spk = 5, dec_pos_rows = 0, text_vocab = 2380;
    int audio_bos = 2016, audio_eos = 2017, max_dec_steps = 500;
    float eps = 1e-5f;
    const float *text_emb = nullptr, *enc_pos = nullptr, *enc_norm_out = nullptr, *dec_pos = nullptr;
    const float *dec_norm_out = nullptr, *baked = nullptr, *audio_emb = nullptr;
    std::vector<EncLayerW> enc;
    std::vector<DecLayerW> dec;
    const float *lt_in_w, *lt_in_b, *lt_pos, *lt_norm_self, *lt_qkv, *lt_o, *lt_norm_ff, *lt_ff1, *lt_ff2, *lt_out_w,
        *lt_out_b;
    float *lt_ptab = nullptr;  // [8][2024][256] = in_proj(audio_emb[c][v]) + b, built at load
    float *lt_qkvtab = nullptr;  // [7][2024][768] = qkv_net(LN(ptab[c][v] + lt_pos[c+1])), built at load
    // f32 weight mode (lt_ffn2_kernel): [7][2024][256] = o_net(v third of lt_qkvtab), and
    // [512][256] = [W_k ; W_o W_v] for position 0 (W_o W_v formed in double on the host)
    float *lt_votab = nullptr, *lt_kvo = nullptr;
    // the LT FFN-down weights [256][1024] re-laid slice-major [LT_FFN_P][256][16]: the FFN
    // workgroup that owns hidden units [16p, 16p+16) reads one contiguous 16 KiB block
    // instead of 256 half cache lines (whose other halves sit with workgroup p +- 1 on
    // another XCD: every line was fetched twice)
    float *lt_ff2s = nullptr;
    // bf16 weight mode (lt_slot_kernel): the LT FFN weights rounded to bf16, W1 row-major
    // [1024][256] and W2 slice-major [LTS_P][256][1024 / LTS_P]
    unsigned short *lt_ff1h = nullptr, *lt_ff2h = nullptr;
    // Q8_0 weight mode (lt_slot_q8_kernel): the F32 FFN-down weights slice-major [LTQ_P][256][1024 / LTQ_P]
    float *lt_ff2q = nullptr;
    std::vector<float *> xq_t;  // per layer W_q^T [768][128] (for K' = K W_q), one block
    // weight mode MP_WEIGHTS_BF16: decode projections repacked as bf16 MFMA fragments
    int weight_mode = 0;
    std::vector<const unsigned short *> pk_qkv, pk_o, pk_ff1, pk_ff2;
    const unsigned short *pk_lt_qkv = nullptr, *pk_lt_o = nullptr, *pk_lt_ff1 = nullptr, *pk_lt_ff2 = nullptr,
                         *pk_lt_out = nullptr,  // lt_out: [8][127 tiles][8][64][8]
                         *pk_lt_in = nullptr;   // F16 mode only: the LT in_proj [256][768]
    // weight mode MP_WEIGHTS_Q8: the file's Q8_0 tensors as stored (ggml's quantised mul_mat)
    bool q8_all = false;  // every decode projection is Q8_0 / Q4_0: batches up to 16
    QW lt_in8, lt_qkv8, lt_o8, lt_out8;  // lt_out8: [8][2024][256] (+ [8][2024][8] scales)
    const signed char *lt_o8t = nullptr;  // lt_o8's int8 transposed by 16-byte chunks [16][256][16] (lt_slot_q8_kernel)
    size_t arena_bytes = 0;  // the f32 arena every tensor of the file lies in
};

// f32 mode's LT (lt_ffn2_kernel) needs o_net applied to v rows ahead of time:
// VO[c][v] = W_o V[c][v] for every table row, and [W_k ; W_o W_v] for position 0.
inline bool f32_lt_mode(const Model &m) { return m.weight_mode == MP_WEIGHTS_AS_STORED; }
// the LT attention through the load-time q|k|vo tables in f32: the f32 mode, and the bf16
// mode (whose LT FFN and heads are bf16: lt_slot_kernel + the bf16 head)
inline bool lt_table_attn(const Model &m) { return m.weight_mode == MP_WEIGHTS_AS_STORED || m.weight_mode == MP_WEIGHTS_BF16; }

// Loads `path` in `weight_mode` into `m`, a fresh Model: header checks, the tensors, the
// mode's repacked copies and the LT tables; load-time kernels run on `stream`. MP_OK, or an
// error code with its text in `err` (m then holds a partial model: drop it).
int load_model(const char *path, int weight_mode, hipStream_t stream, Model &m, std::string &err);

}  // namespace mp
