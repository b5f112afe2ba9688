// Host runtime of the MI355X decode path: weight residency, per-batch device
// state, the per-utterance preamble, and the hipGraph-captured frame loop.
// Exposes the C-ABI declared in include/magpie_hip.h.
//
// Design: one mp_dev per GPU. Weights are uploaded once (f32, one
// arena). A batch of B utterances (1..8 with f32 weights, 1..16 in the bf16 / F16 /
// Q8_0 / Q4_0 modes: mp_hip_max_batch) occupies NB = next_pow2(B) slots; every
// per-utterance quantity (residual stream, KV cache, XA K/V, codes, position,
// done flag) lives in HBM and is addressed by slot, so one decode iteration
// (12 decoder layers + 8-codebook local transformer + EOS bookkeeping, 65
// kernels at NB=1 in the f32 mode) is captured once as a hipGraph and replayed per frame with
// no host round trip; the host only polls the done counter every few frames.
#include <dlfcn.h>
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <future>
#include <string>
#include <vector>

#include "../../include/magpie_hip.h"
#include "mp_device.hpp"
#include "mp_model.hpp"
#include "mp_params.hpp"
#include "mp_ops.hpp"
#include "mp_prefill_api.hpp"

namespace mp {

// The weight mode's op table at NB slots (mp_ops.hpp). f32 and Q8_0 modes: the f32 family
// (a Q8_0 file's quantised tensors take q8_ops(NB) instead, tensor by tensor). bf16 mode:
// every projection on MFMA except the f32 LT in_proj and the direct XA's f32 q_net. F16
// mode (an F16 GGUF): the same MFMA family on f16, the LT in_proj included.
static OpTable table_for(int NB, int weight_mode) {
    if (!h16_mode(weight_mode)) return f32_ops(NB);
    OpTable t = b16_ops(NB, weight_mode == MP_WEIGHTS_F16);
    if (weight_mode == MP_WEIGHTS_BF16) {
        const OpTable &f = f32_ops(NB);
        t.lt_in0 = f.lt_in0; t.lt_inh = f.lt_inh; t.xq = f.xq;
    }
    return t;
}

enum OpKind { K_GEMV = 0, K_ATTN = 1, K_FIN = 2, K_XA = 3, K_XAQ8 = 5, K_LTFFN = 6, K_LTMERGE = 7, K_LTPICK = 8,
              K_LTFFN2 = 10, K_LTKVO = 11, K_LTSLOT = 12, K_LTFRONT = 13, K_LTSLOTQ8 = 14 };
// the f32 batch-1 LT front's granules (one zeroed buffer, LtFrontP::gh): in_proj output, vo_0
constexpr size_t LTFG_TOTAL = 2 * 256;
// MAGPIE_DUMP_LT: the LT buffers of slot 0 a state record is read from after a launch
// (logits null: no record after this launch)
struct LtDumpP {
    const float *logits, *ltX, *ltY, *lty2, *ltq;
    const int *codes_cur;
};
struct OpRec {
    std::string name;
    int kind;
    GemvFn fn;
    GemvP g;
    AttnP a;
    FinP f;
    XaP x;
    XaQ8P xq;
    LtFfnP lf;
    LtFfn2P l2;
    LtFrontP lf3;
    LtSlotQ8P lq8;
    int B;
    double bytes;
    bool add_sa = false;  // the launch also runs the SA (EPI_QKV_SA): its live-cache bytes are added
    LtDumpP dump;
};

// Buffers of the local-transformer + bookkeeping part of an iteration
struct LtIo {
    float *x, *hidden, *trace;
    int trace_steps;
    float *lt_s, *ltX, *ltY, *lty2, *ltq, *ltk, *ltv, *ltf, *logits;
    float *ltp;  // [NB][LT_FFN_P][256] partial FFN-down sums (lt_ffn_kernel; lt_slot_kernel: [NB][LTS_P][256])
    unsigned long long *ltgh;  // [NB][LTS_P or LTQ_P][256] lt_slot(_q8)_kernel's partial-sum granules
    unsigned long long *ltfg;  // [LTFG_TOTAL] lt_front_kernel's hand-off granules (f32, batch 1)
    unsigned long long *ltyg;  // [NB][256] lt_slot_q8_kernel's y granules (Q8_0 mode)
    int *iter, *hx_err;        // decode iteration counter (hand-off tags), hand-off error bits
    int *codes_cur, *codes_prev, *codes_out, *step, *pos, *done, *nframes, *ndone, *argeos, *amax;
    SmpCfg *cfg;
    int sampling, ignore_eos, emit_eos, max_steps, lt_only;
    int guided;  // the slots are paired (Sampling::guided)
};

}  // namespace mp

// The preamble's buffers and stream: the batch's own (mp_hip_begin_batch: batch_ws) or a
// staging workspace of the slot pool (mp_hip_decode_queue), which runs one utterance's
// preamble on a side stream while the batch keeps decoding. The outputs' strides follow
// from Tmax (xak / xav / kp / vp rows per layer) and max_seq (kc / vc rows per layer).
struct PreWs {
    const int32_t *tok, *T, *spk;  // device [NB][Tmax] token ids, [NB] lengths, [NB] speakers
    int NB, Tmax, max_seq, kv16;
    bool xa_direct;                // no K' / V' (kp, vp unused)
    // classifier-free guidance (0: none): slots [n_text, 2 n_text) are the text-free partners
    // of slots [0, n_text). The encoder and the XA K/V run for the n_text leading slots only;
    // the partners' tables are zeros, their context rows the positions alone, and the padding
    // slots behind them get slot 0's tables
    int n_text;
    float *pX, *pH, *pQKV, *pATT, *pF, *pXQ, *pXAO, *gpart, *enc_out;  // scratch
    float *xak, *xav, *kp, *vp, *kc, *vc;                              // outputs
    hipStream_t stream;
};
// A staging workspace of the slot pool: one utterance's preamble (NB = 1) of up to tmax
// tokens, run on the pool's side stream; `ready` is recorded behind the preamble,
// `installed` behind the slot_install_kernel launch that read it (the workspace is reused
// only after that event has completed).
struct StageWs {
    PreWs w{};
    mp::DevBlocks mem;
    int32_t *tok = nullptr, *T = nullptr, *spk = nullptr;  // device
    mp::Pinned pin;  // int32 [tmax + 2]: tokens, length, speaker
    mp::Event ready, installed;
    bool install_pending = false;
    int utt = -1, n = 0;
};

struct mp_dev {
    int device = 0;
    // the decode stream, and the side stream the slot pool's preambles run on (made by the
    // first mp_hip_decode_queue). Declared first: they outlive every buffer below.
    mp::Stream stream, side;
    std::string err;
    mp::Model m;
    bool loaded = false;
    // batch configuration
    int B = 0, NB = 0, Tmax = 0, max_steps = 0, max_seq = 0, nch = 0;
    // mp_hip_set_cfg: applies from the next mp_hip_begin_batch. A guided batch (`guided`) of B
    // utterances has slots = 2 B: slot b < B is utterance b's conditional branch, slot B + b
    // its unconditional partner; otherwise slots = B
    float cfg_scale = 0.f;
    bool guided = false;
    int slots = 0;
    mp_params params{};
    int kv_mode = MP_KV_F32;  // mp_hip_set_kv_mode: applies from the next mp_hip_begin_batch
    int xa_mode = MP_XA_AUTO;  // mp_hip_set_xa_mode: likewise
    // mp_hip_set_stream_codec_mode: applies from the next mp_hip_decode_stream or
    // mp_hip_decode_queue_stream. CONTINUOUS:
    // slot b is lane b of `cstream`, made on the first use of a codec and kept while the
    // codec and the lane count hold (released by mp_hip_free, which does not touch the codec)
    int stream_codec_mode = MP_STREAM_CODEC_STATELESS;
    mp_codec_stream *cstream = nullptr;
    mp_codec *cstream_codec = nullptr;
    int cstream_lanes = 0;
    bool xa_direct = false;    // this batch runs the direct XA form (f32 / bf16 modes)
    int kv16 = 0;             // the current batch's SA cache holds bf16
    // device state (one allocation per buffer, sized for the configuration)
    mp::DevBlocks mem;
    // the hand-off granule buffers among them, with their element counts: reset_decode_state
    // clears exactly what alloc_batch made
    std::vector<std::pair<unsigned long long *, size_t>> granules;
    float *x = nullptr, *x2 = nullptr, *kp = nullptr, *vp = nullptr, *q = nullptr, *sa_out = nullptr,
          *h = nullptr, *hidden = nullptr;
    float *xqb = nullptr;  // Q8 mode: q_net output [NB][128]
    unsigned short *h_b16 = nullptr;  // bf16 mode: GELU(FFN up) as the bf16 FFN-down operand [NB][3072]
    float *gpart = nullptr;            // preamble split-K partial sums (mp::gemm_splits)
    mp::Event sev[2];           // streaming: the two chunk snapshots landed
    mp::Pinned h_codes_pin;     // streaming: pinned mirrors of codes_out and the snapshots (StreamRun's layout)
    float *sa_part = nullptr, *xa_part = nullptr;  // split-K attention states [NB][12][4][68], [NB][4][772]
    unsigned long long *sagh = nullptr, *xagh = nullptr;  // 16-slot merges: split-state granules
    unsigned long long *kgh = nullptr;  // split-K FFN-down partial tiles (16-bit modes): [48][KS][256]
    unsigned long long *xh = nullptr;  // O-projection -> XA hand-off granules [NB][768] (EPI_RESID_XA)
    unsigned long long *qh = nullptr;  // QKV -> SA hand-off granules [NB][2304] (EPI_QKV_SA)
    unsigned long long *xqh = nullptr; // Q8_0 XA q_net -> attention hand-off granules [NB][128] (EPI_RESID_XQ8)
    float *kc = nullptr, *vc = nullptr, *xak = nullptr, *xav = nullptr;
    float *lt_s = nullptr, *ltX = nullptr, *ltY = nullptr, *lty2 = nullptr, *ltq = nullptr, *ltk = nullptr,
          *ltv = nullptr, *ltf = nullptr, *logits = nullptr, *trace = nullptr, *ltp = nullptr;
    unsigned long long *ltgh = nullptr, *ltfg = nullptr, *ltyg = nullptr;
    int *T = nullptr, *spk = nullptr, *pos = nullptr, *step = nullptr, *done = nullptr, *nframes = nullptr,
        *ndone = nullptr, *codes_cur = nullptr, *codes_prev = nullptr, *codes_out = nullptr, *tok = nullptr,
        *argeos = nullptr, *amax = nullptr;
    mp::SmpCfg *smpcfg = nullptr;
    int lt_calls = 0;
    // magpie_local_transformer_sample_all scratch (batch 1, independent of any batch)
    mp::DevBlocks ltio_mem;
    mp::LtIo lt_io{};
    // preamble scratch
    float *pX = nullptr, *pH = nullptr, *pQKV = nullptr, *pATT = nullptr, *pF = nullptr, *pXQ = nullptr,
          *pXAO = nullptr, *enc_out = nullptr;
    // graph
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    std::vector<mp::OpRec> ops;
    bool batch_ready = false;
    mp_timing timing{};
    mp::Pinned h_ndone;  // one int
    // mp_hip_encode_text's private workspace: grows on demand, kept until mp_hip_free (a
    // per-call hipFree would synchronise the whole device, stalling other streams' work)
    mp::DevBlocks enc_ws_mem;
    char *enc_ws = nullptr;
    size_t enc_ws_bytes = 0;
    // diagnostics (MAGPIE_Q8DUMP=1 at mp_hip_begin_batch, Q8_0 weights): one dump slot per
    // int8-MFMA decode GEMM launch of the iteration (GemvP::q8dump), records in q8dump_index
    char *q8dump = nullptr;
    size_t q8dump_slot = 0;
    int q8dump_cap = 0, q8dump_n = 0;
    std::vector<int> q8dump_index;
    // slot pool (mp_hip_decode_queue): two staging workspaces, kept between calls while their
    // shape (tmax, cache type, XA form) holds
    StageWs stage[2];
    int stage_tmax = 0, stage_kv16 = 0;
    bool stage_direct = false;
};

namespace {

#define HIPCHK(expr) MP_HIPCHK_TO(dev->err, expr)

int fail(mp_dev *dev, int code, const std::string &msg) {
    dev->err = msg;
    return code;
}

void free_batch(mp_dev *dev) {
    if (dev->exec) hipGraphExecDestroy(dev->exec);
    if (dev->graph) hipGraphDestroy(dev->graph);
    dev->exec = nullptr;
    dev->graph = nullptr;
    dev->mem.clear();
    dev->granules.clear();
    dev->ops.clear();
    dev->batch_ready = false;
    dev->B = dev->NB = dev->Tmax = dev->max_steps = dev->slots = 0;
    dev->guided = false;
    dev->xa_direct = false;
    dev->kp = dev->vp = nullptr;
    dev->trace = nullptr;  // a batch without a trace must not see (or write) the last one's
    dev->q8dump = nullptr;
    dev->q8dump_cap = dev->q8dump_n = 0;
    dev->q8dump_index.clear();
}

// the slot pool's staging workspaces (the side stream stays until mp_hip_free)
void free_stage(mp_dev *dev) {
    if (dev->side) hipStreamSynchronize(dev->side);
    for (StageWs &s : dev->stage) s = StageWs{};
    dev->stage_tmax = 0;
}

// MAGPIE_Q8DUMP: give a Q8_0 decode GEMM launch its dump slot and index record
// [N, K, NB, layer, cb, byte offset, name (40 bytes)] (16 ints)
constexpr int Q8DUMP_REC = 16;
void q8dump_assign(mp_dev *dev, const char *name, mp::GemvP &g) {
    if (!dev->q8dump || !g.Wq || dev->q8dump_n >= dev->q8dump_cap) return;
    const int n = dev->q8dump_n++;
    g.q8dump = dev->q8dump + (size_t)n * dev->q8dump_slot;
    const int K = strncmp(name, "lt_in", 5) == 0 ? 768 : (strncmp(name, "lt_", 3) == 0 ? 256 : 768);
    int rec[Q8DUMP_REC] = {g.N, K, dev->NB, g.layer, g.cb, (int)((size_t)n * dev->q8dump_slot)};
    strncpy((char *)&rec[6], name, 39);
    dev->q8dump_index.insert(dev->q8dump_index.end(), rec, rec + Q8DUMP_REC);
}

double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// ------------------------------------------------------------------ batch state
// the cross-attention form of a batch (mp_hip_set_xa_mode): direct where it reads fewer
// bytes (Tmax > MP_XA_DIRECT_T); F16 keeps the reassociated form, Q8_0 has its own
bool want_xa_direct(const mp_dev *dev, int Tmax) {
    const int wm = dev->m.weight_mode;
    if (wm != MP_WEIGHTS_AS_STORED && wm != MP_WEIGHTS_BF16) return false;
    return dev->xa_mode == MP_XA_DIRECT || (dev->xa_mode == MP_XA_AUTO && Tmax > MP_XA_DIRECT_T);
}

static size_t enc_gpart_elems(size_t Me);
// The preamble's split-K partial-sum capacity (elements) for Me rows of text, Mc rows of
// context and L decoder layers: the largest S x M x N of its GEMMs (encoder FFN up/down,
// prefill FFN)
static size_t pre_gpart_elems(size_t Me, size_t Mc, int L) {
    size_t cap = enc_gpart_elems(Me);
    auto need = [&](size_t M, int N, int K) { cap = std::max(cap, (size_t)mp::gemm_splits_max(K) * M * N); };
    need(Mc, 2304, 768); need(Mc, 3072, 768); need(Mc, 768, 3072); need(Mc, 768, 768);
    need(Me, 256 * L, 768);  // the XA K/V GEMMs batched over layers
    return cap;
}
// The preamble's scratch set {pX, pH, pQKV, pATT, pF, pXQ, pXAO, enc_out}: `rows` rows (text
// or context, whichever is more) and enc_rows of encoder output; zero-filled on *zero when
// given (the batch's buffers are)
static hipError_t alloc_pre_scratch(mp::DevBlocks &mem, float **const (&p)[8], size_t rows, size_t enc_rows,
                                    const hipStream_t *zero) {
    const size_t n[8] = {rows * 768, rows * 768, rows * 3 * 768, rows * 768, rows * 3072, rows * 128, rows * 128, enc_rows * 768};
    for (int i = 0; i < 8; ++i)
        if (hipError_t e = zero ? mem.get_zeroed(p[i], n[i], *zero) : mem.get(p[i], n[i])) return e;
    return hipSuccess;
}
int alloc_batch(mp_dev *dev, int B, bool guided, int Tmax, int max_steps, bool trace) {
    free_batch(dev);
    const int slots = guided ? 2 * B : B;
    const int NB = slots <= 1 ? 1 : slots <= 2 ? 2 : slots <= 4 ? 4 : slots <= 8 ? 8 : 16;
    const int L = dev->m.dec_layers;
    dev->B = B;
    dev->slots = slots;
    dev->guided = guided;
    dev->NB = NB;
    dev->Tmax = Tmax;
    dev->max_steps = max_steps;
    dev->max_seq = mp::CTX + max_steps + 16;  // magpie.cpp:4077
    dev->nch = (dev->max_seq + mp::SA_CHUNK - 1) / mp::SA_CHUNK;
    dev->max_seq = dev->nch * mp::SA_CHUNK;  // whole chunks: attention loads never leave the cache slab
    const size_t D = 768;
    const hipStream_t st = dev->stream;
#define A(ptr, n) HIPCHK(dev->mem.get_zeroed(&dev->ptr, (size_t)(n), st))
    // a hand-off granule buffer: noted with its size for reset_decode_state
#define G(ptr, n) do { A(ptr, n); dev->granules.push_back({dev->ptr, (size_t)(n)}); } while (0)
    // this batch's KV width and XA form first: the allocations below depend on them
    // (a batch must never inherit the previous batch's form)
    dev->kv16 = dev->kv_mode == MP_KV_BF16;
    dev->xa_direct = want_xa_direct(dev, Tmax);
    A(x, NB * D); A(x2, NB * D); A(q, NB * D);
    if (!dev->xa_direct) { A(kp, (size_t)NB * L * Tmax * D); A(vp, (size_t)NB * L * Tmax * D); }  // else null (free_batch)
    A(sa_out, NB * 768);
    A(h, NB * 3072); A(hidden, NB * D); A(xqb, NB * 128); A(h_b16, NB * 3072);
    A(sa_part, (size_t)NB * mp::NH * mp::SA_SPLITS * mp::SA_PART); A(xa_part, (size_t)NB * mp::XA_SPLITS * mp::XA_PART);
    G(sagh, (size_t)NB * mp::NH * mp::SA_SPLITS * mp::SA_PART); G(xagh, (size_t)NB * mp::XA_SPLITS * mp::XA_PART);
    G(kgh, (size_t)2 * (768 / 16) * mp::KGH_MAX_KS * 256);  // [O-projection | FFN down]
    G(xh, (size_t)NB * D); G(qh, (size_t)NB * 3 * D); G(xqh, (size_t)NB * 128);
    const size_t kvn = (size_t)NB * L * dev->max_seq * D;  // elements; bf16 mode: 2 per float slot
    A(kc, dev->kv16 ? kvn / 2 : kvn); A(vc, dev->kv16 ? kvn / 2 : kvn);
    A(xak, (size_t)NB * L * Tmax * 128); A(xav, (size_t)NB * L * Tmax * 128);
    A(lt_s, NB * 9 * 256); A(ltX, NB * 256); A(ltY, NB * 256); A(lty2, NB * 256); A(ltq, NB * 256);
    A(ltk, NB * 8 * 256); A(ltv, NB * 8 * 256); A(ltf, NB * 1024); A(logits, NB * 2024);
    A(ltp, (size_t)NB * std::max({mp::LT_FFN_P, mp::LTS_P, mp::LTQ_P}) * 256); G(ltgh, (size_t)NB * std::max(mp::LTS_P, mp::LTQ_P) * 256); G(ltfg, mp::LTFG_TOTAL); G(ltyg, (size_t)NB * 256);
    if (trace) A(trace, (size_t)NB * (max_steps + 1) * D);
    A(T, NB); A(spk, NB); A(pos, NB); A(step, NB); A(done, NB); A(nframes, NB); A(ndone, 4);  // ndone: [done count, iteration, hand-off timeout, -]
    A(argeos, NB); A(amax, NB * 8); A(smpcfg, 1);
    A(codes_cur, NB * 8); A(codes_prev, NB * 8); A(codes_out, (size_t)NB * max_steps * 8); A(tok, (size_t)NB * Tmax);
    float **const pre[8] = {&dev->pX, &dev->pH, &dev->pQKV, &dev->pATT, &dev->pF, &dev->pXQ, &dev->pXAO, &dev->enc_out};
    HIPCHK(alloc_pre_scratch(dev->mem, pre, (size_t)NB * std::max(Tmax, mp::CTX), (size_t)NB * Tmax, &st));
    A(gpart, pre_gpart_elems((size_t)NB * Tmax, (size_t)NB * mp::CTX, L));
    if (mp::env_int("MAGPIE_Q8DUMP", 0) != 0 && dev->m.weight_mode == MP_WEIGHTS_Q8) {
        // the largest launch: K = 768, N = 2304 (QKV): rows, blocks, d, dots
        const size_t slot = ((size_t)NB * 768 * 5 + (size_t)NB * 24 * 4 + (size_t)2304 * 24 * NB * 4 + 255) / 256 * 256;
        dev->q8dump_cap = 4 * L + 16;
        dev->q8dump_slot = slot;
        A(q8dump, slot * dev->q8dump_cap);
    }
#undef G
#undef A
    return MP_OK;
}

// ------------------------------------------------------------------ the iteration's launch list
// A decode iteration is a list of OpRec. build_iteration / build_lt decide which kernels it
// consists of for the weight mode, batch size and knobs and fill their parameter structs;
// launch_ops launches a list; the profiling API (mp_hip_profile_ops*, mp_hip_time_op)
// replays the decode's own. The list is invariant per batch configuration: every varying
// quantity (position, step, iteration counter, sampling settings) lives in device memory,
// so it is built once per batch and one captured graph serves every frame.

// MAGPIE_EAGER=1: launch the iteration's kernels directly instead of replaying
// the captured graph (identical kernels and arguments; used under rocprofv3,
// whose kernel tracer crashes on graph replays on this image).
bool eager_mode() { return mp::env_int("MAGPIE_EAGER", 0) != 0; }
// The knobs below are read when a list is built (the first decode of a batch
// configuration), in eager mode as in graph mode.
// MAGPIE_Q8_UNFUSED=1: the Q8_0 mode's SA and XA as separate launches (the fused forms
// compute the same bits; tests/test_q8_fused_gpu.py compares them)
bool q8_unfused() { return mp::env_int("MAGPIE_Q8_UNFUSED", 0) != 0; }
// The SA in the QKV launch at 16 slots: MAGPIE_SA16 unset = the bf16 mode's, 1 = every
// mode's, 0 = none (A/B; both forms compute the same bits). Round 3 kept it separate (bf16
// B=16 20.1k vs 21.5k frames/s then); since round 4's single pollers the fused form is
// faster: 31,891 -> 32,620 / 32,893 frames/s (qkv 4.54 + sa_attn 7.34 -> qkv_sa 11.05 us
// per layer; gpurun_out/r06l_ops_bf16_b16*)
bool sa16_fused(int weight_mode) { return mp::env_int("MAGPIE_SA16", weight_mode == MP_WEIGHTS_BF16) != 0; }
// At 8 bf16 slots, which split states the split workgroups merge themselves (bit 0: SA, in
// the QKV launch; bit 1: XA, in the O-projection's) rather than the consumers' prologues
// (PRO_SA_MERGE, PRO_XA_LN): MAGPIE_MERGE8, default 3 (A/B; every setting the same bits)
int split_merge8() { return mp::env_int("MAGPIE_MERGE8", 3); }
// MAGPIE_LTQ8 (Q8_0 LT step, lt_slot_q8_kernel): 0 = o_net rows split over the workgroups
// (y hand-off) and the FFN merge in the launch; 1 = every workgroup all o_net rows (no y
// hand-off); 2 (default) = that up to 4 slots, and at batch 1 the FFN merge deferred to
// the head's prologue. Every setting computes the same bits (tests/test_q8_fused_gpu.py).
int ltq8_mode() { return mp::env_int("MAGPIE_LTQ8", 2); }

// a tensor's decode bytes per weight: quantised in the file Q8_0 34/32, Q4_0 nibble
// fragments 18/32; else F, its width in the weight mode
double weight_bytes(const mp::QW &q, double F) { return !q ? F : q.nib ? 18.0 / 32.0 : 34.0 / 32.0; }
// a GEMV's weight operands: f32 rows, 16-bit fragments (bf16 / F16 modes), and the Q8_0 /
// Q4_0 fragments of a tensor quantised in the file (the kernel family reads its own)
void set_weights(mp::GemvP &g, const float *W, const unsigned short *Wb, const mp::QW &q) {
    g.W = W; g.Wb = Wb; g.Wq = q.pq; g.Wd = q.pd; g.q4 = q.nib;
}
// the hand-off state of a launch whose workgroups wait on one another: the decode
// iteration counter (the granules' tags) and the error bits, both behind ndone
template <class P> void set_handoff(P &p, int *ndone) { p.iter = ndone + 1; p.hx_err = ndone + 2; }

// a zeroed GemvP with the model's constants and its slots' step and sampling state
mp::GemvP gemv_base(const mp::Model &m, int NB, int *step, const mp::Sampling &smp, bool ignore_eos) {
    mp::GemvP g;
    memset(&g, 0, sizeof g);
    g.eps = m.eps;
    g.step = step;
    g.smp = smp;
    g.nslots = NB;
    g.ignore_eos = ignore_eos;
    g.audio_bos = m.audio_bos;
    g.audio_eos = m.audio_eos;
    return g;
}

// Appends records to a launch list. q8dump: the GEMVs take MAGPIE_Q8DUMP slots (a decode
// iteration's do, mp_hip_lt_sample's do not). dump: noted on every record added; build_lt
// clears it on the records no MAGPIE_DUMP_LT state record follows.
struct Emit {
    mp_dev *dev;
    std::vector<mp::OpRec> &out;
    int NB;
    bool q8dump;
    mp::LtDumpP dump;
    // one record: its kind, the kind's parameter struct (OpRec's member `par`), the
    // algorithmic bytes (weights at their stored width, Q8_0: 34 B per 32; activations f32)
    template <class P> mp::OpRec &add(const char *name, int kind, P mp::OpRec::*par, const P &p, double bytes) const {
        mp::OpRec r{};
        r.name = name; r.kind = kind; r.*par = p; r.B = NB; r.bytes = bytes; r.dump = dump;
        out.push_back(r);
        return out.back();
    }
    // a GEMV from the op table: a null entry is a batch size / weight mode without a kernel
    int gemv(const char *name, mp::GemvFn fn, mp::GemvP g, double bytes) const {
        if (!fn) return fail(dev, MP_ERR_UNSUPPORTED, std::string(name) + ": no kernel for this batch size / weight mode");
        if (q8dump) q8dump_assign(dev, name, g);
        add(name, mp::K_GEMV, &mp::OpRec::g, g, bytes).fn = fn;
        return MP_OK;
    }
};

// The local transformer over one frame (magpie_local_transformer_sample_all,
// magpie.cpp:1113-1317) + the frame bookkeeping (4320-4358), for NB slots whose
// buffers `io` names. lt_only: in_proj of a given normalised hidden, codes only.
int build_lt(mp_dev *dev, const mp::LtIo &io, int NB, std::vector<mp::OpRec> &out, bool q8dump = false) {
    const mp::Model &m = dev->m;
    const bool b16 = mp::h16_mode(m.weight_mode);
    const mp::OpTable tb = mp::table_for(NB, m.weight_mode);
    const mp::OpTable &tq = mp::q8_ops(NB);
    // the family of a tensor: the Q8_0 one where the file holds it quantised
    auto fam = [&](const mp::QW &q) -> const mp::OpTable & { return q ? tq : tb; };
    const double F = b16 ? 2.0 : 4.0, A = 4.0, act = (double)NB;
    const mp::Sampling smp{io.sampling, io.cfg, io.argeos, io.amax, io.guided};
    const Emit e{dev, out, NB, q8dump, mp::LtDumpP{io.logits, io.ltX, io.ltY, io.lty2, io.ltq, io.codes_cur}};
    auto base = [&](int cb) {
        mp::GemvP g = gemv_base(m, NB, io.step, smp, io.ignore_eos);
        g.cb = cb;
        return g;
    };
    // position 0 of the f32 and bf16 modes: LN + [k_0 | vo_0]
    auto kvo = [&]() {
        mp::GemvP g = base(0);
        g.W = m.lt_kvo; g.N = 512; g.lt_s = io.lt_s; g.lt_pos = m.lt_pos; g.ltX = io.ltX; g.lnw = m.lt_norm_self;
        g.lk = io.ltk; g.lv = io.ltv;
        e.add("lt_kvo", mp::K_LTKVO, &mp::OpRec::g, g, A * (512.0 * 256) + A * act * (256 * 4));
    };
    // codebook cb's LT step in one launch (lt_ffn2_kernel, lt_slot_kernel) on FFN f
    auto step2 = [&](int cb, const mp::LtFfnP &f) {
        mp::LtFfn2P l2{};
        l2.f = f;
        l2.cb = cb; l2.ltX = io.ltX; l2.ltk = io.ltk; l2.ltv = io.ltv; l2.qkvtab = m.lt_qkvtab;
        l2.votab = m.lt_votab; l2.ptab = m.lt_ptab; l2.lt_pos = m.lt_pos; l2.logits = io.logits;
        l2.codes_cur = io.codes_cur; l2.step = io.step; l2.ignore_eos = io.ignore_eos;
        l2.audio_bos = m.audio_bos; l2.audio_eos = m.audio_eos;
        l2.smp = smp;
        return l2;
    };
    // the one-workgroup merge of the FFN's partial sums (batches; at batch 1 the head's
    // prologue merges them)
    auto merge = [&](const mp::LtFfnP &lf) {
        if (NB > 1) e.add("lt_merge", mp::K_LTMERGE, &mp::OpRec::lf, lf, A * act * (mp::LT_FFN_P * 256 + 512)).dump = {};
    };
    // codebook cb's head on y2. merged: the FFN merge is its prologue, y2 = y + the
    // partial sums (src_elems of them per slot)
    auto head = [&](int cb, mp::GemvFn fn, bool merged, int src_elems) {
        mp::GemvP g = base(cb);
        g.W = m.lt_out_w + (size_t)cb * 2024 * 256; g.N = 2024; g.bias = m.lt_out_b + (size_t)cb * 2024;
        g.Wb = b16 ? m.pk_lt_out + (size_t)cb * mp::pk_elems(2024, 256) : nullptr;
        g.src = io.lty2; g.src_ld = 256; g.out = io.logits; g.out_ld = 2024;
        if (m.lt_out8) {
            g.Wq = m.lt_out8.pq + (size_t)cb * m.lt_out8.head_q; g.q4 = m.lt_out8.nib;
            g.Wd = (const unsigned short *)((const char *)m.lt_out8.pd + (size_t)cb * mp::q8p_head_d());
        }
        if (merged) { g.part = io.ltp; g.addsrc = io.ltY; }
        return e.gemv("lt_e", fn, g,
                      weight_bytes(m.lt_out8, F) * (2024.0 * 256) + A * 2024 + A * act * (src_elems + 2024));
    };
    // f32 mode at batch 1: final LN + in_proj + position 0 + codebook 0's FFN step in one
    // launch (lt_front_kernel: the same rows, the same arithmetic; 2 in-launch granule edges)
    const bool front = f32_lt_mode(m) && NB == 1 && !io.lt_only && io.ltfg && io.iter;
    if (!front) {
        mp::GemvP g = base(0);
        set_weights(g, m.lt_in_w, m.pk_lt_in, m.lt_in8);  // pk_lt_in: F16 mode only
        g.N = 256; g.bias = m.lt_in_b; g.out = io.lt_s; g.out_ld = 9 * 256;
        const double Fi = weight_bytes(m.lt_in8, m.pk_lt_in ? 2.0 : A);
        if (io.lt_only) {
            // in_proj of the caller's (already normalised) hidden (1161-1163)
            g.src = io.hidden; g.src_ld = 768;
            if (int rc = e.gemv("lt_inh", fam(m.lt_in8).lt_inh, g,
                                Fi * 256.0 * 768 + A * 256 + A * (768 + 256)))
                return rc;
        } else {
            // final LN -> hidden (4394) fused into LT in_proj (1162-1163)
            g.lnw = m.dec_norm_out; g.src = io.x; g.src_ld = 768; g.hidden_out = io.hidden;
            if (io.trace) { g.trace = io.trace; g.trace_steps = io.trace_steps; g.step = io.step; }
            if (int rc = e.gemv("lt_in0", fam(m.lt_in8).lt_in0, g,
                                Fi * 256.0 * 768 + A * 256 + A * act * ((768 + 768 + 256))))
                return rc;
        }
    }
    if (m.weight_mode == MP_WEIGHTS_BF16) {
        // bf16 mode: the f32 mode's position 0 (LN + [k_0 | vo_0]), then per codebook the
        // LT step as LTS_P workgroups per slot (lt_slot_kernel: pick, f32 attention
        // through the tables, bf16 FFN, partial sums merged by the slot's last
        // workgroup) and the bf16 head: 2 launches per codebook at every batch size
        kvo();
        for (int cb = 0; cb < 8; ++cb) {
            mp::LtFfn2P l2 = step2(cb, mp::LtFfnP{io.ltY, m.lt_norm_ff, nullptr, nullptr, m.eps, io.ltp, io.lty2});
            // the partial sums merged by the head's prologue at batch 1 (32 KiB per head
            // workgroup; 4 slots' 128 KiB took 11.5 us), through granules by the LT step
            // itself above (the standalone LT API is batch 1: no iteration counter needed)
            const bool head_merge = NB == 1;
            l2.w1h = m.lt_ff1h; l2.w2h = m.lt_ff2h;
            if (!head_merge) { l2.gh = io.ltgh; l2.iter = io.iter; l2.hx_err = io.hx_err; }
            e.add("lt_slot", mp::K_LTSLOT, &mp::OpRec::l2, l2,
                  F * (1024.0 * 256 * 2) + A * act * (cb ? 2024 + 4 * 256 + 2 * 256 * cb : 512) +
                      A * act * (mp::LTS_P * 256 + 256));
            if (int rc = head(cb, head_merge ? tb.lt_em : tb.lt_e, head_merge, head_merge ? mp::LTS_P * 256 : 256))
                return rc;
        }
    } else if (f32_lt_mode(m)) {
        // f32 mode: LN + [k_0 | vo_0] for position 0, then per codebook ONE launch for
        // pick + attention + o_net + residual + FFN (lt_ffn2_kernel) and the head
        if (!front) kvo();
        for (int cb = 0; cb < 8; ++cb) {
            const mp::LtFfn2P l2 = step2(cb, mp::LtFfnP{io.ltY, m.lt_norm_ff, m.lt_ff1, m.lt_ff2s, m.eps, io.ltp, io.lty2});
            if (front && cb == 0) {
                // lt_front_kernel: the final LN, in_proj, position 0 and codebook 0's FFN step
                mp::LtFrontP fp{};
                fp.l = l2; fp.x = io.x; fp.norm_out = m.dec_norm_out; fp.w_in = m.lt_in_w; fp.b_in = m.lt_in_b;
                fp.lt_s = io.lt_s; fp.hidden_out = io.hidden; fp.lt_pos = m.lt_pos; fp.norm_self = m.lt_norm_self;
                fp.w_kvo = m.lt_kvo; fp.gh = io.ltfg; fp.iter = io.iter; fp.hx_err = io.hx_err;
                if (io.trace) { fp.trace = io.trace; fp.trace_steps = io.trace_steps; }
                e.add("lt_front", mp::K_LTFRONT, &mp::OpRec::lf3, fp,
                      A * (256.0 * 768 + 512.0 * 256 + 1024.0 * 256 * 2) + A * (768 * 2 + 256 * 4) +
                          A * (mp::LT_FFN_P * 256));
            } else {
                e.add("lt_ffn2", mp::K_LTFFN2, &mp::OpRec::l2, l2,
                      A * (1024.0 * 256 * 2) + A * act * (cb ? 2024 + 4 * 256 + 2 * 256 * cb : 512) +
                          A * act * (mp::LT_FFN_P * 256 + 256));
            }
            merge(l2.f);
            if (int rc = head(cb, NB == 1 ? tb.lt_em : tb.lt_e, NB == 1, 256)) return rc;
        }
    } else if (m.weight_mode == MP_WEIGHTS_Q8 && m.lt_o8 && m.lt_out8 && m.lt_ff2q && !io.lt_only && io.ltyg) {
        // Q8_0 mode: position 0's q|k|v (the Q8_0 GEMV), then per codebook the LT step as
        // LTQ_P workgroups per slot (lt_slot_q8_kernel: pick, attention, Q8_0 o_net, F32
        // FFN, partial sums merged through granules) and the Q8_0 head on its output
        mp::GemvP g = base(0);
        set_weights(g, m.lt_qkv, nullptr, m.lt_qkv8);
        g.N = 768; g.lt_s = io.lt_s; g.lt_pos = m.lt_pos; g.ltX = io.ltX;
        g.lnw = m.lt_norm_self; g.lq = io.ltq; g.lk = io.ltk; g.lv = io.ltv;
        if (int rc = e.gemv("lt_a", tq.lt_a, g, weight_bytes(m.lt_qkv8, F) * (768.0 * 256) + A * act * (256 * 3 + 768 + 256)))
            return rc;
        const int lm = ltq8_mode();
        for (int cb = 0; cb < 8; ++cb) {
            mp::LtSlotQ8P sp{};
            sp.g = base(cb);
            sp.g.logits = io.logits; sp.g.codes_cur = io.codes_cur; sp.g.qkvtab = m.lt_qkvtab; sp.g.ptab = m.lt_ptab;
            sp.g.lt_pos = m.lt_pos; sp.g.ltk = io.ltk; sp.g.ltv = io.ltv; sp.g.lk = io.ltk; sp.g.lv = io.ltv;
            sp.g.ltX = io.ltX;
            sp.woq = m.lt_o8.q; sp.wod = m.lt_o8.d; sp.lnw = m.lt_norm_ff; sp.eps = m.eps; sp.w1 = m.lt_ff1;
            sp.w2s = m.lt_ff2q; sp.y = io.ltY; sp.y2 = io.lty2; sp.gy = io.ltyg; sp.gp = io.ltgh;
            sp.iter = io.iter; sp.hx_err = io.hx_err;
            if (lm == 1 || (lm >= 2 && NB <= 4)) sp.wot = m.lt_o8t;  // (8+ slots: 512+ workgroups, the split rows)
            if (lm >= 2 && NB == 1 && sp.wot) sp.part = io.ltp;
            e.add("lt_slot_q8", mp::K_LTSLOTQ8, &mp::OpRec::lq8, sp,
                  (34.0 / 32.0) * (256.0 * 256) + A * (1024.0 * 256 * 2) +
                      A * act * (cb ? 2024 + 4 * 256 + 2 * 256 * cb : 512) + A * act * (mp::LTQ_P * 256 + 512));
            // (sp.part: the FFN merge is the head's prologue)
            if (int rc = head(cb, sp.part ? tq.lt_em : tq.lt_e, sp.part != nullptr, 256)) return rc;
        }
    } else
    for (int cb = 0; cb < 8; ++cb) {
        mp::GemvP g;
        if (cb == 0) {
            // position 0 (the hidden's in_proj): LN + q|k|v GEMV, then attention + o_net
            g = base(0);
            set_weights(g, m.lt_qkv, m.pk_lt_qkv, m.lt_qkv8);
            g.N = 768; g.lt_s = io.lt_s; g.lt_pos = m.lt_pos; g.ltX = io.ltX;
            g.lnw = m.lt_norm_self; g.lq = io.ltq; g.lk = io.ltk; g.lv = io.ltv;
            if (int rc = e.gemv("lt_a", fam(m.lt_qkv8).lt_a, g,
                                weight_bytes(m.lt_qkv8, F) * (768.0 * 256) + A * act * (256 * 3 + 768 + 256)))
                return rc;
            g = base(0);
            set_weights(g, m.lt_o, m.pk_lt_o, m.lt_o8);
            g.N = 256; g.ltq = io.ltq; g.ltk = io.ltk; g.ltv = io.ltv; g.out = io.ltY;
            g.out_ld = 256; g.addsrc = io.ltX;
            if (int rc = e.gemv("lt_b", fam(m.lt_o8).lt_b, g, weight_bytes(m.lt_o8, F) * (256.0 * 256) + A * act * (256 * 5)))
                return rc;
        } else if (NB >= 8) {
            // large batches: the per-slot pick + gathers + attention as one wave per slot
            // (lt_pick_kernel), then o_net + residual; the same arithmetic as lt_bg
            g = base(cb);
            g.logits = io.logits; g.codes_cur = io.codes_cur; g.qkvtab = m.lt_qkvtab; g.ptab = m.lt_ptab;
            g.lt_pos = m.lt_pos; g.ltk = io.ltk; g.ltv = io.ltv; g.lk = io.ltk; g.lv = io.ltv; g.ltX = io.ltX;
            g.out = io.ltq;
            e.add("lt_pick", mp::K_LTPICK, &mp::OpRec::g, g, A * act * (2024 + 4 * 256 + 2 * 256 * cb + 4 * 256));
            g = base(cb);
            set_weights(g, m.lt_o, m.pk_lt_o, m.lt_o8);
            g.N = 256; g.src = io.ltq; g.src_ld = 256; g.out = io.ltY; g.out_ld = 256; g.addsrc = io.ltX;
            if (int rc = e.gemv("lt_bo", fam(m.lt_o8).lt_bo, g, weight_bytes(m.lt_o8, F) * (256.0 * 256) + A * act * (256 * 3)))
                return rc;
        } else {
            // position cb: codebook cb-1's pick, its q|k|v row gathered from the load-time
            // table (no q|k|v GEMV), attention + o_net + residual, one launch
            g = base(cb);
            set_weights(g, m.lt_o, m.pk_lt_o, m.lt_o8);
            g.N = 256; g.out = io.ltY; g.out_ld = 256;
            g.logits = io.logits; g.codes_cur = io.codes_cur; g.qkvtab = m.lt_qkvtab; g.ptab = m.lt_ptab;
            g.lt_pos = m.lt_pos; g.ltk = io.ltk; g.ltv = io.ltv; g.lk = io.ltk; g.lv = io.ltv;
            if (int rc = e.gemv("lt_bg", fam(m.lt_o8).lt_bg, g,
                                weight_bytes(m.lt_o8, F) * (256.0 * 256) +
                                    A * act * (2024 + 3 * 256 + 2 * 256 * cb + 2 * 256 + 256)))
                return rc;
        }
        // FFN up + GELU + FFN down: one launch of partial sums (f32 FFN weights), merged by
        // the head's prologue at batch 1 or by a one-workgroup merge; F16 mode: two GEMVs
        const bool ffn1 = !b16;
        if (ffn1) {
            const mp::LtFfnP lf{io.ltY, m.lt_norm_ff, m.lt_ff1, m.lt_ff2s, m.eps, io.ltp, io.lty2};
            e.add("lt_ffn", mp::K_LTFFN, &mp::OpRec::lf, lf, A * (1024.0 * 256 * 2) + A * act * (256 + mp::LT_FFN_P * 256)).dump = {};
            merge(lf);
        } else {
            g = base(cb);
            g.W = m.lt_ff1; g.Wb = m.pk_lt_ff1; g.N = 1024; g.lnw = m.lt_norm_ff; g.src = io.ltY; g.src_ld = 256;
            g.out = io.ltf; g.out_ld = 1024;
            if (int rc = e.gemv("lt_c", tb.lt_c, g, F * (1024.0 * 256) + A * act * ((256 + 1024)))) return rc;
            g = base(cb);
            g.W = m.lt_ff2; g.Wb = m.pk_lt_ff2; g.N = 256; g.src = io.ltf; g.src_ld = 1024; g.out = io.lty2;
            g.out_ld = 256; g.addsrc = io.ltY;
            if (int rc = e.gemv("lt_d", tb.lt_d, g, F * (256.0 * 1024) + A * act * ((1024 + 512)))) return rc;
        }
        // (batch 1: the FFN merge, lt_ffn_kernel's interleaved partials, is the head's prologue)
        const bool em = ffn1 && NB == 1;
        if (int rc = head(cb, em ? fam(m.lt_out8).lt_emf : fam(m.lt_out8).lt_e, em, 256))
            return rc;
    }
    mp::FinP f{io.logits, io.codes_cur, io.codes_prev, io.codes_out, io.step, io.pos, io.done, io.nframes, io.ndone,
               io.max_steps, io.ignore_eos, m.audio_bos, m.audio_eos, NB, smp, io.emit_eos, io.lt_only,
               io.lt_only ? nullptr : io.ndone + 1};
    if (!io.lt_only) { f.emb = m.audio_emb; f.pos_emb = m.dec_pos; f.x = io.x; f.pos_rows = m.dec_pos_rows; }  // the next frame's input
    e.add("finalize", mp::K_FIN, &mp::OpRec::f, f, A * act * 2024).dump = {};
    return MP_OK;
}

// One decode iteration: decoder step at pos (embedding codes_prev), LT over 8 codebooks,
// finalize. Assigns the MAGPIE_Q8DUMP slots of its Q8_0 GEMVs.
int build_iteration(mp_dev *dev, std::vector<mp::OpRec> &out) {
    const mp::Model &m = dev->m;
    const int NB = dev->NB, L = m.dec_layers;
    const bool b16 = mp::h16_mode(m.weight_mode);  // 16-bit MFMA family (bf16 or F16 weights)
    const mp::OpTable tb = mp::table_for(NB, m.weight_mode);
    const mp::OpTable &tq = mp::q8_ops(NB);
    // the family of a tensor: the Q8_0 one where the file holds it quantised
    auto fam = [&](const mp::QW &q) -> const mp::OpTable & { return q ? tq : tb; };
    // algorithmic bytes: weights at their stored width (Q8_0: 34 B per 32), activations f32
    const double F = b16 ? 2.0 : 4.0, A = 4.0, act = (double)NB;
    const bool sampling = dev->params.temperature >= 0.01f;
    const mp::Sampling smp{sampling, dev->smpcfg, dev->argeos, nullptr, dev->guided};
    const Emit e{dev, out, NB, true, mp::LtDumpP{}};
    dev->q8dump_n = 0;
    dev->q8dump_index.clear();
    auto base = [&](int l) {
        mp::GemvP g = gemv_base(m, NB, dev->step, smp, dev->params.ignore_eos);
        g.layer = l; g.nlayers = L; g.max_seq = dev->max_seq; g.pos = dev->pos; g.ndone = dev->ndone;
        return g;
    };
    // bf16 mode at 8 and 16 slots: the SA and XA split states are merged once, by the split
    // workgroups themselves through granules (sa_merge_split, xa_merge_split: each merges
    // 1 / SPLITS of its head's / slot's outputs), not by every O-projection / FFN-up
    // workgroup's prologue (196 / 245 KiB each at 16 slots); the same arithmetic, so
    // batches still reproduce single runs (at 8 slots the SA merge runs in the QKV launch)
    const bool mb16 = m.weight_mode == MP_WEIGHTS_BF16 && !dev->xa_direct;
    const bool merge_sa = mb16 && (NB >= 16 || (NB == 8 && (split_merge8() & 1)));
    const bool merge_xa = mb16 && (NB >= 16 || (NB == 8 && (split_merge8() & 2)));
    // (Q8_0: the same hand-off in the int8 MFMA launch, mp_decode_q8.hip; MAGPIE_Q8_UNFUSED=1
    // keeps the separate launches, which compute the same bits)
    const bool q8_fuse = !q8_unfused();
    // (at 16 slots too unless MAGPIE_SA16=0, sa16_fused; both forms compute the same bits)
    const bool sa16 = NB < 16 || sa16_fused(m.weight_mode);
    for (int l = 0; l < L; ++l) {
        const mp::DecLayerW &W = m.dec[l];
        mp::GemvP g = base(l);
        // LN + QKV (+ frame embedding on layer 0) + KV append   (3415-3442)
        set_weights(g, W.qkv, b16 ? m.pk_qkv[l] : nullptr, W.qkv8);
        g.N = 2304; g.lnw = W.norm_self; g.src = dev->x; g.src_ld = 768; g.out = dev->q;
        g.kc = dev->kc; g.vc = dev->vc; g.kv16 = dev->kv16;
        // the frame embedding (2746-2787) is in x already: written by the previous
        // iteration's finalize (lt_finalize_kernel), for the first frame by reset_decode_state
        // self-attention over the cache, split over keys (3457-3476); the f32 family runs
        // it in the QKV launch on a hand-off of q|k|v (EPI_QKV_SA), the others separately
        mp::AttnP a{dev->q, dev->kc, dev->vc, l, L, dev->max_seq, dev->pos, dev->kv16, dev->sa_part};
        if (merge_sa) { a.merged = dev->sa_out; a.gh = dev->sagh; set_handoff(a, dev->ndone); }
        const bool sa_in_qkv = fam(W.qkv8).qkv_sa && (!W.qkv8 || q8_fuse) && sa16;
        const double qkv_bytes = weight_bytes(W.qkv8, F) * (2304.0 * 768) + A * act * ((768 + 2304));
        if (sa_in_qkv) {
            g.sa = a; g.qh = dev->qh; set_handoff(g, dev->ndone);
            if (int rc = e.gemv("qkv_sa", fam(W.qkv8).qkv_sa, g, qkv_bytes)) return rc;
            out.back().add_sa = true;
        } else {
            if (int rc = e.gemv("qkv", fam(W.qkv8).qkv, g, qkv_bytes)) return rc;
            e.add("sa_attn", mp::K_ATTN, &mp::OpRec::a, a, -1);  // bytes: the live cache length's, computed at timing time
        }
        // O-proj + residual (3479, 3509)
        g = base(l);
        set_weights(g, W.o, b16 ? m.pk_o[l] : nullptr, W.o8);
        g.N = 768; g.resid = dev->x; g.part = dev->sa_part;
        // split-K partial tiles (MP_OPROJ_KS > 1 builds only): the plain O-projection then
        // carries a hand-off; with one slice it has none and stays timeable standalone
        if (b16 && mp::b16_oproj_ks() > 1) { g.kgh = dev->kgh; set_handoff(g, dev->ndone); }
        mp::XaP xp{dev->x, dev->xa_part, W.norm_xq, m.eps, dev->kp, dev->vp, dev->T, dev->Tmax, l, L};
        xp.q_f16 = m.weight_mode == MP_WEIGHTS_F16;
        const double xa_bytes = A * act * (768.0 + 2.0 * 768 * dev->Tmax + mp::XA_SPLITS * mp::XA_PART);
        // direct XA (Q8_0 q_net / o_net, or long texts: mp_hip_set_xa_mode): x2 materialised
        const bool xa_dir = W.xq8 || dev->xa_direct;
        const bool xa_in_oproj = tb.oproj_xa && !W.o8 && !xa_dir;
        // Q8_0 file: the whole direct Q8_0 cross-attention rides in the Q8_0 O-projection's
        // launch (EPI_RESID_XQ8): q_net workgroups on a hand-off of x1, then attention +
        // o_net workgroups on a hand-off of q (up to XQ8_QIN_NB slots: the attention
        // workgroups compute q on the hand-off of x1 themselves); x2 materialised
        // (up to 8 slots: its 48 + 20 NB workgroups are then co-resident even at one per CU,
        // so no hand-off waits on a workgroup that has not been dispatched)
        const bool xq8_in_oproj = q8_fuse && W.o8 && W.xq8 && W.xo8 && tq.oproj_xq && NB <= 8;
        if (xq8_in_oproj) {
            mp::XaQ8P xq{};
            xq.x2 = dev->x2; xq.xak = dev->xak; xq.xav = dev->xav; xq.T = dev->T; xq.Tmax = dev->Tmax;
            xq.layer = l; xq.nlayers = L; xq.wo = W.xo8.q; xq.wod = W.xo8.d;
            xq.wq = W.xq8.q; xq.wqd = W.xq8.d; xq.lnw = W.norm_xq; xq.eps = m.eps; xq.qg = dev->xqh;
            xq.qin = NB <= mp::XQ8_QIN_NB;  // small batches: q in the attention workgroups (one hand-off)
            g.xq8 = xq; g.xh = dev->xh; set_handoff(g, dev->ndone);
            if (int rc = e.gemv("oproj_xa_q8", tq.oproj_xq, g,
                                weight_bytes(W.o8, F) * (768.0 * 768) + A * act * (768 * 3) + (34.0 / 32.0) * (2.0 * 128 * 768) +
                                    A * act * (768 + 2.0 * 128 * dev->Tmax)))
                return rc;
        } else if (xa_in_oproj) {
            // f32: the fused XA rides in the O-projection's launch on a hand-off of x1
            mp::GemvFn fn = tb.oproj_xa;
            if (merge_sa) {  // the SA output merged by its split workgroups: plain rows
                g.part = nullptr; g.src = dev->sa_out; g.src_ld = 768;
                fn = tb.oproj_xa_pm;
            }
            if (merge_xa) { xp.x2 = dev->x2; xp.gh = dev->xagh; }  // x2 merged by the XA workgroups
            g.xa = xp; g.xh = dev->xh; set_handoff(g, dev->ndone);
            if (int rc = e.gemv("oproj_xa", fn, g, F * (768.0 * 768) + A * act * (768 * 3) + xa_bytes)) return rc;
        } else if (int rc = e.gemv("oproj", fam(W.o8).oproj, g,
                                   weight_bytes(W.o8, F) * (768.0 * 768) + A * act * (768 * 3))) {
            return rc;
        }
        if (xa_dir && !xq8_in_oproj) {
            // cross-attention as ggml computes it (1713-1767): q = q_net LN(x) (GEMV), then
            // x2 = x + o_net attn(q, K, V) (xa_q8_kernel / xa_f32_kernel); Q8_0 q_net / o_net
            // quantise their activations, else f32 (the bf16 mode keeps XA f32)
            g = base(l);
            set_weights(g, W.xq, nullptr, W.xq8);  // (f32 in the 16-bit modes)
            g.N = 128; g.lnw = W.norm_xq; g.src = dev->x; g.src_ld = 768; g.out = dev->xqb; g.out_ld = 128;
            const double Fx = weight_bytes(W.xq8, A);
            if (int rc = e.gemv("xq", fam(W.xq8).xq, g, Fx * (128.0 * 768) + A * act * (768 + 128))) return rc;
            mp::XaQ8P xq{};
            xq.x = dev->x; xq.x2 = dev->x2; xq.q = dev->xqb; xq.xak = dev->xak; xq.xav = dev->xav; xq.T = dev->T;
            xq.Tmax = dev->Tmax; xq.layer = l; xq.nlayers = L;
            if (W.xq8) { xq.wo = W.xo8.q; xq.wod = W.xo8.d; }
            else xq.wof = W.xo;
            e.add(W.xq8 ? "xa_q8" : "xa_dir", mp::K_XAQ8, &mp::OpRec::xq, xq,
                  Fx * (768.0 * 128) + A * act * (128.0 + 768 * 2 + 2.0 * 128 * dev->Tmax));
        } else if (!xa_in_oproj && !xq8_in_oproj) {
            // cross-attention, fused (1713-1767, 3513-3519): x2 = x + o_net(attn(q_net(LN(x))))
            e.add("xa", mp::K_XA, &mp::OpRec::x, xp, xa_bytes);
        }
        // LN + FFN up + GELU (1796-1799)
        g = base(l);
        g.W = W.ff1; g.Wb = b16 ? m.pk_ff1[l] : nullptr; g.N = 3072; g.lnw = W.norm_ff; g.out = dev->h; g.out_ld = 3072;
        if (b16) g.out_b16 = dev->h_b16;  // GELU output stored bf16 / f16 (what FFN down rounds it to)
        if (xa_dir || merge_xa) {  // x2 materialised by the direct XA / the XA tail's merge
            g.src = dev->x2; g.src_ld = 768;
            if (int rc = e.gemv("ff1", tb.ff1, g, F * (3072.0 * 768) + A * act * ((768 + 3072)))) return rc;
        } else {      // x2 = x + merged XA split states, stored by block 0 for the FFN residual
            g.src = dev->x; g.src_ld = 768; g.part = dev->xa_part; g.xres = dev->x2;
            if (int rc = e.gemv("ff1", tb.ff1x, g,
                                F * (3072.0 * 768) + A * act * (768 * 2 + 3072 + mp::XA_SPLITS * mp::XA_PART)))
                return rc;
        }
        // FFN down + residual (1805, 3525): x = x2 + W2 h
        g = base(l);
        g.W = W.ff2; g.Wb = b16 ? m.pk_ff2[l] : nullptr; g.N = 768; g.src = dev->h; g.src_ld = 3072; g.out = dev->x; g.out_ld = 768; g.addsrc = dev->x2;
        if (b16) {
            g.src = nullptr; g.src_b16 = dev->h_b16;
            // split-K partial tiles (the FFN-down half of kgh: each op its own granules)
            g.kgh = dev->kgh + (size_t)(768 / 16) * mp::KGH_MAX_KS * 256; set_handoff(g, dev->ndone);
        }
        if (int rc = e.gemv("ff2", tb.ff2, g, F * (768.0 * 3072) + A * act * ((3072 + 2 * 768)))) return rc;
    }
    mp::LtIo io{};
    io.x = dev->x; io.hidden = dev->hidden; io.trace = dev->trace; io.trace_steps = dev->max_steps + 1;
    io.lt_s = dev->lt_s; io.ltX = dev->ltX; io.ltY = dev->ltY; io.lty2 = dev->lty2; io.ltq = dev->ltq;
    io.ltk = dev->ltk; io.ltv = dev->ltv; io.ltf = dev->ltf; io.logits = dev->logits; io.ltp = dev->ltp;
    io.ltgh = dev->ltgh; io.ltfg = dev->ltfg; io.ltyg = dev->ltyg; set_handoff(io, dev->ndone);
    io.codes_cur = dev->codes_cur; io.codes_prev = dev->codes_prev; io.codes_out = dev->codes_out; io.step = dev->step;
    io.pos = dev->pos; io.done = dev->done; io.nframes = dev->nframes; io.ndone = dev->ndone; io.argeos = dev->argeos;
    io.amax = dev->amax; io.cfg = dev->smpcfg;
    io.sampling = sampling; io.ignore_eos = dev->params.ignore_eos; io.guided = dev->guided;
    io.emit_eos = dev->params.emit_eos_frame; io.max_steps = dev->max_steps; io.lt_only = false;
    return build_lt(dev, io, NB, out, true);
}

// one record, launched on s
hipError_t launch_rec(const mp::OpRec &r, hipStream_t s) {
    switch (r.kind) {
    case mp::K_GEMV: return r.fn(r.g, s);
    case mp::K_ATTN: return mp::op_sa_attn(r.a, r.B, s);
    case mp::K_XA: return mp::op_xa(r.x, r.B, s);
    case mp::K_XAQ8: return mp::op_xa_q8(r.xq, r.B, s);
    case mp::K_LTFFN: return mp::op_lt_ffn(r.lf, r.B, s);
    case mp::K_LTMERGE: return mp::op_lt_merge(r.lf, r.B, s);
    case mp::K_LTPICK: return mp::op_lt_pick(r.g, r.B, s);
    case mp::K_LTFFN2: return mp::op_lt_ffn2(r.l2, r.B, s);
    case mp::K_LTSLOT: return mp::op_lt_slot(r.l2, r.B, s);
    case mp::K_LTFRONT: return mp::op_lt_front(r.lf3, s);
    case mp::K_LTSLOTQ8: return mp::op_lt_slot_q8(r.lq8, r.B, s);
    case mp::K_LTKVO: return mp::op_lt_kvo(r.g, r.B, s);
    case mp::K_FIN: return mp::op_finalize(r.f, r.B, s);
    }
    return hipErrorInvalidValue;
}

// Diagnostics (MAGPIE_EAGER=1 and MAGPIE_DUMP_LT=file): after every launch of
// the local transformer, slot 0's LT state is appended to the file as f32
// records [logits 2024 | codes_cur 8 (int bits) | ltX | ltY | lty2 | ltq 256 each].
void dump_lt(const mp::LtDumpP &d, const char *path, hipStream_t s) {
    if (hipStreamSynchronize(s) != hipSuccess) return;
    std::vector<float> rec(2024 + 8 + 4 * 256);
    float *p = rec.data();
    auto get = [&](const void *src, size_t n) {
        if (hipMemcpy(p, src, n * 4, hipMemcpyDeviceToHost) != hipSuccess) return;
        p += n;
    };
    get(d.logits, 2024); get(d.codes_cur, 8); get(d.ltX, 256); get(d.ltY, 256); get(d.lty2, 256); get(d.ltq, 256);
    if (FILE *fp = fopen(path, "ab")) { fwrite(rec.data(), 4, rec.size(), fp); fclose(fp); }
}

// Launch a list on s: the only place outside the profiling functions that launches a
// decode kernel.
int launch_ops(mp_dev *dev, const std::vector<mp::OpRec> &ops, hipStream_t s) {
    const char *dump = eager_mode() ? getenv("MAGPIE_DUMP_LT") : nullptr;
    for (const mp::OpRec &r : ops) {
        const hipError_t err = launch_rec(r, s);
        if (err != hipSuccess) return fail(dev, MP_ERR_HIP, r.name + " failed: " + hipGetErrorString(err));
        if (dump && r.dump.logits) dump_lt(r.dump, dump, s);
    }
    return MP_OK;
}

// ------------------------------------------------------------------ preamble
// The text encoder's buffers: the batch's preamble scratch (run_preamble) or a private
// workspace (mp_hip_encode_text, which must not touch a batch in progress).
struct EncWs {
    const int32_t *tok, *T;  // device [NB][Tmax] token ids, [NB] lengths
    int NB, Tmax;
    float *pX, *pH, *pQKV, *pATT, *pF, *gpart, *enc_out;
};
static size_t enc_gpart_elems(size_t Me) {
    size_t cap = 0;
    auto need = [&](size_t M, int N, int K) { cap = std::max(cap, (size_t)mp::gemm_splits_max(K) * M * N); };
    need(Me, 2304, 768); need(Me, 3072, 768 * 3); need(Me, 768, 3072 * 3); need(Me, 256, 768);
    return cap;
}
// every preamble GEMM runs split-K over K (deterministic, batch-invariant)
// F16 file: every projection's operand rounded to f16 as ggml's F16 mul_mat does
// (the K'/V' precompute is weight algebra, not a mul_mat of the file)
static hipError_t preamble_gemm(const mp::Model &m, float *gpart, mp::GemmP gp, int epi, hipStream_t st) {
    gp.part = gpart;
    if (gp.ln_w) gp.ln_eps = m.eps;
    gp.xround = gp.xround < 0 ? 0 : (m.weight_mode == MP_WEIGHTS_F16 ? 2 : 0);  // -1: opted out
    return mp::pre_gemm(gp, epi, st);
}
// --- text encoder (magpie_build_full_encoder, 1960-1995) into w.enc_out [NB][Tmax][768]
static int run_encoder(mp_dev *dev, const EncWs &w, hipStream_t s) {
    using namespace mp;
    const Model &m = dev->m;
    const int Tmax = w.Tmax, Me = w.NB * Tmax;
    auto pre_gemm = [&](GemmP gp, int epi, hipStream_t st) { return preamble_gemm(m, w.gpart, gp, epi, st); };
    HIPCHK(pre_embed_text(w.tok, w.T, w.NB, Tmax, m.text_emb, m.enc_pos, w.pX, s));
    // the residual GEMMs (O-projection, FFN down) normalise the rows they complete for the
    // next LayerNorm (GemmP::ln_w: fused into their split reduction)
    HIPCHK(pre_ln_rows(w.pX, 768, m.enc[0].norm_self, w.pH, 768, Me, m.eps, s));
    for (int l = 0; l < m.enc_layers; ++l) {
        const EncLayerW &W = m.enc[l];
        GemmP gp{};
        gp.A = w.pH; gp.lda = 768; gp.W = W.qkv; gp.Wq = W.qkv8.q; gp.Wd = W.qkv8.d; gp.C = w.pQKV; gp.ldc = 2304; gp.M = Me; gp.N = 2304; gp.K = 768;
        gp.rows_per_utt = Tmax; gp.T = w.T;
        HIPCHK(pre_gemm(gp, GE_STORE, s));
        RowAttnP ra{};
        ra.Q = w.pQKV; ra.ldq = 2304; ra.Kb = w.pQKV + 768; ra.Vb = w.pQKV + 1536;
        ra.utt_stride = (size_t)Tmax * 2304; ra.row_stride = 2304; ra.O = w.pATT; ra.M = Me; ra.rows_per_utt = Tmax;
        ra.heads = 12; ra.T = w.T;
        HIPCHK(pre_row_attn(ra, s));
        gp = GemmP{};
        gp.A = w.pATT; gp.lda = 768; gp.W = W.o; gp.Wq = W.o8.q; gp.Wd = W.o8.d; gp.C = w.pX; gp.ldc = 768; gp.M = Me; gp.N = 768; gp.K = 768;
        gp.rows_per_utt = Tmax; gp.T = w.T;
        gp.ln_w = W.norm_ff; gp.ln_out = w.pH; gp.ln_ld = 768;
        HIPCHK(pre_gemm(gp, GE_RESID, s));
        gp = GemmP{};  // causal conv k=3 d_model -> d_ffn + GELU (1816-1869)
        gp.A = w.pH; gp.lda = 768; gp.W = W.ff1; gp.C = w.pF; gp.ldc = 3072; gp.M = Me; gp.N = 3072;
        gp.K = 768 * 3; gp.conv_taps = 3; gp.rows_per_utt = Tmax; gp.T = w.T;
        HIPCHK(pre_gemm(gp, GE_GELU, s));
        gp = GemmP{};  // causal conv k=3 d_ffn -> d_model + residual (1875-1916)
        gp.A = w.pF; gp.lda = 3072; gp.W = W.ff2; gp.C = w.pX; gp.ldc = 768; gp.M = Me; gp.N = 768;
        gp.K = 3072 * 3; gp.conv_taps = 3; gp.rows_per_utt = Tmax; gp.T = w.T;
        if (l + 1 < m.enc_layers) { gp.ln_w = m.enc[l + 1].norm_self; gp.ln_out = w.pH; }
        else { gp.ln_w = m.enc_norm_out; gp.ln_out = w.enc_out; }  // the encoder's final norm
        gp.ln_ld = 768;
        HIPCHK(pre_gemm(gp, GE_RESID, s));
    }
    return MP_OK;
}

static PreWs batch_ws(const mp_dev *dev) {
    return PreWs{dev->tok, dev->T, dev->spk, dev->NB, dev->Tmax, dev->max_seq, dev->kv16, dev->xa_direct,
                 dev->guided ? dev->B : 0,
                 dev->pX, dev->pH, dev->pQKV, dev->pATT, dev->pF, dev->pXQ, dev->pXAO, dev->gpart, dev->enc_out,
                 dev->xak, dev->xav, dev->kp, dev->vp, dev->kc, dev->vc, dev->stream};
}

int run_preamble(mp_dev *dev, const PreWs &w) {
    using namespace mp;
    const Model &m = dev->m;
    const int NB = w.NB, Tmax = w.Tmax, L = m.dec_layers;
    hipStream_t s = w.stream;
    // the slots with a text: all of them, or under guidance the conditional ones
    const int NE = w.n_text > 0 ? w.n_text : NB;
    const int Me = NE * Tmax;
    auto pre_gemm = [&](GemmP gp, int epi, hipStream_t st) { return preamble_gemm(m, w.gpart, gp, epi, st); };
    {
        const EncWs e{w.tok, w.T, NE, Tmax, w.pX, w.pH, w.pQKV, w.pATT, w.pF, w.gpart, w.enc_out};
        if (int rc = run_encoder(dev, e, s)) return rc;
    }
    // --- cross-attention K/V per layer (1663-1711): LN(encoder output) with each layer's
    //     norm_xmem, then kv_net. Layers whose tensors sit at one stride in the arena (the
    //     loader places every layer's tensors alike) run G at a time: one LN launch for G
    //     weight vectors, one batched GEMM (grid.z = G x splits) and its reduce, instead of
    //     3 launches per layer; each layer's arithmetic is its own GEMM's
    auto stride_of = [&](auto get) -> long long {  // elements between layers' tensors, or -1
        if (L == 1) return 0;
        const long long st = (long long)(get(1) - get(0));
        for (int l = 2; l < L; ++l)
            if ((long long)(get(l) - get(0)) != st * l) return -1;
        return st;
    };
    const long long s_norm = stride_of([&](int l) { return m.dec[l].norm_xmem; });
    const long long s_xkv = stride_of([&](int l) { return m.dec[l].xkv; });
    const bool q8kv = (bool)m.dec[0].xkv8;
    const long long s_xkvq = q8kv ? stride_of([&](int l) { return m.dec[l].xkv8.q; }) : 0;
    const long long s_xkvd = q8kv ? stride_of([&](int l) { return m.dec[l].xkv8.d; }) : 0;
    const size_t pf_rows = (size_t)NB * std::max(Tmax, (int)CTX);
    const int G = (s_norm >= 0 && s_xkv >= 0 && s_xkvq >= 0 && s_xkvd >= 0)
                      ? (int)std::max<size_t>(1, std::min<size_t>(L, pf_rows * 3072 / ((size_t)Me * 768)))
                      : 1;
    for (int l0 = 0; l0 < L; l0 += G) {
        const int g = std::min(G, L - l0);
        HIPCHK(pre_ln_rows_multi(w.enc_out, 768, m.dec[l0].norm_xmem, s_norm, w.pF, 768, (long long)Me * 768, Me, g,
                                 m.eps, s));
        GemmP gp{};
        gp.A = w.pF; gp.lda = 768; gp.W = m.dec[l0].xkv; gp.Wq = m.dec[l0].xkv8.q; gp.Wd = m.dec[l0].xkv8.d; gp.M = Me; gp.N = 256; gp.K = 768; gp.rows_per_utt = Tmax;
        gp.T = w.T; gp.xak = w.xak; gp.xav = w.xav; gp.layer = l0; gp.nlayers = L; gp.Tmax = Tmax;
        gp.nbatch = g; gp.wmod = g; gp.sA = (long long)Me * 768; gp.sW = s_xkv; gp.sWq = s_xkvq; gp.sWd = s_xkvd;
        HIPCHK(pre_gemm(gp, GE_XAKV, s));
    }
    // --- K'_t = W_q^T K_t, V'_t = W_o V_t per utterance and layer (decode-time fused XA;
    //     not with Q8_0 q_net / o_net, whose activations ggml quantises: unfused XA there).
    //     Every (utterance, layer) pair in one batched GEMM each (K = 128: no split): A rows
    //     at stride Tmax x 128, weights of layer (pair % L), outputs at stride Tmax x 768
    bool any_xq8 = false;
    for (int l = 0; l < L; ++l) any_xq8 |= (bool)m.dec[l].xq8;
    const long long s_xo = stride_of([&](int l) { return m.dec[l].xo; });
    if (!w.xa_direct && !any_xq8 && s_xo >= 0) {
        GemmP gp{};
        gp.A = w.xak; gp.lda = 128; gp.W = m.xq_t[0]; gp.C = w.kp; gp.ldc = 768;
        gp.M = Tmax; gp.N = 768; gp.K = 128; gp.rows_per_utt = Tmax;
        gp.xround = -1;
        gp.nbatch = NE * L; gp.wmod = L; gp.sA = (long long)Tmax * 128; gp.sW = 768 * 128; gp.sC = (long long)Tmax * 768;
        HIPCHK(pre_gemm(gp, GE_STORE, s));
        gp.A = w.xav; gp.W = m.dec[0].xo; gp.C = w.vp; gp.sW = s_xo;
        HIPCHK(pre_gemm(gp, GE_STORE, s));
    } else {
        for (int b = 0; b < NE; ++b)
            for (int l = 0; l < L; ++l) {
                if (m.dec[l].xq8 || w.xa_direct) continue;
                const size_t xo = ((size_t)(b * L + l) * Tmax) * 128, po = ((size_t)(b * L + l) * Tmax) * 768;
                GemmP gp{};
                gp.A = w.xak + xo; gp.lda = 128; gp.W = m.xq_t[l]; gp.C = w.kp + po; gp.ldc = 768;
                gp.M = Tmax; gp.N = 768; gp.K = 128; gp.rows_per_utt = Tmax;
                gp.xround = -1;
                HIPCHK(pre_gemm(gp, GE_STORE, s));
                gp.A = w.xav + xo; gp.W = m.dec[l].xo; gp.C = w.vp + po;
                HIPCHK(pre_gemm(gp, GE_STORE, s));
            }
    }
    // --- guidance: the unconditional partners' tables are zeros (an all-zero encoder output
    //     through the bias-free kv_net: K = V = 0, hence K' = V' = 0), over every row of the
    //     slot; the padding slots behind the pairs are copies of slot 0
    if (w.n_text > 0) {
        const size_t xs = (size_t)L * Tmax * 128, ps = (size_t)L * Tmax * 768;  // a slot's tables
        const bool kp = !w.xa_direct && w.kp;
        HIPCHK(hipMemsetAsync(w.xak + NE * xs, 0, NE * xs * 4, s));
        HIPCHK(hipMemsetAsync(w.xav + NE * xs, 0, NE * xs * 4, s));
        if (kp) {
            HIPCHK(hipMemsetAsync(w.kp + NE * ps, 0, NE * ps * 4, s));
            HIPCHK(hipMemsetAsync(w.vp + NE * ps, 0, NE * ps * 4, s));
        }
        for (int b = 2 * NE; b < NB; ++b) {
            HIPCHK(hipMemcpyAsync(w.xak + b * xs, w.xak, xs * 4, hipMemcpyDeviceToDevice, s));
            HIPCHK(hipMemcpyAsync(w.xav + b * xs, w.xav, xs * 4, hipMemcpyDeviceToDevice, s));
            if (kp) {
                HIPCHK(hipMemcpyAsync(w.kp + b * ps, w.kp, ps * 4, hipMemcpyDeviceToDevice, s));
                HIPCHK(hipMemcpyAsync(w.vp + b * ps, w.vp, ps * 4, hipMemcpyDeviceToDevice, s));
            }
        }
    }
    // --- baked context + 110-frame causal prefill (3991-4060, 4167-4238); a speaker of -1
    //     (a guidance partner) has no context: its rows are the positions alone
    const int Mc = NB * CTX;
    HIPCHK(pre_embed_context(w.spk, NB, m.baked, m.dec_pos, w.pX, s));
    HIPCHK(pre_ln_rows(w.pX, 768, m.dec[0].norm_self, w.pH, 768, Mc, m.eps, s));
    for (int l = 0; l < L; ++l) {
        const DecLayerW &W = m.dec[l];
        GemmP gp{};
        gp.A = w.pH; gp.lda = 768; gp.W = W.qkv; gp.Wq = W.qkv8.q; gp.Wd = W.qkv8.d; gp.C = w.pQKV; gp.ldc = 2304; gp.M = Mc; gp.N = 2304; gp.K = 768;
        gp.rows_per_utt = CTX; gp.kc = w.kc; gp.vc = w.vc; gp.kv16 = w.kv16; gp.layer = l; gp.nlayers = L;
        gp.max_seq = w.max_seq;
        HIPCHK(pre_gemm(gp, GE_QKV_CACHE, s));
        RowAttnP ra{};
        ra.Q = w.pQKV; ra.ldq = 2304;
        {   // layer l's rows, offset in cache elements (bf16 elements in MP_KV_BF16 mode)
            const size_t off = (size_t)l * w.max_seq * 768;
            ra.Kb = w.kv16 ? (const float *)((const unsigned short *)w.kc + off) : w.kc + off;
            ra.Vb = w.kv16 ? (const float *)((const unsigned short *)w.vc + off) : w.vc + off;
        }
        ra.utt_stride = (size_t)L * w.max_seq * 768; ra.row_stride = 768; ra.O = w.pATT; ra.M = Mc;
        ra.rows_per_utt = CTX; ra.heads = 12; ra.T = w.T; ra.kv16 = w.kv16;
        HIPCHK(pre_row_attn(ra, s));
        gp = GemmP{};
        gp.A = w.pATT; gp.lda = 768; gp.W = W.o; gp.Wq = W.o8.q; gp.Wd = W.o8.d; gp.C = w.pX; gp.ldc = 768; gp.M = Mc; gp.N = 768; gp.K = 768;
        gp.rows_per_utt = CTX;
        gp.ln_w = W.norm_xq; gp.ln_out = w.pH; gp.ln_ld = 768;
        HIPCHK(pre_gemm(gp, GE_RESID, s));
        gp = GemmP{};
        gp.A = w.pH; gp.lda = 768; gp.W = W.xq; gp.Wq = W.xq8.q; gp.Wd = W.xq8.d; gp.C = w.pXQ; gp.ldc = 128; gp.M = Mc; gp.N = 128; gp.K = 768;
        gp.rows_per_utt = CTX;
        HIPCHK(pre_gemm(gp, GE_STORE, s));
        RowXaP rx{w.pXQ, w.xak, w.xav, l, L, Tmax, CTX, Mc, w.T, w.pXAO};
        HIPCHK(pre_row_xa(rx, s));
        gp = GemmP{};
        gp.A = w.pXAO; gp.lda = 128; gp.W = W.xo; gp.Wq = W.xo8.q; gp.Wd = W.xo8.d; gp.C = w.pX; gp.ldc = 768; gp.M = Mc; gp.N = 768; gp.K = 128;
        gp.rows_per_utt = CTX;
        gp.ln_w = W.norm_ff; gp.ln_out = w.pH; gp.ln_ld = 768;
        HIPCHK(pre_gemm(gp, GE_RESID, s));
        gp = GemmP{};
        gp.A = w.pH; gp.lda = 768; gp.W = W.ff1; gp.C = w.pF; gp.ldc = 3072; gp.M = Mc; gp.N = 3072; gp.K = 768;
        gp.rows_per_utt = CTX;
        HIPCHK(pre_gemm(gp, GE_GELU, s));
        gp = GemmP{};
        gp.A = w.pF; gp.lda = 3072; gp.W = W.ff2; gp.C = w.pX; gp.ldc = 768; gp.M = Mc; gp.N = 768; gp.K = 3072;
        gp.rows_per_utt = CTX;
        if (l + 1 < L) { gp.ln_w = m.dec[l + 1].norm_self; gp.ln_out = w.pH; gp.ln_ld = 768; }
        HIPCHK(pre_gemm(gp, GE_RESID, s));
    }
    return MP_OK;
}

}  // namespace

// ====================================================================== C-ABI
extern "C" {

int mp_hip_device_count(int *n) {
    if (!n) return MP_ERR_ARG;
    if (hipGetDeviceCount(n) != hipSuccess) { *n = 0; return MP_ERR_HIP; }
    return MP_OK;
}

const char *mp_hip_runtime_path(void) {
    Dl_info info;
    if (dladdr((void *)&hipGetDeviceCount, &info) && info.dli_fname) return info.dli_fname;
    return "";
}

int mp_hip_init(int device, mp_dev **out) {
    if (!out) return MP_ERR_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return MP_ERR_HIP;
    mp_dev *dev = new mp_dev();
    dev->device = device;
    // the decode stream at the device's greatest priority: when the codec runs beside it (the
    // streaming loop, configs[2]'s overlapped chunks) the dispatcher serves the latency-bound
    // frame loop's workgroups first and the codec (least priority, mp_hip_codec_init) fills in
    // (MAGPIE_STREAM_PRIO=0: the default priority, A/B)
    int least = 0, greatest = 0;
    const bool prio = mp::env_int("MAGPIE_STREAM_PRIO", 1) != 0;
    if (hipSetDevice(device) != hipSuccess || hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess ||
        dev->stream.create(prio ? greatest : 0) != hipSuccess || dev->h_ndone.reserve(64) != hipSuccess) {
        delete dev;
        return MP_ERR_HIP;
    }
    *out = dev;
    return MP_OK;
}

int mp_hip_load_model_ex(mp_dev *dev, const char *path, int weight_mode) {
    if (!dev || !path) return MP_ERR_ARG;
    if (weight_mode != MP_WEIGHTS_AS_STORED && weight_mode != MP_WEIGHTS_BF16 && weight_mode != MP_WEIGHTS_Q8 &&
        weight_mode != MP_WEIGHTS_F16)
        return fail(dev, MP_ERR_ARG, "unknown weight mode");
    HIPCHK(hipSetDevice(dev->device));
    free_batch(dev);
    free_stage(dev);  // sized for the previous model's layers
    // the old model goes before the new one is allocated (peak memory: one model); from here
    // to a completed load the handle holds an empty Model
    dev->loaded = false;
    dev->m = mp::Model{};
    mp::Model m;
    if (int rc = mp::load_model(path, weight_mode, dev->stream, m, dev->err)) return rc;
    dev->m = std::move(m);
    dev->loaded = true;
    return MP_OK;
}

int mp_hip_load_model(mp_dev *dev, const char *path) { return mp_hip_load_model_ex(dev, path, MP_WEIGHTS_AS_STORED); }

int mp_hip_model_info(mp_dev *dev, int *dec_layers, int *enc_layers, size_t *weight_bytes) {
    if (!dev || !dev->loaded) return MP_ERR_STATE;
    if (dec_layers) *dec_layers = dev->m.dec_layers;
    if (enc_layers) *enc_layers = dev->m.enc_layers;
    if (weight_bytes) *weight_bytes = dev->m.arena_bytes;
    return MP_OK;
}

int mp_hip_weight_mode(mp_dev *dev) { return dev && dev->loaded ? dev->m.weight_mode : MP_ERR_STATE; }
int mp_hip_max_batch(mp_dev *dev) {
    if (!dev || !dev->loaded) return MP_ERR_STATE;
    return mp::h16_mode(dev->m.weight_mode) || (dev->m.weight_mode == MP_WEIGHTS_Q8 && dev->m.q8_all) ? 16 : 8;
}

int mp_hip_set_xa_mode(mp_dev *dev, int xa_mode) {
    if (!dev || xa_mode < MP_XA_AUTO || xa_mode > MP_XA_DIRECT) return MP_ERR_ARG;
    dev->xa_mode = xa_mode;
    return MP_OK;
}

int mp_hip_set_stream_codec_mode(mp_dev *dev, int mode) {
    if (!dev || (mode != MP_STREAM_CODEC_STATELESS && mode != MP_STREAM_CODEC_CONTINUOUS)) return MP_ERR_ARG;
    dev->stream_codec_mode = mode;
    return MP_OK;
}

int mp_hip_set_cfg(mp_dev *dev, float scale) {
    if (!dev || !std::isfinite(scale)) return MP_ERR_ARG;
    dev->cfg_scale = scale;
    return MP_OK;
}

int mp_hip_set_kv_mode(mp_dev *dev, int kv_mode) {
    if (!dev || (kv_mode != MP_KV_F32 && kv_mode != MP_KV_BF16)) return MP_ERR_ARG;
    dev->kv_mode = kv_mode;
    return MP_OK;
}

void mp_hip_free(mp_dev *dev) {
    if (!dev) return;
    hipSetDevice(dev->device);
    if (dev->stream) hipStreamSynchronize(dev->stream);
    if (dev->side) hipStreamSynchronize(dev->side);
    free_batch(dev);  // the graph; every owner releases in ~mp_dev, the streams last
    mp_hip_codec_stream_free(dev->cstream);  // its own memory only: the codec may be gone already
    delete dev;
}

const char *mp_hip_error(mp_dev *dev) { return dev ? dev->err.c_str() : "null mp_dev"; }

// mp_hip_begin_batch's argument checks, shared with mp_hip_decode_queue (which applies them
// to every utterance of its queue before anything runs): the sampling settings and the
// frame budget (max_steps receives it) ...
static int check_params(mp_dev *dev, const mp_params *params, int *max_steps) {
    if (params->temperature >= 0.01f && (params->top_k < 1 || params->top_k > mp::VCB))
        return fail(dev, MP_ERR_ARG, "top_k must be in 1..2024 when sampling");
    *max_steps = params->max_dec_steps > 0 ? params->max_dec_steps : dev->m.max_dec_steps;
    if (mp::CTX + *max_steps + 16 > mp::NCH_MAX * mp::SA_CHUNK)
        return fail(dev, MP_ERR_ARG, "max_dec_steps too large (cache limited to 1024 positions)");
    if (mp::CTX + *max_steps > dev->m.dec_pos_rows)
        return fail(dev, MP_ERR_ARG, "max_dec_steps exceeds the decoder position table");
    return MP_OK;
}
// ... and n utterances' lengths, speakers and token ids (Tmax receives the longest text)
static int check_utterances(mp_dev *dev, const int32_t *tokens, const int32_t *n_tokens, const int32_t *speaker, int n,
                            int tmax, int *Tmax_out) {
    int Tmax = 0;
    for (int b = 0; b < n; ++b) {
        if (n_tokens[b] < 1 || n_tokens[b] > tmax) return fail(dev, MP_ERR_ARG, "n_tokens out of range");
        if (speaker[b] < 0 || speaker[b] >= dev->m.n_spk) return fail(dev, MP_ERR_ARG, "speaker id out of range");
        for (int t = 0; t < n_tokens[b]; ++t)
            if (tokens[(size_t)b * tmax + t] < 0 || tokens[(size_t)b * tmax + t] >= dev->m.text_vocab)
                return fail(dev, MP_ERR_ARG, "token id out of range");
        Tmax = std::max(Tmax, (int)n_tokens[b]);
    }
    if (Tmax > mp::TMAX_LIMIT || Tmax > 4096) return fail(dev, MP_ERR_ARG, "too many text tokens");
    *Tmax_out = Tmax;
    return MP_OK;
}

// mp_hip_begin_batch. pin_tmax > 0 (the slot pool): the batch's text stride is pin_tmax,
// not its own longest text, so a later utterance of up to pin_tmax tokens fits any slot.
static int begin_batch(mp_dev *dev, const int32_t *tokens, const int32_t *n_tokens, const int32_t *speaker, int B,
                       int tmax, const mp_params *params, int pin_tmax) {
    if (!dev) return MP_ERR_ARG;
    if (!dev->loaded) return fail(dev, MP_ERR_STATE, "no model loaded");
    const int bmax = mp_hip_max_batch(dev);
    if (!tokens || !n_tokens || !speaker || B < 1 || B > bmax || tmax < 1 || !params)
        return fail(dev, MP_ERR_ARG, "invalid arguments (B must be 1..mp_hip_max_batch: 8 with f32 weights, 16 in the bf16 / F16 / Q8_0 / Q4_0 modes)");
    // classifier-free guidance (mp_hip_set_cfg): two slots per utterance
    const bool guided = dev->cfg_scale != 0.f;
    if (guided) {
        const int wm = dev->m.weight_mode;
        if (wm != MP_WEIGHTS_AS_STORED && wm != MP_WEIGHTS_BF16)
            return fail(dev, MP_ERR_UNSUPPORTED, "guidance (mp_hip_set_cfg) runs with f32 (as stored) and bf16 weights only, not in the F16 or Q8_0 / Q4_0 modes");
        if (2 * B > bmax)
            return fail(dev, MP_ERR_ARG, "under guidance an utterance takes two slots: B must be 1.." + std::to_string(bmax / 2) +
                                             " (half of mp_hip_max_batch = " + std::to_string(bmax) + ")");
    }
    int Tmax = 0, max_steps = 0;
    if (int rc = check_params(dev, params, &max_steps)) return rc;
    if (int rc = check_utterances(dev, tokens, n_tokens, speaker, B, tmax, &Tmax)) return rc;
    if (pin_tmax > 0) Tmax = std::max(Tmax, pin_tmax);
    HIPCHK(hipSetDevice(dev->device));
    const bool trace = params->trace_hidden != 0;
    const bool same = dev->NB > 0 && dev->B == B && dev->guided == guided && dev->Tmax == Tmax && dev->max_steps == max_steps &&
                      (dev->trace != nullptr) == trace && dev->params.ignore_eos == params->ignore_eos &&
                      (dev->params.temperature >= 0.01f) == (params->temperature >= 0.01f) &&
                      dev->params.emit_eos_frame == params->emit_eos_frame &&
                      dev->kv16 == (dev->kv_mode == MP_KV_BF16) && dev->xa_direct == want_xa_direct(dev, Tmax);
    dev->params = *params;
    if (!same) {
        if (int rc = alloc_batch(dev, B, guided, Tmax, max_steps, trace)) return rc;
    }
    const int NB = dev->NB, slots = dev->slots;
    auto t0 = std::chrono::steady_clock::now();
    std::vector<int> h_tok((size_t)NB * Tmax, 0), h_T(NB, 1), h_spk(NB, 0);
    for (int b = 0; b < B; ++b) {
        h_T[b] = n_tokens[b];
        h_spk[b] = speaker[b];
        for (int t = 0; t < n_tokens[b]; ++t) h_tok[(size_t)b * Tmax + t] = tokens[(size_t)b * tmax + t];
    }
    // a text-free partner: its utterance's length (zero XA rows), no speaker context (-1)
    for (int b = B; b < slots; ++b) { h_T[b] = h_T[b - B]; h_spk[b] = -1; }
    for (int b = slots; b < NB; ++b) { h_T[b] = h_T[0]; h_spk[b] = h_spk[0]; }
    HIPCHK(hipMemcpyAsync(dev->tok, h_tok.data(), h_tok.size() * 4, hipMemcpyHostToDevice, dev->stream));
    HIPCHK(hipMemcpyAsync(dev->T, h_T.data(), NB * 4, hipMemcpyHostToDevice, dev->stream));
    HIPCHK(hipMemcpyAsync(dev->spk, h_spk.data(), NB * 4, hipMemcpyHostToDevice, dev->stream));
    {   // sampling settings live on the device: the captured graph serves any of them
        mp::SmpCfg cfg{params->temperature, params->top_k, (unsigned long long)params->seed, params->stream_base, {},
                       dev->cfg_scale, {}};
        for (int b = 0; b < 16; ++b) { cfg.stream[b] = params->stream_base + b; cfg.partner[b] = -1; }
        if (guided)  // the pair draws from the utterance's stream
            for (int b = 0; b < B; ++b) { cfg.partner[b] = B + b; cfg.partner[B + b] = b; cfg.stream[B + b] = cfg.stream[b]; }
        HIPCHK(hipMemcpyAsync(dev->smpcfg, &cfg, sizeof cfg, hipMemcpyHostToDevice, dev->stream));
        HIPCHK(hipMemsetAsync(dev->argeos, 0, NB * 4, dev->stream));
    }
    if (int rc = run_preamble(dev, batch_ws(dev))) return rc;
    HIPCHK(hipStreamSynchronize(dev->stream));
    dev->timing = mp_timing{};
    dev->timing.preamble_ms = ms_since(t0);
    dev->batch_ready = true;
    return MP_OK;
}

int mp_hip_begin_batch(mp_dev *dev, const int32_t *tokens, const int32_t *n_tokens, const int32_t *speaker, int B,
                       int tmax, const mp_params *params) {
    return begin_batch(dev, tokens, n_tokens, speaker, B, tmax, params, 0);
}

// magpie_encode_text (magpie.cpp:2284-2374) on its own: the text encoder of one
// utterance into a private device workspace (kept on the mp_dev, grown on demand), the
// output copied to enc_out [n_tokens][768]. A batch in progress is not touched.
int mp_hip_encode_text(mp_dev *dev, const int32_t *tokens, int n_tokens, float *enc_out) {
    if (!dev) return MP_ERR_ARG;
    if (!dev->loaded) return fail(dev, MP_ERR_STATE, "no model loaded");
    if (!tokens || !enc_out || n_tokens < 1) return fail(dev, MP_ERR_ARG, "invalid arguments");
    if (n_tokens > mp::TMAX_LIMIT || n_tokens > 4096) return fail(dev, MP_ERR_ARG, "too many text tokens");
    for (int t = 0; t < n_tokens; ++t)
        if (tokens[t] < 0 || tokens[t] >= dev->m.text_vocab) return fail(dev, MP_ERR_ARG, "token id out of range");
    HIPCHK(hipSetDevice(dev->device));
    const size_t M = (size_t)n_tokens, D = 768;
    const size_t nf = M * D * 4 + M * 3 * D + M * 3072 + enc_gpart_elems(M) + M * D;  // pX pH pATT enc_out | pQKV | pF | gpart
    const size_t need = nf * 4 + 64 + M * 4;  // floats | T (64 B slot) | token ids
    if (dev->enc_ws_bytes < need) {
        // the old workspace may still be read by this stream's earlier encode: wait for it
        // (the stream only, not the device) before it goes
        HIPCHK(hipStreamSynchronize(dev->stream));
        dev->enc_ws_mem.clear();
        dev->enc_ws = nullptr;
        dev->enc_ws_bytes = 0;
        HIPCHK(dev->enc_ws_mem.bytes(&dev->enc_ws, need));
        dev->enc_ws_bytes = need;
    }
    char *ws = dev->enc_ws;
    float *f = (float *)ws;
    EncWs w{};
    w.NB = 1; w.Tmax = n_tokens;
    w.pX = f; f += M * D; w.pH = f; f += M * D; w.pATT = f; f += M * D; w.enc_out = f; f += M * D;
    w.pQKV = f; f += M * 3 * D; w.pF = f; f += M * 3072; w.gpart = f; f += enc_gpart_elems(M);
    int32_t *ti = (int32_t *)(ws + nf * 4 + 64);
    int32_t *Ti = (int32_t *)(ws + nf * 4);
    w.tok = ti; w.T = Ti;
    HIPCHK(hipMemcpyAsync(ti, tokens, M * 4, hipMemcpyHostToDevice, dev->stream));
    HIPCHK(hipMemcpyAsync(Ti, &n_tokens, 4, hipMemcpyHostToDevice, dev->stream));
    if (int rc = run_encoder(dev, w, dev->stream)) {
        hipStreamSynchronize(dev->stream);  // the host token copies above must land first
        return rc;
    }
    HIPCHK(hipMemcpyAsync(enc_out, w.enc_out, M * D * 4, hipMemcpyDeviceToHost, dev->stream));
    HIPCHK(hipStreamSynchronize(dev->stream));
    return MP_OK;
}

// Per-decode device state: BOS frame at position 110 (magpie.cpp:4243-4318).
int reset_decode_state(mp_dev *dev) {
    const int NB = dev->NB, B = dev->slots;  // a guided pair's two slots are both live
    std::vector<int> h_pos(NB, mp::CTX), h_zero(NB, 0), h_done(NB, 0), h_prev((size_t)NB * 8, dev->m.audio_bos);
    for (int b = B; b < NB; ++b) h_done[b] = 1;
    int h_nd[4] = {NB - B, 0, 0, 0};
    HIPCHK(hipMemcpyAsync(dev->pos, h_pos.data(), NB * 4, hipMemcpyHostToDevice, dev->stream));
    HIPCHK(hipMemcpyAsync(dev->step, h_zero.data(), NB * 4, hipMemcpyHostToDevice, dev->stream));
    HIPCHK(hipMemcpyAsync(dev->nframes, h_zero.data(), NB * 4, hipMemcpyHostToDevice, dev->stream));
    HIPCHK(hipMemcpyAsync(dev->done, h_done.data(), NB * 4, hipMemcpyHostToDevice, dev->stream));
    HIPCHK(hipMemcpyAsync(dev->ndone, h_nd, 16, hipMemcpyHostToDevice, dev->stream));
    HIPCHK(hipMemcpyAsync(dev->codes_prev, h_prev.data(), h_prev.size() * 4, hipMemcpyHostToDevice, dev->stream));
    HIPCHK(hipMemsetAsync(dev->codes_out, 0, (size_t)NB * dev->max_steps * 8 * 4, dev->stream));
    HIPCHK(hipMemsetAsync(dev->argeos, 0, NB * 4, dev->stream));
    // hand-off tags restart with the iteration counter (ndone[1]): no stale tag may match
    for (const auto &g : dev->granules) HIPCHK(hipMemsetAsync(g.first, 0, g.second * 8, dev->stream));
    // the first frame's decoder input (the BOS codes); later frames' by lt_finalize_kernel
    HIPCHK(mp::op_embed(mp::EmbP{dev->m.audio_emb, dev->codes_prev, dev->m.dec_pos, dev->pos, dev->x}, NB, dev->stream));
    // the host copies are stack/heap temporaries: finish the uploads before they go
    HIPCHK(hipStreamSynchronize(dev->stream));
    return MP_OK;
}


// Build the iteration's launch list and capture it into the graph (or, eager, launch it
// once) once per batch configuration; leaves the decode state reset.
int prepare_iteration(mp_dev *dev) {
    const bool fresh = dev->ops.empty();
    if (fresh) {
        if (int rc = build_iteration(dev, dev->ops)) { dev->ops.clear(); return rc; }
    }
    if (eager_mode()) {
        if (fresh) {
            // a real first iteration, on a reset state: at a fresh batch's zeroed position
            // it would append its K/V over row 0 of the prefilled cache
            if (int rc = reset_decode_state(dev)) return rc;
            if (int rc = launch_ops(dev, dev->ops, dev->stream)) return rc;
            HIPCHK(hipStreamSynchronize(dev->stream));
        }
    } else if (!dev->exec) {
        HIPCHK(hipStreamBeginCapture(dev->stream, hipStreamCaptureModeThreadLocal));
        int rc = launch_ops(dev, dev->ops, dev->stream);
        hipGraph_t g = nullptr;
        hipError_t e = hipStreamEndCapture(dev->stream, &g);
        if (rc != MP_OK) { if (g) hipGraphDestroy(g); return rc; }
        if (e != hipSuccess) return fail(dev, MP_ERR_HIP, std::string("graph capture failed: ") + hipGetErrorString(e));
        dev->graph = g;
        HIPCHK(hipGraphInstantiate(&dev->exec, dev->graph, nullptr, nullptr, 0));
    }
    return reset_decode_state(dev);
}

int launch_iteration(mp_dev *dev, hipStream_t s = nullptr) {
    if (!s) s = dev->stream;
    if (eager_mode()) return launch_ops(dev, dev->ops, s);
    HIPCHK(hipGraphLaunch(dev->exec, s));
    return MP_OK;
}

// An in-launch hand-off that gave up (EPI_RESID_XA's bounded sweep) poisons its
// output and raises ndone[2]: report it instead of returning those codes.
static int handoff_bits(mp_dev *dev, int bits) {  // ndone[2] as read by the caller
    if (bits) {
        std::string what;
        if (bits & mp::HX_ERR_XA) what += " O-projection -> cross-attention";
        if (bits & mp::HX_ERR_SA) what += std::string(what.empty() ? "" : ",") + " QKV -> self-attention";
        if (bits & mp::HX_ERR_LT) what += std::string(what.empty() ? "" : ",") + " LT FFN partial sums";
        if (bits & mp::HX_ERR_KS) what += std::string(what.empty() ? "" : ",") + " split-K partial tiles";
        return fail(dev, MP_ERR_HIP, "in-launch hand-off timed out:" + what);
    }
    return MP_OK;
}
static int check_handoff(mp_dev *dev) {
    int nd[4] = {0, 0, 0, 0};
    HIPCHK(hipMemcpy(nd, dev->ndone, sizeof nd, hipMemcpyDeviceToHost));
    return handoff_bits(dev, nd[2]);
}

// The end of an event-timed loop: e1 recorded behind it and waited for, the device time
// e0 -> e1 and the counts into dev->timing
static int end_timing(mp_dev *dev, hipEvent_t e0, hipEvent_t e1, int iterations, int frames) {
    HIPCHK(hipEventRecord(e1, dev->stream));
    HIPCHK(hipEventSynchronize(e1));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    dev->timing.decode_ms = ms;
    dev->timing.frames_total = frames;
    dev->timing.iterations = iterations;
    return MP_OK;
}

int mp_hip_decode(mp_dev *dev, int32_t *codes_out, int32_t *n_frames) {
    if (!dev) return MP_ERR_ARG;
    if (!dev->batch_ready) return fail(dev, MP_ERR_STATE, "mp_hip_begin_batch must precede mp_hip_decode");
    HIPCHK(hipSetDevice(dev->device));
    const int NB = dev->NB, B = dev->B;
    if (int rc = prepare_iteration(dev)) return rc;
    mp::Event e0, e1;
    HIPCHK(e0.create());
    HIPCHK(e1.create());
    HIPCHK(hipEventRecord(e0, dev->stream));
    // one graph replay per frame: capturing 4 to 64 iterations per graph measured the same
    // frames/s (2619 vs 2617-2626, tools_dev/graph_iters_ab.py), replay boundaries cost nothing
    const int poll = 8;  // the host checks the done counter every `poll` iterations
    int it = 0;
    while (it < dev->max_steps) {
        if (int rc = launch_iteration(dev)) return rc;
        ++it;
        if (!dev->params.ignore_eos && it % poll == 0 && it < dev->max_steps) {
            HIPCHK(hipMemcpyAsync(dev->h_ndone.p, dev->ndone, 4, hipMemcpyDeviceToHost, dev->stream));
            HIPCHK(hipStreamSynchronize(dev->stream));
            if (*dev->h_ndone.as<int>() >= NB) break;
        }
    }
    if (int rc = end_timing(dev, e0, e1, it, 0)) return rc;  // (the frames: below, once they are read)
    if (int rc = check_handoff(dev)) return rc;
    std::vector<int> h_nf(NB);
    HIPCHK(hipMemcpy(h_nf.data(), dev->nframes, NB * 4, hipMemcpyDeviceToHost));
    std::vector<int> h_codes((size_t)NB * dev->max_steps * 8);
    HIPCHK(hipMemcpy(h_codes.data(), dev->codes_out, h_codes.size() * 4, hipMemcpyDeviceToHost));
    int total = 0;
    for (int b = 0; b < B; ++b) {
        if (n_frames) n_frames[b] = h_nf[b];
        total += h_nf[b];
    }
    if (codes_out) memcpy(codes_out, h_codes.data(), (size_t)B * dev->max_steps * 8 * 4);
    dev->timing.frames_total = total;
    return MP_OK;
}

// ---------------------------------------------------------------- slot pool
// the decode reads K' / V' (reassociated XA): not in the direct form, nor in a layer whose
// q_net / o_net are Q8_0 (every layer of the converter's Q8_0 files)
static bool batch_reads_kp(const mp_dev *dev) {
    if (!dev->kp) return false;
    for (const mp::DecLayerW &W : dev->m.dec)
        if (!W.xq8) return true;
    return false;
}
// The pool's two staging workspaces: one utterance (NB = 1) of up to tmax tokens each, in
// the current batch's SA cache type and XA form; the cache holds the CTX prefill rows in
// whole SA chunks. Kept on the mp_dev while that shape holds.
static int ensure_stage(mp_dev *dev, int tmax) {
    if (dev->stage_tmax == tmax && dev->stage_kv16 == dev->kv16 && dev->stage_direct == dev->xa_direct) return MP_OK;
    free_stage(dev);
    HIPCHK(dev->side.create());
    const size_t L = dev->m.dec_layers, D = 768, T = tmax;
    const int smax_seq = (mp::CTX + mp::SA_CHUNK - 1) / mp::SA_CHUNK * mp::SA_CHUNK;
    const size_t kvn = L * smax_seq * D / (dev->kv16 ? 2 : 1);
    // (not zero-filled: the preamble writes every row the install reads)
    auto fill = [&](StageWs &s) -> hipError_t {
        PreWs &w = s.w;
        float **const pre[8] = {&w.pX, &w.pH, &w.pQKV, &w.pATT, &w.pF, &w.pXQ, &w.pXAO, &w.enc_out};
        hipError_t e;
        if ((e = s.mem.get(&s.tok, T)) || (e = s.mem.get(&s.T, 1)) || (e = s.mem.get(&s.spk, 1)) ||
            (e = alloc_pre_scratch(s.mem, pre, std::max(tmax, (int)mp::CTX), T, nullptr)) ||
            (e = s.mem.get(&w.gpart, pre_gpart_elems(T, mp::CTX, (int)L))) || (e = s.mem.get(&w.xak, L * T * 128)) ||
            (e = s.mem.get(&w.xav, L * T * 128)) || (e = s.mem.get(&w.kc, kvn)) || (e = s.mem.get(&w.vc, kvn)) ||
            (batch_reads_kp(dev) && ((e = s.mem.get(&w.kp, L * T * D)) || (e = s.mem.get(&w.vp, L * T * D)))) ||
            (e = s.pin.reserve((T + 2) * 4)) || (e = s.ready.create(hipEventDisableTiming)) ||
            (e = s.installed.create(hipEventDisableTiming)))
            return e;
        w.tok = s.tok; w.T = s.T; w.spk = s.spk;
        w.NB = 1; w.Tmax = tmax; w.max_seq = smax_seq; w.kv16 = dev->kv16; w.xa_direct = dev->xa_direct;
        w.stream = dev->side;
        return hipSuccess;
    };
    for (StageWs &s : dev->stage)
        if (hipError_t e = fill(s)) {
            free_stage(dev);
            return fail(dev, MP_ERR_HIP, std::string("slot pool: staging workspace allocation failed: ") + hipGetErrorString(e));
        }
    dev->stage_tmax = tmax;
    dev->stage_kv16 = dev->kv16;
    dev->stage_direct = dev->xa_direct;
    return MP_OK;
}

// One run of the pool (mp_hip_decode_queue, which checks the arguments and cleans up)
struct PoolRun {
    const int32_t *tokens, *n_tokens, *speaker;
    int N, tmax, slots, poll;
    mp_params params;
    mp_next_cb next;
    mp_done_cb done;
    void *user;
    int seq = 0;
    bool drained = false;
    std::vector<char> claimed;
    int cur = 0;          // the staging workspace the next install reads
    bool staged = false;  // ... holds an utterance: one is always staged ahead while any remain
    mp::Pinned h;  // [ndone 4 | done 16 | nframes 16 | codes max_steps x 8]
    mp::Event e0, e1;
    mp_queue_stats st{};
};
// the next utterance to run (-1: drained; out: MP_OK or an error)
static int pool_claim(mp_dev *dev, PoolRun &r, int *utt) {
    *utt = -1;
    if (r.drained) return MP_OK;
    const int u = r.next ? r.next(r.user) : (r.seq < r.N ? r.seq++ : -1);
    if (u < 0) { r.drained = true; return MP_OK; }
    if (u >= r.N) return fail(dev, MP_ERR_ARG, "next: utterance index out of range");
    if (r.claimed[u]) return fail(dev, MP_ERR_ARG, "next: utterance claimed twice");
    r.claimed[u] = 1;
    *utt = u;
    return MP_OK;
}
// utterance utt's preamble into s on the side stream, as a single run computes it
// (NB = 1, Tmax = its own length)
static int pool_stage(mp_dev *dev, PoolRun &r, StageWs &s, int utt) {
    if (s.install_pending) {  // the install that read this workspace must have completed
        HIPCHK(hipEventSynchronize(s.installed));
        s.install_pending = false;
    }
    const int n = r.n_tokens[utt];
    int32_t *const h = s.pin.as<int32_t>();
    memcpy(h, r.tokens + (size_t)utt * r.tmax, (size_t)n * 4);
    h[r.tmax] = n;
    h[r.tmax + 1] = r.speaker[utt];
    HIPCHK(hipMemcpyAsync(s.tok, h, (size_t)n * 4, hipMemcpyHostToDevice, dev->side));
    HIPCHK(hipMemcpyAsync(s.T, h + r.tmax, 4, hipMemcpyHostToDevice, dev->side));
    HIPCHK(hipMemcpyAsync(s.spk, h + r.tmax + 1, 4, hipMemcpyHostToDevice, dev->side));
    PreWs w = s.w;
    w.Tmax = n;
    if (int rc = run_preamble(dev, w)) return rc;
    HIPCHK(hipEventRecord(s.ready, dev->side));
    s.utt = utt;
    s.n = n;
    return MP_OK;
}
// slot b becomes the staged utterance: the decode stream waits for its preamble in-stream
static int pool_install(mp_dev *dev, PoolRun &r, StageWs &s, int b) {
    HIPCHK(hipStreamWaitEvent(dev->stream, s.ready, 0));
    mp::InstallP p{};
    p.skc = (const uint4 *)s.w.kc; p.svc = (const uint4 *)s.w.vc; p.kc = (uint4 *)dev->kc; p.vc = (uint4 *)dev->vc;
    p.nlayers = dev->m.dec_layers; p.smax_seq = s.w.max_seq; p.max_seq = dev->max_seq;
    p.cache_row16 = 768 * (dev->kv16 ? 2 : 4) / 16;
    p.sxak = (const uint4 *)s.w.xak; p.sxav = (const uint4 *)s.w.xav; p.xak = (uint4 *)dev->xak; p.xav = (uint4 *)dev->xav;
    if (batch_reads_kp(dev)) { p.skp = (const uint4 *)s.w.kp; p.svp = (const uint4 *)s.w.vp; p.kp = (uint4 *)dev->kp; p.vp = (uint4 *)dev->vp; }
    p.T = s.n; p.Tmax = dev->Tmax;
    p.b = b; p.spk = r.speaker[s.utt]; p.stream = r.params.stream_base + s.utt;
    p.audio_bos = dev->m.audio_bos; p.max_steps = dev->max_steps;
    p.Tn = dev->T; p.spkn = dev->spk; p.pos = dev->pos; p.step = dev->step; p.done = dev->done; p.nframes = dev->nframes;
    p.argeos = dev->argeos; p.codes_prev = dev->codes_prev; p.codes_out = dev->codes_out; p.ndone = dev->ndone;
    p.cfg = dev->smpcfg; p.emb = dev->m.audio_emb; p.pos_emb = dev->m.dec_pos; p.x = dev->x;
    if (b >= dev->B || s.n > dev->Tmax || s.w.kv16 != dev->kv16 || (dev->kp != nullptr) == s.w.xa_direct)
        return fail(dev, MP_ERR_STATE, "slot pool: staged utterance does not fit the batch");
    HIPCHK(mp::op_slot_install(p, dev->stream));
    HIPCHK(hipEventRecord(s.installed, dev->stream));
    s.install_pending = true;
    s.utt = -1;
    return MP_OK;
}

// the next claimed utterance's preamble into workspace ws (nothing once the queue is drained)
static int pool_stage_next(mp_dev *dev, PoolRun &r, int ws) {
    int u;
    if (int rc = pool_claim(dev, r, &u)) return rc;
    if (u < 0) return MP_OK;
    if (int rc = ensure_stage(dev, r.tmax)) return rc;
    if (int rc = pool_stage(dev, r, dev->stage[ws], u)) return rc;
    r.cur = ws;
    r.staged = true;
    return MP_OK;
}
// slot b takes the staged utterance, and the one after it is staged
static int pool_refill(mp_dev *dev, PoolRun &r, std::vector<int> &occ, int b) {
    StageWs &s = dev->stage[r.cur];
    occ[b] = s.utt;
    ++r.st.refills;
    r.staged = false;
    if (int rc = pool_install(dev, r, s, b)) return rc;
    return pool_stage_next(dev, r, r.cur ^ 1);
}
// The first `slots` claimed utterances: an ordinary batch at text stride tmax, its iteration
// prepared and the next utterance staged. occ: the utterance of each slot (empty: nothing to run).
static int pool_start(mp_dev *dev, PoolRun &r, std::vector<int> &occ) {
    for (int b = 0; b < r.slots; ++b) {
        int u;
        if (int rc = pool_claim(dev, r, &u)) return rc;
        if (u < 0) break;
        occ.push_back(u);
    }
    const int B = (int)occ.size();
    r.st.slots = B;
    if (B == 0) return MP_OK;
    {
        std::vector<int32_t> tok((size_t)B * r.tmax, 0), nt(B), spk(B);
        for (int b = 0; b < B; ++b) {
            nt[b] = r.n_tokens[occ[b]];
            spk[b] = r.speaker[occ[b]];
            memcpy(&tok[(size_t)b * r.tmax], r.tokens + (size_t)occ[b] * r.tmax, (size_t)nt[b] * 4);
        }
        if (int rc = begin_batch(dev, tok.data(), nt.data(), spk.data(), B, r.tmax, &r.params, r.tmax)) return rc;
        // the draw streams follow the utterances, not the slots
        mp::SmpCfg cfg{r.params.temperature, r.params.top_k, (unsigned long long)r.params.seed, r.params.stream_base, {}, 0.f, {}};
        for (int b = 0; b < 16; ++b) { cfg.stream[b] = r.params.stream_base + (b < B ? occ[b] : b); cfg.partner[b] = -1; }
        HIPCHK(hipMemcpyAsync(dev->smpcfg, &cfg, sizeof cfg, hipMemcpyHostToDevice, dev->stream));
        HIPCHK(hipStreamSynchronize(dev->stream));
    }
    dev->batch_ready = false;  // the pool owns the batch: mp_hip_decode needs a new mp_hip_begin_batch
    if (int rc = prepare_iteration(dev)) return rc;
    return pool_stage_next(dev, r, 0);
}

static int pool_run(mp_dev *dev, PoolRun &r) {
    std::vector<int> occ;  // utterance of each slot, -1 once handed out
    if (int rc = pool_start(dev, r, occ)) return rc;
    const int B = (int)occ.size();
    if (B == 0) return MP_OK;
    const int NB = dev->NB, S = dev->max_steps;
    HIPCHK(r.h.reserve((size_t)(36 + S * 8) * 4));
    int32_t *h_nd = r.h.as<int32_t>(), *h_done = h_nd + 4, *h_nf = h_nd + 20, *h_codes = h_nd + 36;
    HIPCHK(r.e0.create());
    HIPCHK(r.e1.create());
    HIPCHK(hipEventRecord(r.e0, dev->stream));
    int it = 0, live = B;
    // every utterance leaves its slot within max_steps iterations and a poll round
    const long long it_max = ((long long)r.N + 1) * ((long long)S + r.poll);
    while (live > 0) {
        if (it >= it_max) return fail(dev, MP_ERR_STATE, "slot pool: a slot never finished");
        if (int rc = launch_iteration(dev)) return rc;
        ++it;
        if (it % r.poll != 0) continue;
        HIPCHK(hipMemcpyAsync(h_nd, dev->ndone, 16, hipMemcpyDeviceToHost, dev->stream));
        HIPCHK(hipMemcpyAsync(h_done, dev->done, NB * 4, hipMemcpyDeviceToHost, dev->stream));
        HIPCHK(hipMemcpyAsync(h_nf, dev->nframes, NB * 4, hipMemcpyDeviceToHost, dev->stream));
        HIPCHK(hipStreamSynchronize(dev->stream));
        if (int rc = handoff_bits(dev, h_nd[2])) return rc;  // before any codes are returned
        for (int b = 0; b < B; ++b) {
            if (occ[b] < 0 || !h_done[b]) continue;
            const int nf = h_nf[b];
            if (nf > 0) {
                HIPCHK(hipMemcpyAsync(h_codes, dev->codes_out + (size_t)b * S * 8, (size_t)nf * 32, hipMemcpyDeviceToHost,
                                      dev->stream));
                HIPCHK(hipStreamSynchronize(dev->stream));
            }
            if (r.done) r.done(occ[b], h_codes, nf, r.user);
            r.st.useful_slot_iters += nf;
            occ[b] = -1;
            --live;
            if (!r.staged) continue;
            ++live;
            if (int rc = pool_refill(dev, r, occ, b)) return rc;
        }
    }
    if (int rc = end_timing(dev, r.e0, r.e1, it, (int)r.st.useful_slot_iters)) return rc;
    r.st.iterations = it;
    r.st.decode_ms = dev->timing.decode_ms;
    return MP_OK;
}

// Both pool calls: the arguments checked before anything runs, `run` on a PoolRun, and nothing
// of the run left in flight whatever its end (a refused call leaves the device usable)
static int pool_call(mp_dev *dev, const int32_t *tokens, const int32_t *n_tokens, const int32_t *speaker, int N, int tmax,
                     int slots, int poll, const mp_params *params, mp_next_cb next, mp_done_cb done, void *user,
                     mp_queue_stats *stats, const std::function<int(PoolRun &)> &run) {
    if (dev->cfg_scale != 0.f)
        return fail(dev, MP_ERR_UNSUPPORTED, "the slot pool does not run under guidance (mp_hip_set_cfg): a refill would have to install a pair");
    const int bmax = mp_hip_max_batch(dev);
    if (!tokens || !n_tokens || !speaker || N < 1 || tmax < 1 || !params)
        return fail(dev, MP_ERR_ARG, "invalid arguments");
    if (slots < 1 || slots > bmax)
        return fail(dev, MP_ERR_ARG, "invalid arguments (slots must be 1..mp_hip_max_batch: 8 with f32 weights, 16 in the bf16 / F16 / Q8_0 / Q4_0 modes)");
    if (params->trace_hidden) return fail(dev, MP_ERR_ARG, "trace_hidden is not available with a slot pool");
    int Tmax = 0, max_steps = 0;
    if (int rc = check_params(dev, params, &max_steps)) return rc;
    if (int rc = check_utterances(dev, tokens, n_tokens, speaker, N, tmax, &Tmax)) return rc;
    HIPCHK(hipSetDevice(dev->device));
    PoolRun r{tokens, n_tokens, speaker, N, tmax, slots, poll, *params, next, done, user};  // released on return
    r.claimed.assign(N, 0);
    const int rc = run(r);
    hipStreamSynchronize(dev->stream);
    if (dev->side) hipStreamSynchronize(dev->side);
    for (StageWs &s : dev->stage) { s.install_pending = false; s.utt = -1; }
    if (rc == MP_OK && stats) *stats = r.st;
    return rc;
}

int mp_hip_decode_queue(mp_dev *dev, const int32_t *tokens, const int32_t *n_tokens, const int32_t *speaker, int N,
                        int tmax, int slots, int poll, const mp_params *params, mp_next_cb next, mp_done_cb done,
                        void *user, mp_queue_stats *stats) {
    if (!dev) return MP_ERR_ARG;
    if (stats) *stats = mp_queue_stats{};
    if (!dev->loaded) return fail(dev, MP_ERR_STATE, "no model loaded");
    return pool_call(dev, tokens, n_tokens, speaker, N, tmax, slots, poll > 0 ? poll : 8, params, next, done, user, stats,
                     [&](PoolRun &r) { return pool_run(dev, r); });
}

// ---------------------------------------------------------------- streaming
// Both streaming drivers (mp_hip_decode_stream: one batch; pool_stream_run: the slot pool) run
// rounds of up to frames_per_chunk graph replays. Behind a round's replays, on the decode
// stream, the codes it wrote and a snapshot [ndone 4 | step | done | nframes] go to a pinned
// host mirror and an event is recorded: the host never waits inside a copy. When a round has
// landed the driver queues the next one and only then sends the landed round's chunks, at
// most one per slot, through the codec, so the decode runs on its stream while the codec runs
// on the codec's (bit-exact beside it: tests/test_concurrency_gpu.py). Slot b decodes on lane
// b of the device's codec stream. A stop requested by a callback takes effect after the round
// already queued, whose frames of that utterance are then not delivered.
// MAGPIE_STREAM_ASYNC=0: queue each chunk from the calling thread (default 1: a helper thread)
static bool stream_async() { return mp::env_int("MAGPIE_STREAM_ASYNC", 1) != 0; }
// MAGPIE_STREAM_TRACE=1: host-side timeline of the streaming loop on stderr (diagnostics)
static bool stream_trace() { return mp::env_int("MAGPIE_STREAM_TRACE", 0) != 0; }
// rounds of at least this many frames queue the next chunk from the helper thread
// (throughput: configs[2]'s 16 slots x 32-frame chunks); smaller rounds (a stream's 4-frame
// chunks, whose first chunk is the time to first audio) queue it from the calling thread
constexpr int STREAM_ASYNC_MIN_FRAMES = 256;

namespace {
// A slot's entry of a round: a chunk of n frames from frame f0 (n = 0: none) of utterance
// utt, in slot and on codec lane b; ended: the utterance ends with it. at: where decode()
// put the chunk's samples in StreamRun::audio.
struct Job { int b, utt, f0, n; bool ended; size_t at; };
// a landed round: the codes mirror [NB][S][8] and the snapshot, as enqueue() filled them
struct Snap { const int32_t *codes, *nd, *step, *done, *nf; };

struct StreamRun {
    mp_dev *dev;
    mp_codec *codec;
    int fpc;
    mp_audio_cb on_audio;
    void *user;
    bool cont = false;  // continuous codec: the lanes carry their state from chunk to chunk
    // the pinned mirror: [codes NB x S x 8] x mirrors, then two snapshots of 4 + 3 NB
    int NB = 0, S = 0, mirrors = 1;
    std::vector<int> delivered, stopped;  // per slot: frames handed out; the callback declined
    std::vector<int32_t> cbm, ids, lens;  // codec staging: codebook-major codes, lanes, lengths
    std::vector<float> audio;
    bool first = true;  // no audio delivered yet
    std::chrono::steady_clock::time_point t0;

    int codec_fail(int rc) { return fail(dev, rc, std::string("codec: ") + mp_hip_codec_error(codec)); }
    size_t ncodes() const { return (size_t)NB * S * 8; }
    int32_t *codes(int k) const { return dev->h_codes_pin.as<int32_t>() + (size_t)(k % mirrors) * ncodes(); }
    int32_t *snap(int k) const { return dev->h_codes_pin.as<int32_t>() + mirrors * ncodes() + (size_t)k * (4 + 3 * NB); }
    Snap view(int k) const {
        const int32_t *s = snap(k);
        return {codes(k), s, s + 4, s + 4 + NB, s + 4 + 2 * NB};
    }

    // B slots of the prepared batch: codec lanes at the start of an utterance, the events and
    // the mirror (one codes mirror, or one per snapshot), the timing reset, the clock started
    int open(int B, int codes_mirrors) {
        NB = dev->NB; S = dev->max_steps; mirrors = codes_mirrors;
        cont = dev->stream_codec_mode == MP_STREAM_CODEC_CONTINUOUS;
        if (cont) {
            if (!dev->cstream || dev->cstream_codec != codec || dev->cstream_lanes < B) {
                mp_hip_codec_stream_free(dev->cstream);
                dev->cstream = nullptr;
                if (int rc = mp_hip_codec_stream_create(codec, B, &dev->cstream)) return codec_fail(rc);
                dev->cstream_codec = codec;
                dev->cstream_lanes = B;
            }
            if (int rc = mp_hip_codec_stream_reset(dev->cstream, -1)) return codec_fail(rc);
        }
        for (mp::Event &e : dev->sev) HIPCHK(e.create(hipEventDisableTiming));
        // pinned: a copy into pageable memory would block the host until the round's kernels finish
        HIPCHK(dev->h_codes_pin.reserve((mirrors * ncodes() + 2 * (4 + 3 * (size_t)NB)) * 4));
        delivered.assign(B, 0);
        stopped.assign(B, 0);
        dev->timing = mp_timing{dev->timing.preamble_ms, 0.0, 0, 0, 0.0};
        t0 = std::chrono::steady_clock::now();
        return MP_OK;
    }

    // A round on the decode stream: n_it replays, then frames f0 .. f0+nf of every slot (nf = S:
    // the whole buffer in one piece) and the snapshot into mirror k, then sev[k]. Touches nothing
    // of this struct: it may run on a helper thread while the caller decodes and delivers.
    int enqueue(int k, int n_it, int f0, int nf) const {
        const hipStream_t st = dev->stream;
        for (int i = 0; i < n_it; ++i)
            if (int rc = launch_iteration(dev, st)) return rc;
        if (nf == S)
            HIPCHK(hipMemcpyAsync(codes(k), dev->codes_out, ncodes() * 4, hipMemcpyDeviceToHost, st));
        else
            HIPCHK(hipMemcpy2DAsync(codes(k) + (size_t)f0 * 8, (size_t)S * 32, dev->codes_out + (size_t)f0 * 8,
                                    (size_t)S * 32, (size_t)nf * 32, NB, hipMemcpyDeviceToHost, st));
        int32_t *h = snap(k);
        HIPCHK(hipMemcpyAsync(h, dev->ndone, 16, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(h + 4, dev->step, NB * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(h + 4 + NB, dev->done, NB * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(h + 4 + 2 * NB, dev->nframes, NB * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipEventRecord(dev->sev[k], st));
        return MP_OK;
    }

    // The round's chunks (jobs with n > 0, at most one per lane) through the codec; sets their `at`
    int decode(std::vector<Job> &jobs, const Snap &v) {
        // frame-major -> codebook-major (decode_frames_to_audio, 4468-4473)
        auto fill = [&](const Job &j, int32_t *dst, int stride) {
            const int32_t *fm = v.codes + ((size_t)j.b * S + j.f0) * 8;
            for (int t = 0; t < j.n; ++t)
                for (int c = 0; c < 8; ++c) dst[(size_t)c * stride + t] = fm[(size_t)t * 8 + c];
        };
        if (cont) {
            // one ragged call: every chunk laid out for the longest of the round
            int mx = 0;
            for (const Job &j : jobs) mx = std::max(mx, j.n);
            ids.clear();
            lens.clear();
            for (Job &j : jobs)
                if (j.n > 0) {
                    j.at = ids.size() * (size_t)mx * 1024;
                    ids.push_back(j.b);
                    lens.push_back(j.n);
                }
            if (ids.empty()) return MP_OK;
            cbm.assign(ids.size() * 8 * mx, 0);
            audio.resize(ids.size() * (size_t)mx * 1024);
            size_t q = 0;
            for (const Job &j : jobs)
                if (j.n > 0) fill(j, cbm.data() + q++ * 8 * mx, mx);
            if (int rc = mp_hip_codec_stream_decode_ragged(dev->cstream, ids.data(), (int)ids.size(), cbm.data(), lens.data(),
                                                           mx, audio.data()))
                return codec_fail(rc);
            return MP_OK;
        }
        // the reference's per-chunk semantics (chunks are independent, magpie.cpp:4739-4742):
        // full chunks in one launch sequence, a shorter one on its own
        size_t nfull = 0, nsamp = 0;
        for (Job &j : jobs)
            if (j.n == fpc) j.at = nfull++ * (size_t)fpc * 1024;
        nsamp = nfull * (size_t)fpc * 1024;
        for (Job &j : jobs)
            if (j.n > 0 && j.n != fpc) { j.at = nsamp; nsamp += (size_t)j.n * 1024; }
        audio.resize(nsamp);
        cbm.assign(std::max<size_t>(nfull, 1) * 8 * fpc, 0);
        size_t q = 0;
        for (const Job &j : jobs)
            if (j.n == fpc) fill(j, cbm.data() + q++ * 8 * fpc, fpc);
        if (nfull)
            if (int rc = mp_hip_codec_decode_chunks(codec, cbm.data(), (int)nfull, fpc, audio.data())) return codec_fail(rc);
        for (const Job &j : jobs)
            if (j.n > 0 && j.n != fpc) {
                fill(j, cbm.data(), j.n);
                if (int rc = mp_hip_codec_decode(codec, cbm.data(), j.n, audio.data() + j.at)) return codec_fail(rc);
            }
        return MP_OK;
    }

    // A decoded chunk to the callback. Declined (4820-4824) on a chunk that does not end its
    // utterance: the slot is stopped, its done flag set behind the round already queued.
    int deliver(const Job &j) {
        if (first) {
            dev->timing.first_audio_ms = ms_since(t0);
            first = false;
        }
        delivered[j.b] = j.f0 + j.n;
        if (on_audio && !on_audio(j.utt, audio.data() + j.at, j.n * 1024, user) && !j.ended) {
            stopped[j.b] = 1;
            static const int one = 1;
            HIPCHK(hipMemcpyAsync(dev->done + j.b, &one, 4, hipMemcpyHostToDevice, dev->stream));
            if (dev->guided)  // the pair stops together
                HIPCHK(hipMemcpyAsync(dev->done + dev->B + j.b, &one, 4, hipMemcpyHostToDevice, dev->stream));
            HIPCHK(hipStreamSynchronize(dev->stream));
        }
        return MP_OK;
    }
};
}  // namespace

// Streaming frame loop (magpie_synthesize_sentence_streaming's loop, magpie.cpp:4762-4838)
// for every utterance of the batch: a round is frames_per_chunk iterations (fewer at
// max_dec_steps), an utterance's last chunk may be shorter (EOS or max_dec_steps), and the
// chunks reach `on_audio` in slot order. An utterance that ends, by its EOS or because its
// callback declined a chunk, gets its end notice in the same round. Only the columns a round
// wrote go to the single codes mirror.
int mp_hip_decode_stream(mp_dev *dev, mp_codec *codec, int frames_per_chunk, mp_audio_cb on_audio, void *user,
                         int32_t *codes_out, int32_t *n_frames, int64_t *total_samples) {
    if (!dev) return MP_ERR_ARG;
    if (!dev->batch_ready) return fail(dev, MP_ERR_STATE, "mp_hip_begin_batch must precede mp_hip_decode_stream");
    if (!codec) return fail(dev, MP_ERR_ARG, "codec is required");
    const int fpc = frames_per_chunk > 0 ? frames_per_chunk : 4;  // default 4 (magpie.h:621)
    HIPCHK(hipSetDevice(dev->device));
    const int B = dev->B, S = dev->max_steps;
    if (int rc = prepare_iteration(dev)) return rc;
    StreamRun sr{dev, codec, fpc, on_audio, user};
    if (int rc = sr.open(B, 1)) return rc;
    std::vector<int> ended(B, 0);
    std::vector<Job> jobs;
    // The next round, to be queued by whoever calls the result. `it` counts the replays queued
    // and moves here, on the calling thread: a helper thread gets the round's numbers by value
    // and shares nothing with this loop but the decode stream and the mirror it fills.
    int it = 0;
    auto next_round = [&](int k) {
        const int f0 = it, n_it = std::min(fpc, S - it);
        it += n_it;
        return [&sr, k, n_it, f0]() -> int { return sr.enqueue(k, n_it, f0, n_it); };
    };
    if (int rc = next_round(0)()) return rc;
    for (int k = 0;; k ^= 1) {
        HIPCHK(hipEventSynchronize(dev->sev[k]));
        const Snap v = sr.view(k);
        if (int rc = handoff_bits(dev, v.nd[2])) return rc;  // before any frame of the round is delivered
        const double t_wait = ms_since(sr.t0);
        // this round's chunks: a live slot delivers whole chunks, an ended one what is left
        jobs.clear();
        bool more = false;
        for (int b = 0; b < B; ++b) {
            const bool done = v.done[b] != 0;
            more |= !(done || sr.stopped[b]);
            if (ended[b]) continue;
            const int n = (done ? v.nf[b] : v.step[b]) - sr.delivered[b];
            if (n < 0 || n > fpc) return fail(dev, MP_ERR_STATE, "stream: a slot offers more than one chunk in a round");
            if (done || n == fpc) jobs.push_back({b, b, sr.delivered[b], n, done, 0});
        }
        more &= it < S;
        // Queuing a round's graph replays can block the host (the queue's packet slots fill
        // up: 32 iterations of 65 launches), which left the codec waiting behind the next
        // round's decode, serialising the two (configs[2]: 27.2k vs 27.5k frames/s serial,
        // r06d): a round with codec work large enough to matter is queued from a helper
        // thread while this thread runs the codec (HIP calls are thread-safe)
        std::future<int> queued;
        const bool async_q = more && stream_async() && B * fpc >= STREAM_ASYNC_MIN_FRAMES;  // (a thread per round)
        if (more) {
            auto enqueue = next_round(k ^ 1);
            if (async_q) {
                queued = std::async(std::launch::async, [dev, enqueue]() -> int {
                    HIPCHK(hipSetDevice(dev->device));  // the current device is per thread
                    return enqueue();
                });
            } else if (int rc = enqueue()) {
                return rc;
            }
        }
        if (stream_trace()) fprintf(stderr, "[stream] round at %.3f ms: chunk landed, next queued %s at %.3f ms\n", t_wait,
                                    async_q ? "(async)" : "", ms_since(sr.t0));
        if (int rc = sr.decode(jobs, v)) return rc;
        if (stream_trace()) fprintf(stderr, "[stream]   codec of %zu chunks done at %.3f ms\n", jobs.size(), ms_since(sr.t0));
        if (queued.valid())
            if (int rc = queued.get()) return rc;
        for (const Job &j : jobs) {
            if (j.n > 0)
                if (int rc = sr.deliver(j)) return rc;
            if (j.ended || sr.stopped[j.b]) {  // end-of-utterance notice: (utt, NULL, 0)
                ended[j.b] = 1;
                if (on_audio) on_audio(j.b, nullptr, 0, user);
            }
        }
        if (!more) break;
    }
    HIPCHK(hipStreamSynchronize(dev->stream));
    dev->timing.decode_ms = ms_since(sr.t0);
    dev->timing.iterations = it;
    int total = 0;
    for (int b = 0; b < B; ++b) {
        if (n_frames) n_frames[b] = sr.delivered[b];
        total += sr.delivered[b];
    }
    dev->timing.frames_total = total;
    if (codes_out) HIPCHK(hipMemcpy(codes_out, dev->codes_out, (size_t)B * S * 8 * 4, hipMemcpyDeviceToHost));
    if (total_samples) *total_samples = (int64_t)total * 1024;
    return MP_OK;
}

// ---------------------------------------------------------------- streaming slot pool
// pool_run's loop with a round of fpc = r.poll replays between two looks at the slots, and the
// streaming mechanism above. Installs happen at round ends only, so a slot is a whole number
// of chunks in unless it finished inside the round. An utterance that ended, or whose callback
// declined a chunk in the round before, leaves its slot at the round end: the slot takes the
// staged utterance before the next round is queued, its codec lane starts over, and its
// chunks reach on_audio under the utterance's index (the event order is
// magpie_amd.dist.simulate_pool_stream). Each snapshot has a codes mirror of its own, copied
// whole ahead of the installs that zero a refilled slot's rows: a finished utterance's codes
// are on the host before its slot is reinstalled.
static int pool_stream_run(mp_dev *dev, PoolRun &r, mp_codec *codec, mp_audio_cb on_audio) {
    const int fpc = r.poll;
    std::vector<int> occ;  // utterance of each slot, -1 once it has ended
    if (int rc = pool_start(dev, r, occ)) return rc;
    const int B = (int)occ.size();
    if (B == 0) return MP_OK;
    const int S = dev->max_steps;
    StreamRun sr{dev, codec, fpc, on_audio, r.user};
    if (int rc = sr.open(B, 2)) return rc;
    HIPCHK(r.e0.create());
    HIPCHK(r.e1.create());
    HIPCHK(hipEventRecord(r.e0, dev->stream));
    std::vector<Job> jobs;
    int it = 0, live = B;
    // every utterance leaves its slot within max_steps iterations and two rounds
    const long long it_max = ((long long)r.N + 1) * ((long long)S + 2 * fpc);
    if (int rc = sr.enqueue(0, fpc, 0, S)) return rc;
    it += fpc;
    for (int k = 0;; k ^= 1) {
        if (it > it_max) return fail(dev, MP_ERR_STATE, "slot pool: a slot never finished");
        HIPCHK(hipEventSynchronize(dev->sev[k]));
        const Snap v = sr.view(k);
        if (int rc = handoff_bits(dev, v.nd[2])) return rc;  // before any frame is delivered
        jobs.clear();
        for (int b = 0; b < B; ++b) {
            if (occ[b] < 0) continue;
            const bool ended = v.done[b] != 0 || sr.stopped[b];
            // a stopped utterance's frames of the round that was already queued are not delivered
            const int n = sr.stopped[b] ? 0 : (v.done[b] ? v.nf[b] : v.step[b]) - sr.delivered[b];
            if (n < 0 || n > fpc) return fail(dev, MP_ERR_STATE, "slot pool: a slot is not a whole number of chunks in");
            if (n > 0 || ended) jobs.push_back({b, occ[b], sr.delivered[b], n, ended, 0});
        }
        // finished slots take the staged utterances, then the next round is queued
        for (const Job &j : jobs) {
            if (!j.ended) continue;
            occ[j.b] = -1;
            --live;
            if (!r.staged) continue;
            ++live;
            if (int rc = pool_refill(dev, r, occ, j.b)) return rc;
        }
        const bool more = live > 0;
        if (more) {
            if (int rc = sr.enqueue(k ^ 1, fpc, 0, S)) return rc;
            it += fpc;
        }
        if (int rc = sr.decode(jobs, v)) return rc;
        for (const Job &j : jobs)  // a finished slot's lane starts over
            if (sr.cont && j.ended)
                if (int rc = mp_hip_codec_stream_reset(dev->cstream, j.b)) return sr.codec_fail(rc);
        for (const Job &j : jobs) {
            if (j.n > 0)
                if (int rc = sr.deliver(j)) return rc;
            if (!j.ended) continue;
            on_audio(j.utt, nullptr, 0, r.user);  // end-of-utterance notice
            if (r.done) r.done(j.utt, v.codes + (size_t)j.b * S * 8, j.f0 + j.n, r.user);
            r.st.useful_slot_iters += j.f0 + j.n;
            sr.delivered[j.b] = sr.stopped[j.b] = 0;  // the slot's next utterance starts from nothing
        }
        if (!more) break;
    }
    if (int rc = end_timing(dev, r.e0, r.e1, it, (int)r.st.useful_slot_iters)) return rc;
    r.st.iterations = it;
    r.st.decode_ms = dev->timing.decode_ms;
    return MP_OK;
}

int mp_hip_decode_queue_stream(mp_dev *dev, mp_codec *codec, const int32_t *tokens, const int32_t *n_tokens,
                               const int32_t *speaker, int N, int tmax, int slots, int frames_per_chunk,
                               const mp_params *params, mp_next_cb next, mp_audio_cb on_audio, mp_done_cb done,
                               void *user, mp_queue_stats *stats) {
    if (!dev) return MP_ERR_ARG;
    if (stats) *stats = mp_queue_stats{};
    if (!dev->loaded) return fail(dev, MP_ERR_STATE, "no model loaded");
    if (!codec) return fail(dev, MP_ERR_ARG, "codec is required");
    if (!on_audio) return fail(dev, MP_ERR_ARG, "on_audio is required");
    const int fpc = frames_per_chunk > 0 ? frames_per_chunk : 4;  // default 4 (magpie.h:621)
    return pool_call(dev, tokens, n_tokens, speaker, N, tmax, slots, fpc, params, next, done, user, stats,
                     [&](PoolRun &r) { return pool_stream_run(dev, r, codec, on_audio); });
}

int mp_hip_lt_sample(mp_dev *dev, const float *hidden, float temperature, int top_k, int forbid_eos, uint64_t seed,
                     int32_t *sampled, int32_t *argmax) {
    if (!dev || !hidden || !sampled || !argmax) return MP_ERR_ARG;
    if (!dev->loaded) return fail(dev, MP_ERR_STATE, "no model loaded");
    if (temperature >= 0.01f && (top_k < 1 || top_k > mp::VCB)) return fail(dev, MP_ERR_ARG, "top_k must be in 1..2024");
    HIPCHK(hipSetDevice(dev->device));
    mp::LtIo &io = dev->lt_io;
    if (dev->ltio_mem.empty()) {
        bool ok = true;
        auto al = [&](auto **p, size_t n) {  // n 4-byte elements and the tail, zeroed
            ok = ok && dev->ltio_mem.bytes(p, n * 4 + 256) == hipSuccess &&
                 hipMemsetAsync(*p, 0, n * 4 + 256, dev->stream) == hipSuccess;
        };
        al(&io.hidden, 768); al(&io.lt_s, 9 * 256); al(&io.ltX, 256); al(&io.ltY, 256); al(&io.lty2, 256); al(&io.ltq, 256);
        al(&io.ltk, 8 * 256); al(&io.ltv, 8 * 256); al(&io.ltf, 1024);
        al(&io.ltp, std::max({mp::LT_FFN_P, mp::LTS_P, mp::LTQ_P}) * 256);
        al(&io.logits, 2024); al(&io.codes_cur, 8); al(&io.step, 1); al(&io.done, 1); al(&io.argeos, 1); al(&io.amax, 8);
        al(&io.cfg, (sizeof(mp::SmpCfg) + 3) / 4);
        if (!ok) {
            dev->ltio_mem.clear();
            return fail(dev, MP_ERR_HIP, "LT sample scratch allocation failed");
        }
        io.lt_only = 1;
        io.max_steps = 1;
    }
    io.sampling = temperature >= 0.01f;
    io.ignore_eos = forbid_eos != 0;
    // step: a call counter >= 4 (so only forbid_eos masks EOS), also the draw's step index
    const int step = 4 + dev->lt_calls++;
    mp::SmpCfg cfg{temperature, top_k, (unsigned long long)seed, -1, {-1}, 0.f, {}};
    for (int &pb : cfg.partner) pb = -1;
    HIPCHK(hipMemcpyAsync(io.hidden, hidden, 768 * 4, hipMemcpyHostToDevice, dev->stream));
    HIPCHK(hipMemcpyAsync(io.step, &step, 4, hipMemcpyHostToDevice, dev->stream));
    HIPCHK(hipMemcpyAsync(io.cfg, &cfg, sizeof cfg, hipMemcpyHostToDevice, dev->stream));
    HIPCHK(hipMemsetAsync(io.argeos, 0, 4, dev->stream));
    std::vector<mp::OpRec> ops;  // sampling / ignore_eos vary per call: a list per call
    if (int rc = build_lt(dev, io, 1, ops)) return rc;
    if (int rc = launch_ops(dev, ops, dev->stream)) return rc;
    HIPCHK(hipMemcpyAsync(sampled, io.codes_cur, 32, hipMemcpyDeviceToHost, dev->stream));
    HIPCHK(hipMemcpyAsync(argmax, io.amax, 32, hipMemcpyDeviceToHost, dev->stream));
    HIPCHK(hipStreamSynchronize(dev->stream));
    return MP_OK;
}

int mp_hip_get_trace(mp_dev *dev, float *hidden) {
    if (!dev || !hidden) return MP_ERR_ARG;
    if (!dev->trace) return fail(dev, MP_ERR_STATE, "trace_hidden was not enabled");
    HIPCHK(hipMemcpy(hidden, dev->trace, (size_t)dev->B * (dev->max_steps + 1) * 768 * 4, hipMemcpyDeviceToHost));
    return MP_OK;
}

int mp_hip_get_trace_uncond(mp_dev *dev, float *hidden) {
    if (!dev || !hidden) return MP_ERR_ARG;
    if (!dev->trace) return fail(dev, MP_ERR_STATE, "trace_hidden was not enabled");
    if (!dev->guided) return fail(dev, MP_ERR_STATE, "the batch was not begun under guidance (mp_hip_set_cfg)");
    const size_t n = (size_t)dev->B * (dev->max_steps + 1) * 768;  // slots B .. 2B-1 follow the conditional ones
    HIPCHK(hipMemcpy(hidden, dev->trace + n, n * 4, hipMemcpyDeviceToHost));
    return MP_OK;
}

int64_t mp_hip_debug_buffer(mp_dev *dev, const char *name, void *host, int64_t bytes) {
    if (!dev || !name || bytes < 0) return MP_ERR_ARG;
    if (!dev->batch_ready) return fail(dev, MP_ERR_STATE, "no batch");
    const size_t NB = dev->NB, L = dev->m.dec_layers, T = dev->Tmax, S = dev->max_seq;
    const std::string n(name);
    const void *src = nullptr;
    size_t sz = 0;
    if (n == "enc_out") { src = dev->enc_out; sz = NB * T * 768 * 4; }
    else if (n == "xak") { src = dev->xak; sz = NB * L * T * 128 * 4; }
    else if (n == "xav") { src = dev->xav; sz = NB * L * T * 128 * 4; }
    else if (n == "kc") { src = dev->kc; sz = NB * L * S * 768 * (dev->kv16 ? 2 : 4); }
    else if (n == "vc") { src = dev->vc; sz = NB * L * S * 768 * (dev->kv16 ? 2 : 4); }
    else if (n == "x") { src = dev->x; sz = NB * 768 * 4; }
    else if (n == "q8dump" && dev->q8dump) { src = dev->q8dump; sz = dev->q8dump_slot * dev->q8dump_n; }
    else if (n == "q8dump_index" && dev->q8dump) {
        sz = dev->q8dump_index.size() * 4;
        if (host) memcpy(host, dev->q8dump_index.data(), std::min<size_t>(sz, (size_t)bytes));
        return (int64_t)sz;
    }
    else return fail(dev, MP_ERR_ARG, "unknown buffer " + n);
    if (host) {
        HIPCHK(hipSetDevice(dev->device));
        HIPCHK(hipStreamSynchronize(dev->stream));
        HIPCHK(hipMemcpy(host, src, std::min<size_t>(sz, (size_t)bytes), hipMemcpyDeviceToHost));
    }
    return (int64_t)sz;
}

int mp_hip_get_timing(mp_dev *dev, mp_timing *t) {
    if (!dev || !t) return MP_ERR_ARG;
    *t = dev->timing;
    return MP_OK;
}

int mp_hip_num_ops(mp_dev *dev) { return dev ? (int)dev->ops.size() : 0; }

const char *mp_hip_op_name(mp_dev *dev, int op) {
    if (!dev || op < 0 || op >= (int)dev->ops.size()) return "";
    return dev->ops[op].name.c_str();
}

double mp_hip_op_bytes(mp_dev *dev, int op) {
    if (!dev || op < 0 || op >= (int)dev->ops.size()) return -1.0;
    const mp::OpRec &r = dev->ops[op];
    if (r.kind == mp::K_ATTN || r.add_sa) {
        // live cache length of slot 0 after the run: keys 0..pos
        int pos = 0;
        hipMemcpy(&pos, dev->pos, 4, hipMemcpyDeviceToHost);
        // K, V rows (+ q in, unless handed over in-launch) + the split states out
        const double kvb = dev->kv16 ? 2.0 : 4.0;
        return (r.add_sa ? r.bytes : 4.0 * dev->NB * 768) +
               dev->NB * ((double)(pos + 1) * 768 * 2 * kvb + 4.0 * mp::NH * mp::SA_SPLITS * mp::SA_PART);
    }
    return r.bytes;
}

int mp_hip_profile_ops(mp_dev *dev, int iters, float *avg_us) { return mp_hip_profile_ops_ex(dev, iters, avg_us, nullptr); }

int mp_hip_profile_ops_ex(mp_dev *dev, int iters, float *avg_us, float *pair_us) {
    if (!dev || !avg_us || iters < 1) return MP_ERR_ARG;
    if (!dev->batch_ready || dev->ops.empty())
        return fail(dev, MP_ERR_STATE, "mp_hip_profile_ops needs a decoded batch (mp_hip_decode first)");
    HIPCHK(hipSetDevice(dev->device));
    const int n = (int)dev->ops.size();
    std::vector<mp::Event> ev(3 * (size_t)n);  // [before, after, after + an empty pair's second event]
    for (auto &e : ev) HIPCHK(e.create());
    std::vector<double> sum(n, 0.0), psum(n, 0.0);
    int rc = MP_OK;
    for (int it = 0; it < iters && rc == MP_OK; ++it) {
        for (int i = 0; i < n; ++i) {
            const mp::OpRec &r = dev->ops[i];
            HIPCHK(hipEventRecord(ev[3 * i], dev->stream));
            const hipError_t e = launch_rec(r, dev->stream);
            HIPCHK(e);
            HIPCHK(hipEventRecord(ev[3 * i + 1], dev->stream));
            if (pair_us) HIPCHK(hipEventRecord(ev[3 * i + 2], dev->stream));
        }
        HIPCHK(hipStreamSynchronize(dev->stream));
        for (int i = 0; i < n; ++i) {
            float ms = 0.f;
            HIPCHK(hipEventElapsedTime(&ms, ev[3 * i], ev[3 * i + 1]));
            sum[i] += ms;
            if (pair_us) {
                HIPCHK(hipEventElapsedTime(&ms, ev[3 * i + 1], ev[3 * i + 2]));
                psum[i] += ms;
            }
        }
    }
    for (int i = 0; i < n; ++i) avg_us[i] = (float)(sum[i] * 1000.0 / iters);
    if (pair_us)
        for (int i = 0; i < n; ++i) pair_us[i] = (float)(psum[i] * 1000.0 / iters);
    return rc;
}

int mp_hip_profile_ops_ts(mp_dev *dev, int iters, float *avg_us) {
    if (!dev || !avg_us || iters < 1) return MP_ERR_ARG;
    if (!dev->batch_ready || dev->ops.empty())
        return fail(dev, MP_ERR_STATE, "mp_hip_profile_ops_ts needs a decoded batch (mp_hip_decode first)");
    HIPCHK(hipSetDevice(dev->device));
    const int n = (int)dev->ops.size();
    const size_t per = (size_t)2 * TS_BLOCKS * TS_WAVES;  // u64 per op
    mp::DevBlocks ts_mem;
    unsigned long long *ts = nullptr;
    HIPCHK(ts_mem.bytes(&ts, (size_t)n * per * 8));
    std::vector<unsigned long long> h((size_t)n * per);
    std::vector<double> sum(n, 0.0);
    std::vector<int> cnt(n, 0);
    int rc = MP_OK;
    for (int it = 0; it < iters && rc == MP_OK; ++it) {
        HIPCHK(hipMemsetAsync(ts, 0, (size_t)n * per * 8, dev->stream));
        for (int i = 0; i < n; ++i) {
            mp::OpRec r = dev->ops[i];
            unsigned long long *t = ts + (size_t)i * per;
            r.g.ts = t; r.a.ts = t; r.x.ts = t; r.f.ts = t; r.lf.ts = t; r.l2.f.ts = t; r.lf3.l.f.ts = t; r.lq8.ts = t;
            const hipError_t e = launch_rec(r, dev->stream);
            if (e != hipSuccess) { rc = fail(dev, MP_ERR_HIP, std::string("profile launch: ") + hipGetErrorString(e)); break; }
        }
        if (rc != MP_OK) break;
        HIPCHK(hipMemcpyAsync(h.data(), ts, (size_t)n * per * 8, hipMemcpyDeviceToHost, dev->stream));
        HIPCHK(hipStreamSynchronize(dev->stream));
        if (const char *dump = getenv("MAGPIE_TS_DUMP")) {  // raw stamps of the last iteration (diagnostics)
            if (FILE *fp = fopen(dump, "wb")) { fwrite(h.data(), 8, h.size(), fp); fclose(fp); }
        }
        for (int i = 0; i < n; ++i) {
            unsigned long long t0 = ~0ull, t1 = 0;
            for (size_t k = 0; k < per / 2; ++k) {
                const unsigned long long a = h[(size_t)i * per + 2 * k], b = h[(size_t)i * per + 2 * k + 1];
                if (b == 0) continue;  // slot not written
                t0 = std::min(t0, a);
                t1 = std::max(t1, b);
            }
            if (t1 > t0 && t0 != ~0ull) { sum[i] += (double)(t1 - t0); ++cnt[i]; }
        }
    }
    // s_memrealtime counts at 100 MHz: 10 ns per tick; -1 for ops without timestamps
    for (int i = 0; i < n; ++i) avg_us[i] = cnt[i] ? (float)(sum[i] / cnt[i] * 0.01) : -1.f;
    return rc;
}

// Empty dispatches bracketing mp_hip_profile_ops_kev's launches, so that a
// rocprofv3 kernel trace of the same command can be cut to exactly those launches
// (tools_dev/prof_phase.py) and compared with the events' figures.
__global__ void profile_mark_kernel() {}

int mp_hip_profile_ops_kev(mp_dev *dev, int iters, float *avg_us) {
    if (!dev || !avg_us || iters < 1) return MP_ERR_ARG;
    if (!dev->batch_ready || dev->ops.empty())
        return fail(dev, MP_ERR_STATE, "mp_hip_profile_ops_kev needs a decoded batch (mp_hip_decode first)");
    HIPCHK(hipSetDevice(dev->device));
    const int n = (int)dev->ops.size();
    std::vector<mp::Event> ev(2 * (size_t)n);
    for (auto &e : ev) HIPCHK(e.create());
    std::vector<double> sum(n, 0.0);
    int rc = MP_OK;
    hipLaunchKernelGGL(profile_mark_kernel, dim3(1), dim3(64), 0, dev->stream);
    for (int it = 0; it < iters && rc == MP_OK; ++it) {
        for (int i = 0; i < n && rc == MP_OK; ++i) {
            mp::g_kev[0] = ev[2 * i];
            mp::g_kev[1] = ev[2 * i + 1];
            const hipError_t e = launch_rec(dev->ops[i], dev->stream);
            mp::g_kev[0] = mp::g_kev[1] = nullptr;
            if (e != hipSuccess) rc = fail(dev, MP_ERR_HIP, std::string("profile launch: ") + hipGetErrorString(e));
        }
        if (rc != MP_OK) break;
        HIPCHK(hipStreamSynchronize(dev->stream));
        for (int i = 0; i < n; ++i) {
            float ms = 0.f;
            HIPCHK(hipEventElapsedTime(&ms, ev[2 * i], ev[2 * i + 1]));
            sum[i] += ms;
        }
    }
    hipLaunchKernelGGL(profile_mark_kernel, dim3(1), dim3(64), 0, dev->stream);
    HIPCHK(hipStreamSynchronize(dev->stream));
    for (int i = 0; i < n; ++i) avg_us[i] = (float)(sum[i] * 1000.0 / iters);
    return rc;
}

int mp_hip_time_op(mp_dev *dev, int op, int reps, float *avg_us) {
    if (!dev || !avg_us || reps < 1 || op < 0 || op >= (int)dev->ops.size()) return MP_ERR_ARG;
    HIPCHK(hipSetDevice(dev->device));
    mp::OpRec r = dev->ops[op];
    r.g.ndone = nullptr;
    r.g.trace = nullptr;
    // XA rewrites this layer's split states only; XA-Q8 rewrites x2 with the same values
    auto launch = [&]() -> hipError_t { return launch_rec(r, dev->stream); };
    if (r.kind == mp::K_FIN) return fail(dev, MP_ERR_ARG, "op cannot be timed standalone");
    // an op carrying an in-launch hand-off (QKV -> SA, O-projection -> XA) tags it with the
    // iteration counter: relaunched with the same tag, its consumers would find the previous
    // launch's granules and not wait for their producers (a different, shorter critical path)
    const bool handoff = (r.kind == mp::K_GEMV && r.g.iter) || (r.kind == mp::K_LTSLOT && r.l2.gh) ||
                         r.kind == mp::K_LTFRONT || r.kind == mp::K_LTSLOTQ8 ||
                         (r.kind == mp::K_ATTN && r.a.gh);
    if (handoff)
        return fail(dev, MP_ERR_ARG, "op carries an in-launch hand-off: back-to-back timing would not wait for it");
    HIPCHK(launch());  // warm
    mp::Event e0, e1;
    HIPCHK(e0.create());
    HIPCHK(e1.create());
    HIPCHK(hipEventRecord(e0, dev->stream));
    for (int i = 0; i < reps; ++i) HIPCHK(launch());
    HIPCHK(hipEventRecord(e1, dev->stream));
    HIPCHK(hipEventSynchronize(e1));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    *avg_us = ms * 1000.f / reps;
    return MP_OK;
}

}  // extern "C"
