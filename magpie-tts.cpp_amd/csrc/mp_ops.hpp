// The decode launchers' catalogue: what the three kernel families (mp_decode.hip f32,
// mp_decode_b16.hip bf16 / F16, mp_decode_q8.hip Q8_0 / Q4_0) offer the runtime's list
// builders (mp_runtime.hip build_iteration / build_lt). Included by all four, so a
// declaration and its definition cannot drift apart.
#pragma once
#include <hip/hip_runtime.h>

#include "mp_params.hpp"

namespace mp {

using GemvFn = hipError_t (*)(const GemvP &, hipStream_t);

// One family's fused GEMV ops at one batch size. Each entry points at the instantiation of
// the family's launch_*<> template itself; null = the family has no kernel for that op at
// that batch size (Emit::gemv answers MP_ERR_UNSUPPORTED).
struct OpTable {
    // decoder layer
    GemvFn qkv;          // LN + QKV + KV append, the SA a launch of its own
    GemvFn qkv_sa;       // the same + the SA in the launch (EPI_QKV_SA)
    GemvFn oproj;        // SA split states merged + O-projection + residual
    GemvFn oproj_xa;     // the same + the fused XA in the launch (EPI_RESID_XA)
    GemvFn oproj_xa_pm;  // oproj_xa on an SA output its split workgroups merged (plain rows; bf16, 8 and 16 slots)
    GemvFn oproj_xq;     // Q8_0: O-projection + the whole direct Q8_0 XA in the launch (EPI_RESID_XQ8)
    GemvFn xq;           // the direct XA's q_net
    GemvFn ff1;          // LN + FFN up + GELU from a materialised x2 (direct XA, merged XA tail)
    GemvFn ff1x;         // the same, the fused XA's split states merged into x2 first
    GemvFn ff2;          // FFN down + residual
    // local transformer
    GemvFn lt_in0;       // final LN + in_proj
    GemvFn lt_inh;       // in_proj of a caller's normalised hidden (the standalone LT sample; batch 1)
    GemvFn lt_a;         // position 0: LN + q|k|v
    GemvFn lt_b;         // position 0: attention + o_net + residual
    GemvFn lt_bg;        // position cb >= 1: pick + gathers + attention + o_net + residual (below 8 slots)
    GemvFn lt_bo;        // o_net + residual after lt_pick_kernel (from 8 slots)
    GemvFn lt_c, lt_d;   // FFN up + GELU, FFN down + residual (F16 mode)
    GemvFn lt_e;         // a codebook's head on y2
    GemvFn lt_em;        // the head with the family's own LT step's partial sums merged first (batch 1)
    GemvFn lt_emf;       // the head with lt_ffn_kernel's partial sums merged first (batch 1)
};

inline int op_nb_index(int NB) { return NB == 1 ? 0 : NB == 2 ? 1 : NB == 4 ? 2 : NB == 8 ? 3 : 4; }

// The families' tables, NB in {1, 2, 4, 8, 16}; each defined beside its launch_*<> template.
const OpTable &f32_ops(int NB);            // mp_decode.hip (16 slots: only what another mode's list takes from it)
const OpTable &b16_ops(int NB, bool f16);  // mp_decode_b16.hip
const OpTable &q8_ops(int NB);             // mp_decode_q8.hip

// The launchers outside the tables (their own parameter structs or a run-time batch size)
hipError_t op_sa_attn(const AttnP &, int, hipStream_t);
hipError_t op_xa(const XaP &, int, hipStream_t);
hipError_t op_xa_q8(const XaQ8P &, int, hipStream_t);
hipError_t op_finalize(const FinP &, int, hipStream_t);
hipError_t op_embed(const EmbP &, int, hipStream_t);
hipError_t op_slot_install(const InstallP &, hipStream_t);  // between two replays, never in the iteration's list
hipError_t op_lt_kvo(const GemvP &, int, hipStream_t);
hipError_t op_lt_pick(const GemvP &, int, hipStream_t);
hipError_t op_lt_ffn(const LtFfnP &, int, hipStream_t);
hipError_t op_lt_merge(const LtFfnP &, int, hipStream_t);
hipError_t op_lt_ffn2(const LtFfn2P &, int, hipStream_t);
hipError_t op_lt_front(const LtFrontP &, hipStream_t);
hipError_t op_lt_slot(const LtFfn2P &, int, hipStream_t);
hipError_t op_lt_slot_q8(const LtSlotQ8P &, int, hipStream_t);
// load-time repacking into MFMA fragment order
hipError_t pack_b16(const float *, int, int, unsigned short *, hipStream_t, bool f16);
hipError_t pack_q8(const signed char *, const unsigned short *, int, int, unsigned char *, unsigned short *, hipStream_t);
hipError_t pack_q4(const signed char *, int, int, unsigned char *, hipStream_t);
int b16_oproj_ks();  // the 16-bit O-projection's split-K slices (MP_OPROJ_KS)

}  // namespace mp
