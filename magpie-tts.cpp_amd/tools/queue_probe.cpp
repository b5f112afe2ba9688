// queue_probe — the drop-in C++ API's continuous batching (magpie_synthesize_codes_queue,
// include/magpie.h) against magpie_synthesize_codes utterance by utterance, for
// tests/test_pool_gpu.py: prints one JSON line, exit 0 when every utterance's codes match.
// The utterances are synthetic token rows (BOS, ids below 96, EOS) of the given lengths.
// usage: magpie-queue-probe MODEL.gguf SLOTS MAX_DEC_STEPS LEN [LEN ...]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/magpie.h"

int main(int argc, char **argv) {
    if (argc < 5) {
        fprintf(stderr, "usage: %s MODEL.gguf SLOTS MAX_DEC_STEPS LEN [LEN ...]\n", argv[0]);
        return 2;
    }
    magpie_context *ctx = magpie_init(argv[1]);
    if (!ctx) return 1;
    const int slots = atoi(argv[2]);
    ctx->model.hparams.max_dec_steps = atoi(argv[3]);
    ctx->temperature = 0.0f;  // greedy: a single run and a queue entry draw nothing
    ctx->speaker_id = 1;
    const int N = argc - 4;
    std::vector<std::vector<int32_t>> toks(N);
    unsigned long long lcg = 0x9E3779B97F4A7C15ull;
    for (int i = 0; i < N; ++i) {
        const int len = atoi(argv[4 + i]);
        if (len < 1) return 2;
        for (int t = 0; t < len; ++t) {
            lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
            toks[i].push_back(t == 0 && len > 1 ? 2378 : t == len - 1 && len > 1 ? 2379 : (int32_t)((lcg >> 33) % 96));
        }
    }
    std::vector<const int32_t *> tp(N);
    std::vector<int> nt(N);
    for (int i = 0; i < N; ++i) { tp[i] = toks[i].data(); nt[i] = (int)toks[i].size(); }
    std::vector<std::vector<int32_t>> got(N);
    const bool ok = magpie_synthesize_codes_queue(ctx, tp.data(), nt.data(), N, slots, got.data());
    bool equal = ok;
    printf("{\"ok\": %s, \"frames\": [", ok ? "true" : "false");
    for (int i = 0; i < N; ++i) {
        const std::vector<int32_t> ref = magpie_synthesize_codes(ctx, tp[i], nt[i]);
        equal = equal && ref == got[i];
        printf("%s%d", i ? ", " : "", (int)got[i].size() / 8);
    }
    printf("], \"equal\": %s}\n", equal ? "true" : "false");
    magpie_free(ctx);
    return equal ? 0 : 1;
}
