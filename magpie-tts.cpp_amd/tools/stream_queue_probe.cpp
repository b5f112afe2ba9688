// stream_queue_probe — the drop-in C++ API's streaming slot pool
// (magpie_synthesize_streaming_queue, include/magpie.h), for tests/test_pool_stream_gpu.py:
// every utterance's codes against magpie_synthesize_codes, and its audio against
// magpie_codec_decode of those codes: the concatenated chunks against one decode of all the
// frames, bit for bit, in continuous mode, else every chunk against the decode of that chunk's
// frames alone. Prints one JSON line, exit 0 when everything matches.
// The utterances are synthetic token rows (BOS, ids below 96, EOS) of the given lengths.
// usage: magpie-stream-queue-probe MODEL.gguf CODEC.gguf SLOTS MAX_DEC_STEPS CONTINUOUS(0|1) LEN [LEN ...]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/magpie.h"

namespace {
struct Heard {
    std::vector<std::vector<std::vector<float>>> chunks;  // [utterance][chunk]
    std::vector<int> ends;
    bool in_order = true;  // no chunk after an utterance's end notice
};
bool on_audio(int utt, const float *x, int n, void *user) {
    Heard &h = *(Heard *)user;
    if (!x) {
        ++h.ends[utt];
        return true;
    }
    if (h.ends[utt]) h.in_order = false;
    h.chunks[utt].emplace_back(x, x + n);
    return true;
}
// frames [f0, f0 + n) of frame-major codes, codebook-major
std::vector<int32_t> cb_major(const std::vector<int32_t> &codes, int f0, int n) {
    std::vector<int32_t> out((size_t)8 * n);
    for (int t = 0; t < n; ++t)
        for (int c = 0; c < 8; ++c) out[(size_t)c * n + t] = codes[(size_t)(f0 + t) * 8 + c];
    return out;
}
}  // namespace

int main(int argc, char **argv) {
    if (argc < 7) {
        fprintf(stderr, "usage: %s MODEL.gguf CODEC.gguf SLOTS MAX_DEC_STEPS CONTINUOUS(0|1) LEN [LEN ...]\n", argv[0]);
        return 2;
    }
    magpie_context *ctx = magpie_init(argv[1]);
    if (!ctx) return 1;
    magpie_codec *codec = magpie_codec_init(argv[2]);
    if (!codec) return 1;
    const int slots = atoi(argv[3]);
    ctx->model.hparams.max_dec_steps = atoi(argv[4]);
    ctx->continuous_codec = atoi(argv[5]) != 0;
    magpie_stream_params prm;
    prm.temperature = 0.0f;  // greedy: a single run and a queue entry draw nothing
    prm.speaker_id = 1;
    const int fpc = prm.frames_per_chunk;
    const int N = argc - 6;
    std::vector<std::vector<int32_t>> toks(N);
    unsigned long long lcg = 0x9E3779B97F4A7C15ull;
    for (int i = 0; i < N; ++i) {
        const int len = atoi(argv[6 + i]);
        if (len < 1) return 2;
        for (int t = 0; t < len; ++t) {
            lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
            toks[i].push_back(t == 0 && len > 1 ? 2378 : t == len - 1 && len > 1 ? 2379 : (int32_t)((lcg >> 33) % 96));
        }
    }
    std::vector<const int32_t *> tp(N);
    std::vector<int> nt(N);
    for (int i = 0; i < N; ++i) { tp[i] = toks[i].data(); nt[i] = (int)toks[i].size(); }
    Heard heard;
    heard.chunks.resize(N);
    heard.ends.assign(N, 0);
    prm.user_data = &heard;
    std::vector<std::vector<int32_t>> got(N);
    const int total = magpie_synthesize_streaming_queue(ctx, codec, tp.data(), nt.data(), N, slots, prm, on_audio, got.data());
    const bool ok = total >= 0;
    bool equal = ok && heard.in_order, audio_equal = ok;
    long long samples = 0;
    printf("{\"ok\": %s, \"continuous\": %s, \"frames\": [", ok ? "true" : "false", ctx->continuous_codec ? "true" : "false");
    for (int i = 0; i < N; ++i) {
        const std::vector<int32_t> ref = magpie_synthesize_codes(ctx, tp[i], nt[i]);
        equal = equal && ref == got[i] && heard.ends[i] == 1;
        const int nf = (int)got[i].size() / 8;
        printf("%s%d", i ? ", " : "", nf);
        // the chunks are frames_per_chunk frames each, the last one the remainder
        std::vector<float> all;
        int f0 = 0;
        for (const std::vector<float> &ch : heard.chunks[i]) {
            const int n = (int)ch.size() / 1024;
            if (n != (nf - f0 < fpc ? nf - f0 : fpc) || n < 1) { audio_equal = false; break; }
            if (!ctx->continuous_codec) {
                const std::vector<int32_t> cm = cb_major(got[i], f0, n);
                audio_equal = audio_equal && magpie_codec_decode(codec, cm.data(), n) == ch;
            }
            all.insert(all.end(), ch.begin(), ch.end());
            f0 += n;
        }
        audio_equal = audio_equal && f0 == nf;
        samples += (long long)all.size();
        if (ctx->continuous_codec && audio_equal && nf > 0) {
            const std::vector<int32_t> cm = cb_major(got[i], 0, nf);
            audio_equal = magpie_codec_decode(codec, cm.data(), nf) == all;
        }
    }
    audio_equal = audio_equal && samples == total;
    equal = equal && audio_equal;
    printf("], \"samples\": %lld, \"audio_equal\": %s, \"equal\": %s}\n", samples, audio_equal ? "true" : "false",
           equal ? "true" : "false");
    magpie_codec_free(codec);
    magpie_free(ctx);
    return equal ? 0 : 1;
}
