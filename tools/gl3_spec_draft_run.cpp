// gl3_spec_draft_run — speculative decoding of ONE sequence with a DRAFT MODEL over the C-ABI of libgpullama_hip.so (no Python, no torch): two
// plans on one device, a small model drafting for a large one.  Every step the draft plan makes up to K single-token steps, then ONE
// gl3_forward_batch_verify_dist call on the target forwards the last real token and the drafts in one pass over the target's weights and
// decides on the device how many drafts stand (8 bytes come back).  At a temperature each draft is verified against the distribution it
// was drawn from — accept with probability min(1, p / q), on rejection resample from the normalised max(p - q, 0) — so the emitted ids are
// distributed as the target model's own samples, whatever the draft model.
//
//   gl3_spec_draft_run -m target.gguf -md draft.gguf --ids 1,2,3 -n NEW [--draft K] [-b BATCH] [--temperature T] [--draft-temperature Td]
//                      [--seed S] [--chain]
//
// Positions: prompt id k at position k, generated ids behind them (tools/gl3_spec_run's protocol).  Both plans are prefilled with all but the
// last prompt id.  A step that starts with the last real token at position p:
//   drafting   k = min(K (default 4), ids still wanted - 1, context left, BATCH (default 16) - 1) single-token steps of the draft plan, the
//              first on the last real token at p, each next on the id the previous one gave.  T > 0 and Td > 0 (default Td = T):
//              gl3_forward_decode_sample(topp 0, one coin) and gl3_draft_probs_put(target, j, draft) for draft j, q_slots[j] = j.
//              T == 0 or Td == 0: gl3_forward_decode's argmax, a fixed token, q_slots = -1 (the one-hot rule; T == 0: greedy verification,
//              the ids of plain greedy decoding of the target).
//              --chain: the k steps and their puts are ONE gl3_forward_decode_chain on the draft plan (target and slot 0 when sampled, no
//              target when greedy): one host wait per speculation step instead of one per draft.  The same coins in the same order, so the
//              ids and the counts line are those of a run without it.
//   verifying  the run [last real token, drafts] of m = k + 1 rows -> {a, token}: the first a drafts and `token` are appended, the target
//              continues at p + a + 1 and overwrites the K / V rows of the rejected drafts before anything reads them.
//   draft KV   the draft plan has consumed the ids at p .. p + k - 1.  Rejected positions are overwritten by its next steps, as the
//              target's; when every draft stood (a == k) the id at p + k has not been through the draft plan: it is fed with one
//              gl3_forward_decode whose output is ignored.
//   coins      one L32X64MixRandom seeded --seed (default 1234): per step first one nextFloat per sampled draft, in draft order, then (T > 0)
//              coins[i][0], coins[i][1] for every row i of the run in row order — all 2 m are drawn wherever the rejection falls.
// stdout: "generated: id id ...".  stderr: the line "steps=… drafted=… accepted=… tokens=…", then a line "timing: …" with the loop's host-clock
// times (prefill_ms, decode_ms, tok_s, draft_ms = the part of decode_ms spent in the draft plan, step_us=rows:mean microseconds of a verify
// step by run length).
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../include/gpullama3_hip.h"

// jdk.random.L32X64MixRandom (the JDK's default RandomGenerator), as tools/gl3_run.cpp has it: 32-bit LCG s = M s + a, xoroshiro64 (x0, x1),
// mixer lea32(s + x0).
struct L32X64MixRandom {
    uint32_t a, s, x0, x1;
    static uint32_t murmur32(uint32_t z) { z = (z ^ (z >> 16)) * 0x85EBCA6Bu; z = (z ^ (z >> 13)) * 0xC2B2AE35u; return z ^ (z >> 16); }
    static uint32_t lea32(uint32_t z) { z = (z ^ (z >> 16)) * 0xD36D884Bu; z = (z ^ (z >> 16)) * 0xD36D884Bu; return z ^ (z >> 16); }
    static uint32_t rotl(uint32_t x, int k) { return (x << k) | (x >> (32 - k)); }
    explicit L32X64MixRandom(uint64_t seed) {
        seed ^= 0x6A09E667F3BCC909ULL;
        a = murmur32((uint32_t)(seed >> 32)) | 1u;
        s = 1;
        x0 = lea32((uint32_t)seed);
        x1 = lea32((uint32_t)seed + 0x9E3779B9u);
        if ((x0 | x1) == 0) { const uint32_t v = s + 0x9E3779B9u; x0 = murmur32(v); x1 = murmur32(v + 0x9E3779B9u); }
    }
    uint32_t nextInt() {
        const uint32_t r = lea32(s + x0);
        s = 0xADB4A92Du * s + a;
        uint32_t q0 = x0, q1 = x1;
        q1 ^= q0; q0 = rotl(q0, 26); q0 = q0 ^ q1 ^ (q1 << 9); q1 = rotl(q1, 13);
        x0 = q0; x1 = q1;
        return r;
    }
    float nextFloat() { return (float)(nextInt() >> 8) * (1.0f / (float)(1 << 24)); }      // RandomSupport.boundedNextFloat(rng, 1f)
};

static double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
static std::vector<int32_t> parse_ids(const char* s) {
    std::vector<int32_t> v;
    for (const char* p = s; *p;) {
        char* e;
        const long x = strtol(p, &e, 10);
        if (e == p) break;
        v.push_back((int32_t)x);
        p = *e == ',' ? e + 1 : e;
    }
    return v;
}

#define CK(ctx, call)                                                                                   \
    do {                                                                                                \
        const int32_t r_ = (call);                                                                      \
        if (r_ != GL3_OK) { fprintf(stderr, "%s failed (%d): %s\n", #call, r_, ctx ? gl3_last_error(ctx) : gl3_gguf_last_error(nullptr)); return 1; } \
    } while (0)

int main(int argc, char** argv) {
    std::string path, draft_path;
    std::vector<int32_t> prompt;
    int n_new = 0, K = 4, batch = 16;
    float T = 0.f, Td = -1.f;
    uint64_t seed = 1234;
    bool chain = false;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto val = [&]() { return i + 1 < argc ? argv[++i] : (char*)""; };
        if (a == "-m") path = val();
        else if (a == "-md") draft_path = val();
        else if (a == "--ids") prompt = parse_ids(val());
        else if (a == "-n") n_new = atoi(val());
        else if (a == "--draft") K = atoi(val());
        else if (a == "-b") batch = atoi(val());
        else if (a == "--temperature") T = (float)atof(val());
        else if (a == "--draft-temperature") Td = (float)atof(val());
        else if (a == "--seed") seed = strtoull(val(), nullptr, 10);
        else if (a == "--chain") chain = true;
        else { fprintf(stderr, "gl3_spec_draft_run: unknown argument %s (see the header of tools/gl3_spec_draft_run.cpp)\n", a.c_str()); return 2; }
    }
    if (path.empty() || draft_path.empty() || prompt.empty() || n_new <= 0) {
        fprintf(stderr, "gl3_spec_draft_run: -m target.gguf, -md draft.gguf, --ids a,b,c and -n NEW (> 0) are required\n");
        return 2;
    }
    if (Td < 0.f) Td = T;
    if (K < 0 || batch < 2 || !(T >= 0.f) || !(Td >= 0.f)) { fprintf(stderr, "gl3_spec_draft_run: --draft >= 0, -b >= 2, temperatures >= 0\n"); return 2; }
    if (chain && K > GL3_CHAIN_MAX) { fprintf(stderr, "gl3_spec_draft_run: --chain takes --draft <= %d\n", GL3_CHAIN_MAX); return 2; }
    const bool sampled_draft = T > 0.f && Td > 0.f;

    const int N = (int)prompt.size();
    int ctx_len = N + n_new;      // kept if both files' context lengths admit it, else clamped: the plans' context bounds the loop
    int vocab[2] = {0, 0};
    for (int w = 0; w < 2; ++w) {
        const std::string& f = w ? draft_path : path;
        gl3_gguf* g = nullptr;
        gl3_model_desc d{};
        d.ctx = ctx_len;
        if (gl3_gguf_open(f.c_str(), &g) != GL3_OK || gl3_gguf_model_desc(g, &d, nullptr) != GL3_OK) { fprintf(stderr, "cannot read %s: %s\n", f.c_str(), gl3_gguf_last_error(g)); return 1; }
        gl3_gguf_close(g);
        ctx_len = d.ctx;
        vocab[w] = d.vocab;
    }
    if (vocab[0] != vocab[1]) { fprintf(stderr, "gl3_spec_draft_run: the draft model's vocabulary (%d) is not the target's (%d)\n", vocab[1], vocab[0]); return 2; }
    for (int32_t t : prompt) if (t < 0 || t >= vocab[0]) { fprintf(stderr, "gl3_spec_draft_run: prompt id %d outside the vocabulary\n", t); return 2; }
    if (N > ctx_len) { fprintf(stderr, "gl3_spec_draft_run: the prompt (%d ids) does not fit the context (%d)\n", N, ctx_len); return 2; }

    gl3_ctx *target = nullptr, *draft = nullptr;
    gl3_model_desc opts{};
    opts.struct_size = sizeof(opts);
    opts.ctx = ctx_len;
    opts.max_batch = batch;
    opts.tp_size = 1;
    CK(target, gl3_load_gguf(path.c_str(), &opts, &target));
    CK(draft, gl3_load_gguf(draft_path.c_str(), &opts, &draft));

    std::vector<int32_t> generated, toks, seqs, poss, q_slots;
    std::vector<float> coins, draft_coins;
    std::vector<int8_t> none((size_t)batch, 0);
    L32X64MixRandom rng(seed);
    const double t_start = now_s();
    for (int c0 = 0; c0 < N - 1; c0 += batch) {      // all but the last prompt id, both plans: K / V rows only
        const int rows = c0 + batch < N - 1 ? batch : N - 1 - c0;
        seqs.assign((size_t)rows, 0);
        poss.resize((size_t)rows);
        for (int i = 0; i < rows; ++i) poss[i] = c0 + i;
        CK(target, gl3_forward_batch(target, prompt.data() + c0, seqs.data(), poss.data(), none.data(), rows, nullptr, nullptr));
        CK(draft, gl3_forward_prefill(draft, prompt.data() + c0, rows, c0));
    }
    const double t_decode = now_s();
    long steps = 0, drafted = 0, accepted = 0;
    double draft_s = 0;
    std::vector<double> len_s((size_t)batch + 1, 0.0);
    std::vector<long> len_n((size_t)batch + 1, 0);
    int pos = N - 1;                                  // position of the last real token
    int32_t last = prompt[N - 1];
    while ((int)generated.size() < n_new && pos < ctx_len) {
        int k = K;
        const int left = n_new - (int)generated.size();
        if (k > left - 1) k = left - 1;
        if (k > ctx_len - 1 - pos) k = ctx_len - 1 - pos;
        if (k > batch - 1) k = batch - 1;
        const int m = k + 1;
        toks.assign(1, last);
        q_slots.assign((size_t)m, -1);
        double t0 = now_s();
        if (chain && k > 0) {
            toks.resize((size_t)m);
            draft_coins.resize((size_t)k);
            if (sampled_draft) for (int j = 0; j < k; ++j) { draft_coins[j] = rng.nextFloat(); q_slots[j] = j; }
            CK(draft, gl3_forward_decode_chain(draft, last, pos, k, sampled_draft ? Td : 0.f, sampled_draft ? draft_coins.data() : nullptr,
                                               sampled_draft ? target : nullptr, 0, toks.data() + 1));
        }
        for (int j = 0; !chain && j < k; ++j) {
            int32_t id = 0;
            if (sampled_draft) {
                CK(draft, gl3_forward_decode_sample(draft, toks[j], pos + j, Td, 0.f, rng.nextFloat(), &id));
                CK(target, gl3_draft_probs_put(target, j, draft));
                q_slots[j] = j;
            } else {
                CK(draft, gl3_forward_decode(draft, toks[j], pos + j, nullptr, &id));
            }
            toks.push_back(id);
        }
        draft_s += now_s() - t0;
        coins.assign((size_t)2 * m, 0.f);
        if (T > 0.f) for (float& c : coins) c = rng.nextFloat();
        seqs.assign((size_t)m, 0);
        poss.resize((size_t)m);
        for (int i = 0; i < m; ++i) poss[i] = pos + i;
        gl3_verify_result res{};
        int32_t n_runs = 0;
        t0 = now_s();
        CK(target, gl3_forward_batch_verify_dist(target, toks.data(), seqs.data(), poss.data(), m, &T, coins.data(), q_slots.data(), &res, &n_runs));
        len_s[m] += now_s() - t0; ++len_n[m];
        ++steps; drafted += k; accepted += res.accepted;
        for (int i = 0; i < res.accepted; ++i) generated.push_back(toks[i + 1]);
        generated.push_back(res.token);
        if (res.accepted == k && (int)generated.size() < n_new && pos + k + 1 < ctx_len) {      // the id at pos + k has not been through the draft plan
            t0 = now_s();
            CK(draft, gl3_forward_decode(draft, toks[k], pos + k, nullptr, nullptr));
            draft_s += now_s() - t0;
        }
        pos += res.accepted + 1;
        last = res.token;
    }
    const double t_end = now_s();
    printf("generated:");
    for (int32_t v : generated) printf(" %d", v);
    printf("\n");
    fprintf(stderr, "steps=%ld drafted=%ld accepted=%ld tokens=%zu\n", steps, drafted, accepted, generated.size());
    fprintf(stderr, "timing: prefill_ms=%.1f decode_ms=%.1f tok_s=%.1f draft_ms=%.1f step_us=", (t_decode - t_start) * 1e3, (t_end - t_decode) * 1e3,
            generated.size() / (t_end - t_decode + 1e-12), draft_s * 1e3);
    bool first = true;
    for (int m = 1; m <= batch; ++m)
        if (len_n[m]) { fprintf(stderr, "%s%d:%.1f", first ? "" : ",", m, len_s[m] / len_n[m] * 1e6); first = false; }
    fprintf(stderr, "\n");
    gl3_destroy(draft);
    gl3_destroy(target);
    return 0;
}
