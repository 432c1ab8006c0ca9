// gl3_spec_batch_run — continuous-batching speculative decoding with a DRAFT MODEL over the C-ABI of libgpullama_hip.so (no Python, no
// torch): many requests share the sequence slots of two plans on one device.  Every step the draft plan drafts for ALL running requests in
// ONE gl3_forward_decode_batch_chain — k static-batched steps behind one host wait, one pass over the draft's weights per step whatever the
// number of requests — and ONE gl3_forward_batch_verify_dist on the target verifies every request's run in one pass over the target's weights.
//
//   gl3_spec_batch_run -m target.gguf -md draft.gguf --prompts ids.txt -np NP -n NEW [--draft K] [-b BATCH] [--temperature T]
//                      [--draft-temperature Td] [--seed S] [--no-chain]
//
// The prompts file has one comma-separated id list per line (tools/gl3_batch_run's format); one "request r: id id ..." line per request comes
// out, r = line order.  Both plans have NP sequence slots; the target's max_batch is BATCH (default NP * (K + 1), and never less: exit 2), the
// draft's max(NP, 2).  Request r owns an L32X64MixRandom seeded S + r (default S = 1234), takes the lowest free slot in request order and
// leaves when it has NEW ids.  Per request the protocol is tools/gl3_spec_draft_run's, so request r's ids are those of
// gl3_spec_draft_run --seed S+r on its prompt with the same --draft, and at --temperature 0 those of plain greedy decoding.
//   admission  all but the request's last prompt id through gl3_forward_batch (no output rows) on both plans, on the request's slot.
// A step, over the running requests (last real token at position p):
//   catch-up   the requests whose drafts all stood in their last step have not had the id at p through the draft plan (it was the target's,
//              not a draft's input): ONE gl3_forward_batch on the draft plan, no output rows, feeds each of them the id before `last`.
//   k          k_r = min(K, ids still wanted - 1, context left), as the single-sequence host.
//   drafting   the requests with k_r >= 1, sorted by k_r descending (stable by slot), are the rows of ONE gl3_forward_decode_batch_chain on
//              the draft plan with k_rows = their k_r.  T > 0 and Td > 0 (default Td = T): row temperature Td, the request's k_r coins, and
//              slots[i] = the row index of the request's first draft in the verify step, so the chain files every draft's distribution in the
//              target's table.  Else greedy rows (temperature 0, slot -1: the one-hot rule).
//              --no-chain: the same step as k calls of gl3_forward_decode_batch_sample over the shrinking row prefix, each followed by
//              gl3_draft_probs_put_row for the rows with a slot: a host wait and a token upload per drafted position.  The same coins, so
//              the same ids and counts.
//   verifying  ONE gl3_forward_batch_verify_dist on the target: per running request, in slot order, the run [last real token, drafts] of
//              k_r + 1 rows; q_slots of the row in front of draft j = slots + j, -1 elsewhere.
//   appending  request r takes its a drafts and the token; a finished request frees its slot for the next waiting one.
//   coins      request r's generator, per step: first one nextFloat per sampled draft, then (T > 0) 2 (k_r + 1) verify coins in row order.
// stderr: the line "steps=… drafted=… accepted=… tokens=…" (steps = verify calls), then a line "timing: …" with the loop's host-clock times
// (prefill_ms = admission, decode_ms = the rest, tok_s, draft_ms = the part of decode_ms spent in the draft plan, draft_calls = forward calls
// on the draft plan while drafting and catching up, each of which waits for the device once, step_us=rows:mean microseconds of a verify step
// by row count).
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
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

// "1,2,3" -> ids; false for anything that is not a non-empty list of non-negative integers (tools/gl3_batch_run.cpp)
static bool parse_id_list(const std::string& line, std::vector<int32_t>& out) {
    out.clear();
    const char* p = line.c_str();
    while (true) {
        while (*p == ' ' || *p == '\t') ++p;
        if (*p < '0' || *p > '9') return false;
        char* e;
        const long x = strtol(p, &e, 10);
        if (x > 0x7FFFFFFF) return false;
        out.push_back((int32_t)x);
        p = e;
        while (*p == ' ' || *p == '\t' || *p == '\r') ++p;
        if (!*p) return true;
        if (*p != ',') return false;
        ++p;
    }
}

static int usage(const char* why) {
    fprintf(stderr, "gl3_spec_batch_run: %s\nusage: gl3_spec_batch_run -m target.gguf -md draft.gguf --prompts file -np NP -n NEW [--draft K] [-b BATCH] "
                    "[--temperature T] [--draft-temperature Td] [--seed S] [--no-chain]\n", why);
    return 2;
}

#define CK(ctx, call)                                                                                   \
    do {                                                                                                \
        const int32_t r_ = (call);                                                                      \
        if (r_ != GL3_OK) { fprintf(stderr, "%s failed (%d): %s\n", #call, r_, ctx ? gl3_last_error(ctx) : gl3_gguf_last_error(nullptr)); return 1; } \
    } while (0)

struct Request {
    std::vector<int32_t> prompt, generated;
    L32X64MixRandom rng{0};
};
struct Slot {
    int req = -1;            // request in this slot, -1 = free
    int pos = 0;             // position of the last real token
    int32_t last = 0;        // the last real token
    int32_t behind = 0;      // the id at pos - 1 (what a catch-up feeds the draft plan)
    bool catch_up = false;   // every draft of the last step stood: the draft plan has not seen the id at pos - 1
    int k = 0, row0 = 0;     // this step: drafts, first row of the run in the verify step
};

int main(int argc, char** argv) {
    std::string path, draft_path, prompts_path;
    int np = 0, n_new = 0, K = 4, batch = 0;
    float T = 0.f, Td = -1.f;
    uint64_t seed = 1234;
    bool chain = true;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto val = [&]() { return i + 1 < argc ? argv[++i] : (char*)""; };
        if (a == "-m") path = val();
        else if (a == "-md") draft_path = val();
        else if (a == "--prompts") prompts_path = val();
        else if (a == "-np") np = atoi(val());
        else if (a == "-n") n_new = atoi(val());
        else if (a == "--draft") K = atoi(val());
        else if (a == "-b") batch = atoi(val());
        else if (a == "--temperature") T = (float)atof(val());
        else if (a == "--draft-temperature") Td = (float)atof(val());
        else if (a == "--seed") seed = strtoull(val(), nullptr, 10);
        else if (a == "--no-chain") chain = false;
        else return usage(("unknown argument " + a).c_str());
    }
    if (path.empty() || draft_path.empty() || prompts_path.empty()) return usage("-m target.gguf, -md draft.gguf and --prompts file are required");
    if (np < 1) return usage("-np must be at least 1");
    if (n_new < 1) return usage("-n must be at least 1");
    if (Td < 0.f) Td = T;
    if (K < 0 || K > GL3_CHAIN_MAX || !(T >= 0.f) || !(Td >= 0.f)) return usage("--draft in [0, GL3_CHAIN_MAX], temperatures >= 0");
    if (batch == 0) batch = np * (K + 1) < 2 ? 2 : np * (K + 1);
    if (batch < 2 || batch < np * (K + 1)) return usage("-b must be at least 2 and at least NP * (K + 1): every running request's run in one verify step");
    const bool sampled_draft = T > 0.f && Td > 0.f;

    std::vector<Request> reqs;
    {
        std::ifstream f(prompts_path);
        if (!f) return usage(("cannot open " + prompts_path).c_str());
        std::string line;
        int ln = 0;
        while (std::getline(f, line)) {
            ++ln;
            if (line.find_first_not_of(" \t\r") == std::string::npos) continue;
            Request r;
            if (!parse_id_list(line, r.prompt)) return usage(("malformed prompts file, line " + std::to_string(ln)).c_str());
            r.rng = L32X64MixRandom(seed + reqs.size());
            reqs.push_back(std::move(r));
        }
    }
    if (reqs.empty()) return usage("the prompts file holds no request");
    size_t longest = 0;
    for (const Request& r : reqs) longest = r.prompt.size() > longest ? r.prompt.size() : longest;
    const int need = (int)longest + n_new;
    int vocab[2] = {0, 0};
    for (int w = 0; w < 2; ++w) {
        const std::string& f = w ? draft_path : path;
        gl3_gguf* g = nullptr;
        gl3_model_desc d{};
        if (gl3_gguf_open(f.c_str(), &g) != GL3_OK || gl3_gguf_model_desc(g, &d, nullptr) != GL3_OK) { fprintf(stderr, "cannot read %s: %s\n", f.c_str(), gl3_gguf_last_error(g)); return 1; }
        gl3_gguf_close(g);
        if (need > d.ctx) return usage("a prompt plus -n exceeds a model's context length");
        vocab[w] = d.vocab;
    }
    if (vocab[0] != vocab[1]) return usage("the draft model's vocabulary is not the target's");
    for (const Request& r : reqs)
        for (int32_t t : r.prompt) if (t >= vocab[0]) return usage(("prompt id " + std::to_string(t) + " outside the vocabulary").c_str());

    gl3_ctx *target = nullptr, *draft = nullptr;
    gl3_model_desc opts{};
    opts.struct_size = sizeof(opts);
    opts.ctx = need;
    opts.tp_size = 1;
    opts.n_seqs = np;
    opts.max_batch = batch;
    CK(target, gl3_load_gguf(path.c_str(), &opts, &target));
    const int draft_batch = np < 2 ? 2 : np;
    opts.max_batch = draft_batch;
    CK(draft, gl3_load_gguf(draft_path.c_str(), &opts, &draft));

    std::vector<Slot> slot((size_t)np);
    size_t next_req = 0, finished = 0;
    std::vector<int32_t> toks, seqs, poss, q_slots;
    std::vector<int32_t> d_toks, d_seqs, d_poss, d_krows, d_slots, d_out, d_step;
    std::vector<float> coins, d_temp, d_coins, run_T, zeros((size_t)draft_batch, 0.f);
    std::vector<int8_t> none((size_t)(batch > draft_batch ? batch : draft_batch), 0);
    std::vector<gl3_verify_result> res((size_t)batch);
    std::vector<int> order;
    long steps = 0, drafted = 0, accepted = 0, draft_calls = 0;
    size_t tokens_total = 0;
    double draft_s = 0, prefill_s = 0;
    std::vector<double> len_s((size_t)batch + 1, 0.0);
    std::vector<long> len_n((size_t)batch + 1, 0);
    const double t_start = now_s();
    while (finished < reqs.size()) {
        for (int f = 0; f < np; ++f) {      // admission: all but the last prompt id on both plans, K / V rows only
            Slot& s = slot[f];
            if (s.req >= 0 || next_req >= reqs.size()) continue;
            s.req = (int)next_req++;
            const std::vector<int32_t>& pr = reqs[s.req].prompt;
            const int N = (int)pr.size();
            const double t0 = now_s();
            for (int w = 0; w < 2; ++w) {
                gl3_ctx* plan = w ? draft : target;
                const int cap = w ? draft_batch : batch;
                for (int c0 = 0; c0 < N - 1; c0 += cap) {
                    const int rows = c0 + cap < N - 1 ? cap : N - 1 - c0;
                    seqs.assign((size_t)rows, f);
                    poss.resize((size_t)rows);
                    for (int i = 0; i < rows; ++i) poss[i] = c0 + i;
                    CK(plan, gl3_forward_batch(plan, pr.data() + c0, seqs.data(), poss.data(), none.data(), rows, nullptr, nullptr));
                }
            }
            prefill_s += now_s() - t0;
            s.pos = N - 1; s.last = pr[N - 1]; s.behind = 0; s.catch_up = false;
        }
        // catch-up: one mixed step on the draft plan for the requests whose drafts all stood
        d_toks.clear(); d_seqs.clear(); d_poss.clear();
        for (int f = 0; f < np; ++f) {
            Slot& s = slot[f];
            if (s.req < 0 || !s.catch_up) continue;
            d_toks.push_back(s.behind); d_seqs.push_back(f); d_poss.push_back(s.pos - 1);
            s.catch_up = false;
        }
        if (!d_toks.empty()) {
            const double t0 = now_s();
            CK(draft, gl3_forward_batch(draft, d_toks.data(), d_seqs.data(), d_poss.data(), none.data(), (int32_t)d_toks.size(), nullptr, nullptr));
            draft_s += now_s() - t0; ++draft_calls;
        }
        // k per request, the rows of the verify step in slot order, the rows of the chain by k descending
        int m_total = 0;
        order.clear();
        for (int f = 0; f < np; ++f) {
            Slot& s = slot[f];
            if (s.req < 0) continue;
            int k = K;
            const int left = n_new - (int)reqs[s.req].generated.size();
            if (k > left - 1) k = left - 1;
            if (k > need - 1 - s.pos) k = need - 1 - s.pos;
            s.k = k; s.row0 = m_total;
            m_total += k + 1;
            if (k >= 1) order.push_back(f);
        }
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return slot[a].k > slot[b].k; });
        toks.assign((size_t)m_total, 0); seqs.resize((size_t)m_total); poss.resize((size_t)m_total);
        q_slots.assign((size_t)m_total, -1);
        coins.assign((size_t)2 * m_total, 0.f);
        const int n = (int)order.size(), kmax = n ? slot[order[0]].k : 0;
        if (n) {
            d_toks.resize((size_t)n); d_seqs.resize((size_t)n); d_poss.resize((size_t)n); d_krows.resize((size_t)n); d_slots.resize((size_t)n);
            d_temp.assign((size_t)n, sampled_draft ? Td : 0.f);
            d_coins.assign((size_t)kmax * n, 0.f);
            d_out.assign((size_t)kmax * n, -1);
            for (int i = 0; i < n; ++i) {
                Slot& s = slot[order[i]];
                d_toks[i] = s.last; d_seqs[i] = order[i]; d_poss[i] = s.pos; d_krows[i] = s.k;
                d_slots[i] = sampled_draft ? s.row0 + 1 : -1;
                if (sampled_draft) for (int j = 0; j < s.k; ++j) { d_coins[(size_t)j * n + i] = reqs[s.req].rng.nextFloat(); q_slots[s.row0 + j] = s.row0 + 1 + j; }
            }
            const double t0 = now_s();
            if (chain) {
                CK(draft, gl3_forward_decode_batch_chain(draft, d_toks.data(), d_seqs.data(), d_poss.data(), n, kmax, d_krows.data(), d_temp.data(),
                                                         sampled_draft ? d_coins.data() : nullptr, sampled_draft ? target : nullptr,
                                                         sampled_draft ? d_slots.data() : nullptr, d_out.data()));
                ++draft_calls;
            } else {
                d_step = d_toks;
                for (int j = 0; j < kmax; ++j) {
                    int nj = 0;
                    while (nj < n && d_krows[nj] > j) ++nj;
                    for (int i = 0; i < nj; ++i) d_poss[i] = slot[order[i]].pos + j;
                    CK(draft, gl3_forward_decode_batch_sample(draft, d_step.data(), d_seqs.data(), d_poss.data(), nj, d_temp.data(), zeros.data(),
                                                              d_coins.data() + (size_t)j * n, d_out.data() + (size_t)j * n));
                    ++draft_calls;
                    for (int i = 0; i < nj; ++i) {
                        d_step[i] = d_out[(size_t)j * n + i];
                        if (d_slots[i] >= 0) CK(target, gl3_draft_probs_put_row(target, d_slots[i] + j, draft, i));
                    }
                }
            }
            draft_s += now_s() - t0;
            for (int i = 0; i < n; ++i) {
                const Slot& s = slot[order[i]];
                for (int j = 0; j < s.k; ++j) toks[s.row0 + 1 + j] = d_out[(size_t)j * n + i];
            }
        }
        run_T.clear();
        for (int f = 0; f < np; ++f) {
            Slot& s = slot[f];
            if (s.req < 0) continue;
            toks[s.row0] = s.last;
            for (int i = 0; i <= s.k; ++i) { seqs[s.row0 + i] = f; poss[s.row0 + i] = s.pos + i; }
            if (T > 0.f) for (int i = 0; i < 2 * (s.k + 1); ++i) coins[(size_t)2 * s.row0 + i] = reqs[s.req].rng.nextFloat();
            run_T.push_back(T);
        }
        int32_t n_runs = 0;
        const double t0 = now_s();
        CK(target, gl3_forward_batch_verify_dist(target, toks.data(), seqs.data(), poss.data(), m_total, run_T.data(), coins.data(), q_slots.data(), res.data(), &n_runs));
        len_s[m_total] += now_s() - t0; ++len_n[m_total];
        ++steps;
        int run = 0;
        for (int f = 0; f < np; ++f) {
            Slot& s = slot[f];
            if (s.req < 0) continue;
            Request& r = reqs[s.req];
            const gl3_verify_result& v = res[run++];
            drafted += s.k; accepted += v.accepted;
            for (int i = 0; i < v.accepted; ++i) r.generated.push_back(toks[s.row0 + 1 + i]);
            r.generated.push_back(v.token);
            tokens_total += v.accepted + 1;
            s.behind = toks[s.row0 + v.accepted];      // the id in front of the new last token
            s.catch_up = v.accepted == s.k;            // it was the last draft (or, k == 0, the last real token): not yet through the draft plan
            s.pos += v.accepted + 1;
            s.last = v.token;
            if ((int)r.generated.size() >= n_new) { s.req = -1; ++finished; }
        }
        if (run != n_runs) { fprintf(stderr, "gl3_spec_batch_run: the verify step found %d runs, %d requests are running\n", n_runs, run); return 1; }
    }
    const double t_end = now_s();
    for (size_t k = 0; k < reqs.size(); ++k) {
        printf("request %zu:", k);
        for (int32_t v : reqs[k].generated) printf(" %d", v);
        printf("\n");
    }
    const double decode_s = t_end - t_start - prefill_s;
    fprintf(stderr, "steps=%ld drafted=%ld accepted=%ld tokens=%zu\n", steps, drafted, accepted, tokens_total);
    fprintf(stderr, "timing: prefill_ms=%.1f decode_ms=%.1f tok_s=%.1f draft_ms=%.1f draft_calls=%ld step_us=", prefill_s * 1e3, decode_s * 1e3,
            tokens_total / (decode_s + 1e-12), draft_s * 1e3, draft_calls);
    bool first = true;
    for (int m = 1; m <= batch; ++m)
        if (len_n[m]) { fprintf(stderr, "%s%d:%.1f", first ? "" : ",", m, len_s[m] / len_n[m] * 1e6); first = false; }
    fprintf(stderr, "\n");
    gl3_destroy(draft);
    gl3_destroy(target);
    return 0;
}
