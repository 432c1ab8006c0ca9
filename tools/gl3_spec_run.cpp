// gl3_spec_run — greedy speculative decoding of ONE sequence over the C-ABI of libgpullama_hip.so (no Python, no torch): prompt-lookup
// drafting on the host, every step ONE gl3_forward_batch_verify call that forwards the last real token and the drafts in one pass over the
// weights and decides on the device how many drafts stand (8 bytes come back).  Greedy verification emits exactly the ids that decoding one
// token per step emits, so the output is that of a plain greedy loop over the same (token, position) sequence.
//
//   gl3_spec_run -m model.gguf --ids 1,2,3 -n NEW [--draft K] [--ngram G] [-b BATCH] [--stop id,id]
//
// Positions: prompt id k at position k, generated ids behind them, no begin-of-text of the tool's own.  All but the last prompt id are
// prefilled with gl3_forward_batch (no output rows) in runs of up to -b rows (default 16).  A step is the run [last real token, drafts]:
//   drafting   for g = G (default 3) down to 1: the most recent EARLIER occurrence of the last g ids of the history (prompt + generated);
//              the up-to-K (default 4) ids that followed it are the drafts.  No match: a run of one row.  Drafts are clipped so that no
//              run passes the context, -b rows or -n: a step with k drafts emits at most k + 1 ids.
//   result     {a, token}: the first a drafts and `token` are appended; the next run starts a + 1 positions on and overwrites the K / V
//              rows of the rejected drafts before anything reads them.
// --draft 0 is plain decoding through the same entry.  A stop id ends generation AT the stop id (it is printed), also when drafts behind
// it were accepted.  stdout: "generated: id id ...".  stderr: the line "steps=… drafted=… accepted=… tokens=…", then a line "timing: …" with
// the loop's host-clock times (prefill_ms, decode_ms, tok_s, step_us=rows:mean microseconds of a step by run length).
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>
#include <vector>

#include "../include/gpullama3_hip.h"

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

// prompt lookup: the ids behind the most recent earlier occurrence of the longest matching suffix (g = ngram .. 1), at most k of them
static std::vector<int32_t> draft(const std::vector<int32_t>& h, int ngram, int k) {
    const int n = (int)h.size();
    if (k <= 0) return {};
    for (int g = ngram < n - 1 ? ngram : n - 1; g >= 1; --g)
        for (int s = n - g - 1; s >= 0; --s) {
            bool same = true;
            for (int i = 0; i < g && same; ++i) same = h[s + i] == h[n - g + i];
            if (!same) continue;
            const int e = s + g + k < n ? s + g + k : n;
            return std::vector<int32_t>(h.begin() + s + g, h.begin() + e);
        }
    return {};
}

#define CK(call)                                                                                        \
    do {                                                                                                \
        const int32_t r_ = (call);                                                                      \
        if (r_ != GL3_OK) { fprintf(stderr, "%s failed (%d): %s\n", #call, r_, ctx ? gl3_last_error(ctx) : gl3_gguf_last_error(nullptr)); return 1; } \
    } while (0)

int main(int argc, char** argv) {
    std::string path;
    std::vector<int32_t> prompt, stop;
    int n_new = 0, K = 4, G = 3, batch = 16;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto val = [&]() { return i + 1 < argc ? argv[++i] : (char*)""; };
        if (a == "-m") path = val();
        else if (a == "--ids") prompt = parse_ids(val());
        else if (a == "-n") n_new = atoi(val());
        else if (a == "--draft") K = atoi(val());
        else if (a == "--ngram") G = atoi(val());
        else if (a == "-b") batch = atoi(val());
        else if (a == "--stop") stop = parse_ids(val());
        else { fprintf(stderr, "gl3_spec_run: unknown argument %s (see the header of tools/gl3_spec_run.cpp)\n", a.c_str()); return 2; }
    }
    if (path.empty() || prompt.empty() || n_new <= 0) { fprintf(stderr, "gl3_spec_run: -m model.gguf, --ids a,b,c and -n NEW (> 0) are required\n"); return 2; }
    if (K < 0 || G < 1 || batch < 2) { fprintf(stderr, "gl3_spec_run: --draft >= 0, --ngram >= 1, -b >= 2\n"); return 2; }

    const int N = (int)prompt.size();
    gl3_gguf* g = nullptr;
    gl3_model_desc d{};
    d.ctx = N + n_new;      // kept if the file's context length admits it, else clamped to it: the plan's context bounds the loop
    if (gl3_gguf_open(path.c_str(), &g) != GL3_OK || gl3_gguf_model_desc(g, &d, nullptr) != GL3_OK) { fprintf(stderr, "cannot read %s: %s\n", path.c_str(), gl3_gguf_last_error(g)); return 1; }
    gl3_gguf_close(g);
    for (int32_t t : prompt) if (t < 0 || t >= d.vocab) { fprintf(stderr, "gl3_spec_run: prompt id %d outside the vocabulary\n", t); return 2; }
    const int ctx_len = d.ctx;
    if (N > ctx_len) { fprintf(stderr, "gl3_spec_run: the prompt (%d ids) does not fit the context (%d)\n", N, ctx_len); return 2; }

    gl3_ctx* ctx = nullptr;
    gl3_model_desc opts{};
    opts.struct_size = sizeof(opts);
    opts.ctx = ctx_len;
    opts.max_batch = batch;
    opts.tp_size = 1;
    CK(gl3_load_gguf(path.c_str(), &opts, &ctx));

    const std::set<int32_t> stop_set(stop.begin(), stop.end());
    std::vector<int32_t> history = prompt, generated, toks, seqs, poss;
    std::vector<int8_t> none((size_t)batch, 0);
    const double t_start = now_s();
    for (int c0 = 0; c0 < N - 1; c0 += batch) {      // all but the last prompt id: K / V rows only, no output row
        const int rows = c0 + batch < N - 1 ? batch : N - 1 - c0;
        seqs.assign((size_t)rows, 0);
        poss.resize((size_t)rows);
        for (int i = 0; i < rows; ++i) poss[i] = c0 + i;
        CK(gl3_forward_batch(ctx, prompt.data() + c0, seqs.data(), poss.data(), none.data(), rows, nullptr, nullptr));
    }
    const double t_decode = now_s();
    long steps = 0, drafted = 0, accepted = 0;
    std::vector<double> len_s((size_t)batch + 1, 0.0);
    std::vector<long> len_n((size_t)batch + 1, 0);
    int pos = N - 1;                                  // position of the last real token
    bool stopped = false;
    while (!stopped && (int)generated.size() < n_new && pos < ctx_len) {
        int k = K;
        const int left = n_new - (int)generated.size();
        if (k > left - 1) k = left - 1;
        if (k > ctx_len - 1 - pos) k = ctx_len - 1 - pos;
        if (k > batch - 1) k = batch - 1;
        const std::vector<int32_t> dr = draft(history, G, k);
        const int m = 1 + (int)dr.size();
        toks.assign(1, history.back());
        toks.insert(toks.end(), dr.begin(), dr.end());
        seqs.assign((size_t)m, 0);
        poss.resize((size_t)m);
        for (int i = 0; i < m; ++i) poss[i] = pos + i;
        gl3_verify_result res{};
        int32_t n_runs = 0;
        const double t0 = now_s();
        CK(gl3_forward_batch_verify(ctx, toks.data(), seqs.data(), poss.data(), m, nullptr, nullptr, &res, &n_runs));
        len_s[m] += now_s() - t0; ++len_n[m];
        ++steps; drafted += m - 1; accepted += res.accepted;
        for (int i = 0; i <= res.accepted && !stopped; ++i) {
            const int32_t id = i < res.accepted ? dr[i] : res.token;
            generated.push_back(id);
            history.push_back(id);
            stopped = stop_set.count(id) != 0;
        }
        pos += res.accepted + 1;
    }
    const double t_end = now_s();
    printf("generated:");
    for (int32_t v : generated) printf(" %d", v);
    printf("\n");
    fprintf(stderr, "steps=%ld drafted=%ld accepted=%ld tokens=%zu\n", steps, drafted, accepted, generated.size());
    fprintf(stderr, "timing: prefill_ms=%.1f decode_ms=%.1f tok_s=%.1f step_us=", (t_decode - t_start) * 1e3, (t_end - t_decode) * 1e3,
            generated.size() / (t_end - t_decode + 1e-12));
    bool first = true;
    for (int m = 1; m <= batch; ++m)
        if (len_n[m]) { fprintf(stderr, "%s%d:%.1f", first ? "" : ",", m, len_s[m] / len_n[m] * 1e6); first = false; }
    fprintf(stderr, "\n");
    gl3_destroy(ctx);
    return 0;
}
