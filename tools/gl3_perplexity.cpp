// gl3_perplexity — perplexity of a model on a token stream over the C-ABI of libgpullama_hip.so (no Python, no torch), with the protocol of
// llama.cpp's llama-perplexity: the probabilities come from gl3_forward_batch_score, 16 bytes per scored row; no logits leave the device.
//
//   gl3_perplexity -m model.gguf --ids file -c CTX -b BATCH [-np SLOTS]
//
// The ids file holds one comma-separated id list (line breaks between ids are allowed).  The text is cut into windows of CTX tokens, a
// short tail is dropped.  Every window is forwarded from position 0 in a sequence slot of its own, and its rows at positions
// CTX/2 .. CTX-2 are scored against the token that follows them: CTX - 1 - CTX/2 scores per window, each with at least CTX/2 tokens of
// context.  Scheduling per step: the windows in the SLOTS slots, in slot order, each as one run of consecutive positions, up to BATCH rows;
// a window longer than the room left continues in the next step, and a slot whose window is done takes the next window (position 0
// again: no cache reset, attention reads nothing above a row's position).
//
// Arithmetic, all in double: ln p = (double) (logit - max) - log((double) sum) of the row's gl3_token_score (logit - max is the f32
// difference; prob itself underflows for unlikely tokens); a window's nll adds -ln p in position order starting from 0.0; the total adds
// the windows' nll in window order; ppl = exp(total / count).  Prints "window k: nll <%.17g> over <count>" per window and "ppl <%.17g>"
// (stdout), a summary (stderr).  Usage errors exit 2.
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../include/gpullama3_hip.h"

static double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// "1,2,3" -> ids (white space, line breaks included, around the ids); false for anything that is not a non-empty list of non-negative integers
static bool parse_id_list(const std::string& text, std::vector<int32_t>& out) {
    out.clear();
    const char* p = text.c_str();
    auto blank = [](char c) { return c == ' ' || c == '\t' || c == '\r' || c == '\n'; };
    while (true) {
        while (blank(*p)) ++p;
        if (*p < '0' || *p > '9') return false;
        char* e;
        const long x = strtol(p, &e, 10);
        if (x > 0x7FFFFFFF) return false;
        out.push_back((int32_t)x);
        p = e;
        while (blank(*p)) ++p;
        if (!*p) return true;
        if (*p != ',') return false;
        ++p;
    }
}

static int usage(const char* why) {
    fprintf(stderr, "gl3_perplexity: %s\nusage: gl3_perplexity -m model.gguf --ids file -c CTX -b BATCH [-np SLOTS]\n", why);
    return 2;
}

#define CK(call)                                                                                        \
    do {                                                                                                \
        const int32_t r_ = (call);                                                                      \
        if (r_ != GL3_OK) { fprintf(stderr, "%s failed (%d): %s\n", #call, r_, ctx ? gl3_last_error(ctx) : gl3_gguf_last_error(nullptr)); return 1; } \
    } while (0)

struct Slot {
    int win = -1;            // window in this slot, -1 = free
    int fed = 0;             // its tokens forwarded so far = position of its next row
};

int main(int argc, char** argv) {
    std::string path, ids_path;
    int n_ctx = 0, batch = 0, slots = 1;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto val = [&]() { return i + 1 < argc ? argv[++i] : (char*)""; };
        if (a == "-m") path = val();
        else if (a == "--ids") ids_path = val();
        else if (a == "-c") n_ctx = atoi(val());
        else if (a == "-b") batch = atoi(val());
        else if (a == "-np") slots = atoi(val());
        else return usage(("unknown argument " + a).c_str());
    }
    if (path.empty() || ids_path.empty()) return usage("-m model.gguf and --ids file are required");
    if (n_ctx < 3) return usage("-c must be at least 3 (a window scores its positions CTX/2 .. CTX-2)");
    if (batch < 2) return usage("-b must be at least 2");
    if (slots < 1) return usage("-np must be at least 1");

    std::vector<int32_t> ids;
    {
        std::ifstream f(ids_path);
        if (!f) return usage(("cannot open " + ids_path).c_str());
        std::stringstream ss;
        ss << f.rdbuf();
        if (!parse_id_list(ss.str(), ids)) return usage("malformed ids file: one comma-separated list of non-negative ids");
    }
    const int n_win = (int)(ids.size() / (size_t)n_ctx);
    if (n_win < 1) return usage("the ids file holds fewer than CTX ids");

    gl3_gguf* g = nullptr;
    gl3_model_desc d{};
    if (gl3_gguf_open(path.c_str(), &g) != GL3_OK || gl3_gguf_model_desc(g, &d, nullptr) != GL3_OK) { fprintf(stderr, "cannot read %s: %s\n", path.c_str(), gl3_gguf_last_error(g)); return 1; }
    gl3_gguf_close(g);
    for (int32_t t : ids) if (t >= d.vocab) return usage(("id " + std::to_string(t) + " outside the vocabulary").c_str());
    if (n_ctx > d.ctx) return usage("-c exceeds the model's context length");      // d.ctx: the file's context length clamped by the loader's default
    if (slots > n_win) slots = n_win;

    gl3_ctx* ctx = nullptr;
    gl3_model_desc opts{};
    opts.struct_size = sizeof(opts);
    opts.ctx = n_ctx;
    opts.max_batch = batch;
    opts.tp_size = 1;
    opts.n_seqs = slots;
    CK(gl3_load_gguf(path.c_str(), &opts, &ctx));

    const int first = n_ctx / 2, last = n_ctx - 2;      // scored positions of a window
    std::vector<double> nll((size_t)n_win, 0.0);
    std::vector<int> count((size_t)n_win, 0);
    std::vector<Slot> slot((size_t)slots);
    int next_win = 0, done = 0, steps = 0;
    long rows_total = 0;
    std::vector<int32_t> tokens, seqs, poss, targets;
    std::vector<int8_t> want;
    std::vector<int> out_win;            // window of every output row, in row order (a window's rows are in position order)
    std::vector<gl3_token_score> scores((size_t)batch);
    const double t0 = now_s();
    while (done < n_win) {
        for (Slot& s : slot)             // admission: the next window takes a free slot and starts at position 0
            if (s.win < 0 && next_win < n_win) { s.win = next_win++; s.fed = 0; }
        tokens.clear(); seqs.clear(); poss.clear(); want.clear(); targets.clear(); out_win.clear();
        for (int sl = 0; sl < slots && (int)tokens.size() < batch; ++sl) {
            Slot& s = slot[sl];
            if (s.win < 0) continue;
            const int32_t* w = ids.data() + (size_t)s.win * n_ctx;
            const int room = batch - (int)tokens.size(), left = n_ctx - s.fed;
            const int c = left < room ? left : room;
            for (int j = 0; j < c; ++j) {
                const int pos = s.fed + j;
                const bool scored = pos >= first && pos <= last;
                tokens.push_back(w[pos]); seqs.push_back(sl); poss.push_back(pos); want.push_back(scored ? 1 : 0);
                if (scored) { targets.push_back(w[pos + 1]); out_win.push_back(s.win); }
            }
            s.fed += c;
            if (s.fed == n_ctx) { s.win = -1; ++done; }
        }
        const int n = (int)tokens.size();
        CK(gl3_forward_batch_score(ctx, tokens.data(), seqs.data(), poss.data(), want.data(), n, targets.data(), nullptr, scores.data(), nullptr));
        ++steps; rows_total += n;
        for (size_t o = 0; o < out_win.size(); ++o) {
            const gl3_token_score& sc = scores[o];
            const double lnp = (double)(sc.logit - sc.max) - log((double)sc.sum);
            nll[out_win[o]] += -lnp;
            ++count[out_win[o]];
        }
    }
    const double t1 = now_s();
    double total = 0.0;
    long total_count = 0;
    for (int k = 0; k < n_win; ++k) {
        printf("window %d: nll %.17g over %d\n", k, nll[k], count[k]);
        total += nll[k];
        total_count += count[k];
    }
    printf("ppl %.17g\n", exp(total / (double)total_count));
    fprintf(stderr, "%d windows of %d tokens on %d slots, %d steps, %ld rows (%ld scored) in %.1f ms (%.1f rows/s)\n", n_win, n_ctx, slots, steps, rows_total,
            total_count, (t1 - t0) * 1e3, rows_total / (t1 - t0 + 1e-12));
    gl3_destroy(ctx);
    return 0;
}
