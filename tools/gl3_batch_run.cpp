// gl3_batch_run — continuous-batching generation loop over the C-ABI of libgpullama_hip.so (no Python, no torch): many requests share
// the plan's sequence slots, and every step is ONE gl3_forward_batch — the decode rows of the running requests and prompt chunks of the
// newly admitted ones in the same pass over the weights.
//
//   gl3_batch_run -m model.gguf --prompts file -np SLOTS -b BATCH -n NEW [--stop id,id] [--share-prefix]
//
// The prompts file has one comma-separated id list per line (one request per line, blank lines ignored).  Prints one
// "request k: id id ..." line per request (stdout, k = line order) and a summary (stderr).
//
// Protocol per request: prompt token j at position j; the first generated id is the greedy id (first index of the maximum) of the last
// prompt row; each generated id is forwarded at the next position, until NEW ids or a stop id (which is part of the result).
// Scheduling per step: one decode row per running request, then prompt tokens of admitted requests, in slot order, up to BATCH rows; a
// prompt longer than the room left continues in the next step (a continuation chunk).  A waiting request takes a slot as soon as one
// finishes and starts again at position 0 there: no cache reset, attention reads nothing above a row's position.
//
// --share-prefix: prefix reuse.  Every slot remembers `hist`, the tokens whose K / V rows it holds at positions 0 .. hist.size() - 1 (prompt
// tokens and generated ids forwarded in a completed step; it outlives its request).  A request admitted to free slot f looks at every slot s,
// f itself and the running ones included, for c_s = the length of the common prefix of its prompt and s.hist, capped at prompt length - 1 (the
// last prompt token must be forwarded to get the first id), and takes the largest (ties: f itself, then the lowest slot).  c == 0: position 0
// as above.  Best slot f itself: it starts at position c with nothing copied ("in place").  Another slot: gl3_kv_seq_copy(s -> f, rows [0, c))
// and it starts at position c.  Admissions happen one after another in slot order, each seeing the hist the previous one left.  The rows are
// bit for bit what forwarding the prefix would have written, so the printed ids are the same with and without the flag; the summary gains
// the line "prefix rows reused: R (C copied in K calls, P in place)" and the first line's rows count is smaller by R.
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <set>
#include <string>
#include <vector>

#include "../include/gpullama3_hip.h"

static double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// "1,2,3" -> ids; false for anything that is not a non-empty list of non-negative integers
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
    fprintf(stderr, "gl3_batch_run: %s\nusage: gl3_batch_run -m model.gguf --prompts file -np SLOTS -b BATCH -n NEW [--stop id,id] [--share-prefix]\n", why);
    return 2;
}

#define CK(call)                                                                                        \
    do {                                                                                                \
        const int32_t r_ = (call);                                                                      \
        if (r_ != GL3_OK) { fprintf(stderr, "%s failed (%d): %s\n", #call, r_, ctx ? gl3_last_error(ctx) : gl3_gguf_last_error(nullptr)); return 1; } \
    } while (0)

struct Request {
    std::vector<int32_t> prompt, generated;
};
struct Slot {
    int req = -1;            // request in this slot, -1 = free
    int fed = 0;             // prompt tokens forwarded so far
    int pos = 0;             // position of the next row
    int32_t cur = 0;         // decode: the id to forward next
    std::vector<int32_t> hist;   // --share-prefix: the tokens whose K / V rows the slot holds at positions 0 .. hist.size() - 1
};

int main(int argc, char** argv) {
    std::string path, prompts_path;
    int slots = 0, batch = 0, n_new = 0;
    std::vector<int32_t> stop;
    bool share_prefix = false;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto val = [&]() { return i + 1 < argc ? argv[++i] : (char*)""; };
        if (a == "-m") path = val();
        else if (a == "--prompts") prompts_path = val();
        else if (a == "-np") slots = atoi(val());
        else if (a == "-b") batch = atoi(val());
        else if (a == "-n") n_new = atoi(val());
        else if (a == "--stop") { if (!parse_id_list(val(), stop)) return usage("--stop takes a comma-separated id list"); }
        else if (a == "--share-prefix") share_prefix = true;
        else return usage(("unknown argument " + a).c_str());
    }
    if (path.empty() || prompts_path.empty()) return usage("-m model.gguf and --prompts file are required");
    if (slots < 1) return usage("-np must be at least 1");
    if (n_new < 1) return usage("-n must be at least 1");
    if (batch < 2 || batch < slots) return usage("-b must be at least 2 and at least -np (one decode row per running request)");

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
            reqs.push_back(std::move(r));
        }
    }
    if (reqs.empty()) return usage("the prompts file holds no request");

    gl3_gguf* g = nullptr;
    gl3_model_desc d{};
    if (gl3_gguf_open(path.c_str(), &g) != GL3_OK || gl3_gguf_model_desc(g, &d, nullptr) != GL3_OK) { fprintf(stderr, "cannot read %s: %s\n", path.c_str(), gl3_gguf_last_error(g)); return 1; }
    gl3_gguf_close(g);
    size_t longest = 0;
    for (const Request& r : reqs) {
        for (int32_t t : r.prompt) if (t >= d.vocab) return usage(("prompt id " + std::to_string(t) + " outside the vocabulary").c_str());
        longest = r.prompt.size() > longest ? r.prompt.size() : longest;
    }
    // a request's last forwarded row sits at prompt + NEW - 2; d.ctx is the file's context length clamped by the loader's default
    const int need = (int)longest + n_new;
    if (need > d.ctx) return usage("a prompt plus -n exceeds the model's context length");

    gl3_ctx* ctx = nullptr;
    gl3_model_desc opts{};
    opts.struct_size = sizeof(opts);
    opts.ctx = need;
    opts.max_batch = batch;
    opts.tp_size = 1;
    opts.n_seqs = slots;
    CK(gl3_load_gguf(path.c_str(), &opts, &ctx));

    const std::set<int32_t> stop_set(stop.begin(), stop.end());
    std::vector<Slot> slot((size_t)slots);
    size_t next_req = 0, finished = 0;
    std::vector<int32_t> tokens, seqs, poss, amax((size_t)batch);
    std::vector<int8_t> want;
    std::vector<int> out_slot;           // slot of every output row, in row order
    int steps = 0, mixed_steps = 0;
    long rows_total = 0, rows_copied = 0, rows_in_place = 0;
    int copy_calls = 0;
    const double t0 = now_s();
    while (finished < reqs.size()) {
        for (int f = 0; f < slots; ++f) {      // admission: a waiting request takes a free slot and starts at position 0, or behind a shared prefix
            Slot& s = slot[f];
            if (s.req >= 0 || next_req >= reqs.size()) continue;
            s.req = (int)next_req++; s.fed = s.pos = 0; s.cur = 0;
            if (!share_prefix) continue;
            const std::vector<int32_t>& pr = reqs[s.req].prompt;
            auto common = [&](const std::vector<int32_t>& h) {
                size_t c = 0;
                while (c + 1 < pr.size() && c < h.size() && h[c] == pr[c]) ++c;
                return (int)c;
            };
            int best = f, c = common(s.hist);
            for (int o = 0; o < slots; ++o) {
                const int co = o == f ? 0 : common(slot[o].hist);
                if (co > c) { best = o; c = co; }
            }
            if (c > 0 && best != f) {
                const int32_t dst = f;
                CK(gl3_kv_seq_copy(ctx, best, &dst, 1, 0, c));
                ++copy_calls; rows_copied += c;
            } else rows_in_place += c;
            s.hist.assign(pr.begin(), pr.begin() + c);
            s.fed = s.pos = c;
        }
        tokens.clear(); seqs.clear(); poss.clear(); want.clear(); out_slot.clear();
        auto row = [&](int32_t tok, int sl, int pos, bool w) {
            tokens.push_back(tok); seqs.push_back(sl); poss.push_back(pos); want.push_back(w ? 1 : 0);
            if (w) out_slot.push_back(sl);
        };
        for (int sl = 0; sl < slots; ++sl) {                         // one decode row per running request
            Slot& s = slot[sl];
            if (s.req >= 0 && s.fed == (int)reqs[s.req].prompt.size()) row(s.cur, sl, s.pos++, true);
        }
        const size_t n_decode = tokens.size();
        for (int sl = 0; sl < slots && (int)tokens.size() < batch; ++sl) {      // then prompt chunks, up to BATCH rows
            Slot& s = slot[sl];
            if (s.req < 0) continue;
            const std::vector<int32_t>& pr = reqs[s.req].prompt;
            if (s.fed == (int)pr.size()) continue;                       // running: its decode row is in the step already
            const int room = batch - (int)tokens.size(), left = (int)pr.size() - s.fed;
            const int c = left < room ? left : room;
            for (int j = 0; j < c; ++j) row(pr[s.fed + j], sl, s.pos + j, s.fed + j + 1 == (int)pr.size());
            s.fed += c; s.pos += c;
        }
        const int n = (int)tokens.size();
        CK(gl3_forward_batch(ctx, tokens.data(), seqs.data(), poss.data(), want.data(), n, nullptr, amax.data()));
        ++steps; rows_total += n;
        if (share_prefix)
            for (int i = 0; i < n; ++i) { std::vector<int32_t>& h = slot[seqs[i]].hist; h.resize((size_t)poss[i]); h.push_back(tokens[i]); }
        if (n_decode && (size_t)n > n_decode) ++mixed_steps;
        for (size_t o = 0; o < out_slot.size(); ++o) {
            Slot& s = slot[out_slot[o]];
            Request& r = reqs[s.req];
            r.generated.push_back(amax[o]);
            if ((int)r.generated.size() >= n_new || stop_set.count(amax[o])) { s.req = -1; ++finished; }
            else s.cur = amax[o];
        }
    }
    const double t1 = now_s();
    for (size_t k = 0; k < reqs.size(); ++k) {
        printf("request %zu:", k);
        for (int32_t v : reqs[k].generated) printf(" %d", v);
        printf("\n");
    }
    fprintf(stderr, "%zu requests on %d slots, %d steps (%d with decode rows and prompt rows together), %ld rows in %.1f ms (%.1f rows/s)\n", reqs.size(), slots, steps,
            mixed_steps, rows_total, (t1 - t0) * 1e3, rows_total / (t1 - t0 + 1e-12));
    if (share_prefix)
        fprintf(stderr, "prefix rows reused: %ld (%ld copied in %d calls, %ld in place)\n", rows_copied + rows_in_place, rows_copied, copy_calls, rows_in_place);
    gl3_destroy(ctx);
    return 0;
}
