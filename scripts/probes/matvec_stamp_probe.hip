// Per-workgroup stamps of matvec_q8t_kernel at the decode shapes: how long after the chip's last weight product the chip's last result
// is stored (the serial tail of the ordered block sum), and what one workgroup barrier round costs.  Random bytes as weights, launch
// geometry as launch_matvec (gl3_api.hip) picks it.  One JSON line per class; scripts/matvec_chain_tail.py turns them into a table.
// hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -I../../gpullama3.java_amd/csrc matvec_stamp_probe.hip -o matvec_stamp_probe
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
#define GL3_MV_TIMING 1
#include "gl3_decode_kernels.h"
using namespace gl3;

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %s:%d\n", hipGetErrorString(e), __FILE__, __LINE__); exit(1); } } while (0)

struct Shape { const char* name; int pro, epi, rows, k; };

static double median(std::vector<double> v) { std::sort(v.begin(), v.end()); return v.empty() ? 0.0 : v[v.size() / 2]; }

template <int PRO, int EPI, int NPW>
static void run(const Shape& sh, const MatvecArgs& a, int wgs, size_t smem, std::vector<uint8_t*>& wb, std::vector<uint8_t*>& w2b, const char* tag) {
    // as launch_matvec: the segmented chain for strips of more than one segment
    auto kern = a.ng > mv_seg_groups(NPW, EPI) ? matvec_q8t_kernel<PRO, EPI, NPW, false, false, true> : matvec_q8t_kernel<PRO, EPI, NPW>;
    CK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 256));
    MatvecArgs b = a;
    const int reps = 24;
    std::vector<double> chip_tail, wg_tail, chain, span, last_begin;
    std::vector<unsigned long long> st((size_t)MV_WG_STAMPS * 8);
    void* sym; CK(hipGetSymbolAddress(&sym, HIP_SYMBOL(gl3::gl3_mv_wg_stamp)));
    for (int i = 0; i < 4 + reps; ++i) {
        b.w = wb[i % wb.size()]; b.w2 = w2b.empty() ? nullptr : w2b[i % w2b.size()];
        CK(hipMemset(sym, 0, st.size() * 8));
        CK(hipDeviceSynchronize());
        hipLaunchKernelGGL(kern, dim3(wgs), dim3(mv_threads(NPW)), smem, 0, b);
        CK(hipDeviceSynchronize());
        if (i < 4) continue;
        CK(hipMemcpy(st.data(), sym, st.size() * 8, hipMemcpyDeviceToHost));
        const int n = std::min(wgs, MV_WG_STAMPS);
        unsigned long long t0 = ~0ull, p = 0, s = 0, cb = 0;
        std::vector<double> tails, chains;
        for (int w = 0; w < n; ++w) {
            const unsigned long long* q = &st[(size_t)w * 8];
            t0 = std::min(t0, q[0]); p = std::max(p, q[1]); s = std::max(s, q[4]); cb = std::max(cb, q[2]);
            tails.push_back(10.0 * (double)(long long)(q[4] - q[1]));        // 100 MHz ticks -> ns
            chains.push_back(10.0 * (double)(long long)(q[3] - q[2]));
        }
        chip_tail.push_back(10.0 * (double)(long long)(s - p));
        last_begin.push_back(10.0 * (double)(long long)(s - cb));
        span.push_back(10.0 * (double)(long long)(s - t0));
        wg_tail.push_back(median(tails));
        chain.push_back(median(chains));
    }
    std::sort(chip_tail.begin(), chip_tail.end());
    printf("{\"build\": \"%s\", \"class\": \"%s\", \"segmented\": %d, \"rows\": %d, \"k\": %d, \"ng\": %d, \"wgs\": %d, \"npw\": %d, \"reps\": %d, "
           "\"chip_tail_ns_median\": %.0f, \"chip_tail_ns_min\": %.0f, \"chip_tail_ns_max\": %.0f, \"wg_tail_ns_median\": %.0f, "
           "\"last_chain_ns_median\": %.0f, \"chip_last_chain_begin_to_store_ns_median\": %.0f, \"span_ns_median\": %.0f}\n",
           tag, sh.name, (int)(a.ng > mv_seg_groups(NPW, EPI)), sh.rows, sh.k, a.ng, wgs, NPW, reps, median(chip_tail), chip_tail.front(), chip_tail.back(), median(wg_tail),
           median(chain), median(last_begin), median(span));
    fflush(stdout);
}

// one workgroup barrier round (s_waitcnt lgkmcnt(0); s_barrier) with one LDS write per wavefront in front of it, as the producers have
template <int WAVES>
__global__ __launch_bounds__(64 * WAVES) void barrier_round_kernel(int rounds, unsigned long long* out) {
    __shared__ float buf[64 * WAVES];
    const unsigned long long t0 = wall_clock64();
    for (int r = 0; r < rounds; ++r) {
        buf[threadIdx.x] = (float)r;
        lds_barrier();
    }
    const unsigned long long t1 = wall_clock64();
    if (threadIdx.x == 0) out[blockIdx.x] = t1 - t0 + (unsigned long long)(buf[1] == -1.f);
}

template <int WAVES>
static void barrier_cost(int wgs, const char* tag) {
    unsigned long long* d; CK(hipMalloc(&d, wgs * 8));
    const int rounds = 4096;
    std::vector<unsigned long long> h(wgs);
    for (int i = 0; i < 3; ++i) hipLaunchKernelGGL(barrier_round_kernel<WAVES>, dim3(wgs), dim3(64 * WAVES), 0, 0, rounds, d);
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(h.data(), d, wgs * 8, hipMemcpyDeviceToHost));
    std::vector<double> v; for (auto x : h) v.push_back(10.0 * (double)x / rounds);
    std::sort(v.begin(), v.end());
    printf("{\"build\": \"%s\", \"class\": \"barrier_round\", \"waves\": %d, \"wgs\": %d, \"ns_per_round_median\": %.1f, \"ns_per_round_max\": %.1f}\n", tag, WAVES, wgs, median(v), v.back());
    CK(hipFree(d));
}

int main(int argc, char** argv) {
    const char* tag = argc > 1 ? argv[1] : "build";
    const Shape shapes[] = {
        {"qkv 8B", PRO_RMS, EPI_STORE, 6144, 4096}, {"wo 8B", PRO_QUANT, EPI_RESID, 4096, 4096},
        {"gate/up 8B", PRO_RMS, EPI_SWIGLU, 14336, 4096}, {"down 8B", PRO_QUANT, EPI_RESID, 4096, 14336},
        {"logits 8B", PRO_RMS, EPI_STORE, 128256, 4096},
        {"down 1B", PRO_QUANT, EPI_RESID, 2048, 8192}, {"down qwen3-4b", PRO_QUANT, EPI_RESID, 2560, 9728},
    };
    float *x, *nw, *out;
    CK(hipMalloc(&x, 16384 * 4)); CK(hipMalloc(&nw, 16384 * 4)); CK(hipMalloc(&out, 131072 * 4));
    std::vector<float> hx(16384);
    for (auto& v : hx) v = (rand() / (float)RAND_MAX - 0.5f);
    CK(hipMemcpy(x, hx.data(), 16384 * 4, hipMemcpyHostToDevice));
    for (auto& v : hx) v = 1.0f + 0.02f * (rand() / (float)RAND_MAX - 0.5f);
    CK(hipMemcpy(nw, hx.data(), 16384 * 4, hipMemcpyHostToDevice));
    CK(hipMemset(out, 0, 131072 * 4));
    for (const Shape& sh : shapes) {
        MatvecArgs a{};
        a.rows = sh.rows; a.k = sh.k; a.ng = (sh.k / 32 + 3) / 4; a.nstrips = (sh.rows + 15) / 16;
        a.x = x; a.norm_w = nw; a.eps = 1e-5f; a.out = out; a.resid_in = sh.epi == EPI_RESID ? out : nullptr; a.out_scale = 1.0f;
        const size_t bytes = (size_t)a.nstrips * a.ng * TILE_BYTES;
        const int nm = sh.epi == EPI_SWIGLU ? 2 : 1;
        const int nbuf = (int)std::max<size_t>(2, (600ull << 20) / (bytes * nm) + 1);      // distinct buffers: nothing stays in the Infinity Cache
        std::vector<uint8_t*> wb, w2b;
        for (int i = 0; i < nbuf; ++i) { uint8_t* p; CK(hipMalloc(&p, bytes)); CK(hipMemset(p, 0x11 + i, bytes)); wb.push_back(p);
            if (nm == 2) { CK(hipMalloc(&p, bytes)); CK(hipMemset(p, 0x23 + i, bytes)); w2b.push_back(p); } }
        const size_t smem = (size_t)a.ng * 4 * 32 + (size_t)a.ng * 4 * 4 + (sh.pro == PRO_RMS ? (size_t)(a.k + 32) * 4 : 0) + (size_t)2 * nm * a.ng * 64 * 4 + 128;
        const int wgs = std::min(a.nstrips, 512);
        if (sh.pro == PRO_RMS && sh.epi == EPI_STORE) run<PRO_RMS, EPI_STORE, 4>(sh, a, wgs, smem, wb, w2b, tag);
        else if (sh.pro == PRO_RMS) run<PRO_RMS, EPI_SWIGLU, 4>(sh, a, wgs, smem, wb, w2b, tag);
        else if (a.nstrips <= 256) run<PRO_QUANT, EPI_RESID, 8>(sh, a, wgs, smem, wb, w2b, tag);
        else run<PRO_QUANT, EPI_RESID, 4>(sh, a, wgs, smem, wb, w2b, tag);
        for (auto p : wb) CK(hipFree(p));
        for (auto p : w2b) CK(hipFree(p));
    }
    barrier_cost<5>(512, tag);        // 4 producers + chain, two workgroups per CU
    barrier_cost<9>(256, tag);        // 8 producers + chain
    return 0;
}
