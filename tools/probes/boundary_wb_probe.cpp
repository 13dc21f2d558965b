// What a dependent launch boundary costs behind a producer that leaves its output dirty in L2, and whether a store cache policy moves it.
// A hipGraph of N dependent pairs (producer, then consumer) on one stream; the producer (256 workgroups x 256 threads) writes B bytes of
// bf16 rows (320 channels = 640 B per row) and does nothing else.  Store forms, as the step's kernels emit them:
//   row16  16 B per lane, 1 KiB contiguous per wave instruction (the staged write-out of the fast t2v_gemm epilogue)
//   lpr32  a lane owns 32 B of one row, two 16-B stores; a wave instruction touches 32 rows (linear_pr.hip epilogue)
//   attn8  8 B per lane, 4 lanes cover 32 B of one row, a wave instruction touches 16 rows (attention.hip temporal epilogue)
// each with the default policy, `nt` and `sc1` (write-through).  Consumers: `line` reads one 128-B line per workgroup, `all` reads the B
// bytes with the producer's own workgroup -> chunk map, `all_shift` reads them with the map shifted by one workgroup (another XCD).
// Prints and writes (argv[1]) B,form,policy,consumer,pair_us,producer_us,pair_spread_us: graph time / N, best of 5 replays; the spread is
// worst - best of the same 5.
//   hipcc -O3 --offload-arch=gfx950 tools/probes/boundary_wb_probe.cpp -o tools/probes/boundary_wb_probe
//   tools/probes/boundary_wb_probe profiles/r13_boundary_writeback.csv
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <cstdint>

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); exit(1); } } while (0)
typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));

constexpr int WGS = 256, THREADS = 256, WAVES = THREADS / 64, ROWB = 640;
constexpr int AUX_PLAIN = 0, AUX_NT = 2, AUX_SC1 = 16;   // gfx950 cache-policy bits of the buffer-store builtins
enum { ROW16 = 0, LPR32 = 1, ATTN8 = 2 };
constexpr int unit_bytes(int form) { return form == ROW16 ? 1024 : 2048; }

// every 32-bit word written is `tag`; the buffer descriptor bounds every store to [out, out + bytes)
template <int FORM, int AUX>
__global__ __launch_bounds__(THREADS) void producer(char* out, unsigned bytes, unsigned tag) {
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(out, 0, bytes, 0x00020000);
    const unsigned nunits = bytes / unit_bytes(FORM), chunk = (nunits + WGS - 1) / WGS;
    const unsigned u0 = blockIdx.x * chunk, u1 = min(u0 + chunk, nunits);
    const u32x4_t v4 = {tag, tag, tag, tag};
    const u32x2_t v2 = {tag, tag};
    for (unsigned u = u0 + wave; u < u1; u += WAVES) {
        if (FORM == ROW16) {
            __builtin_amdgcn_raw_buffer_store_b128(v4, rsrc, u * 1024u + lane * 16u, 0, AUX);
        } else if (FORM == LPR32) {   // unit = rows 32 g .. 32 g + 31, bytes 64 blk .. 64 blk + 63 of each
            const unsigned g = u / 10u, blk = u % 10u;
            const unsigned off = (g * 32u + (lane & 31u)) * ROWB + blk * 64u + (lane >> 5) * 32u;
            __builtin_amdgcn_raw_buffer_store_b128(v4, rsrc, off, 0, AUX);
            __builtin_amdgcn_raw_buffer_store_b128(v4, rsrc, off + 16u, 0, AUX);
        } else {                      // unit = rows 16 g .. 16 g + 15, the 128 bytes of head h of each
            const unsigned g = u / 5u, h = u % 5u;
            const unsigned off = (g * 16u + (lane >> 2)) * ROWB + h * 128u + (lane & 3u) * 8u;
#pragma unroll
            for (unsigned m = 0; m < 4; ++m) __builtin_amdgcn_raw_buffer_store_b64(v2, rsrc, off + m * 32u, 0, AUX);
        }
    }
}

__global__ __launch_bounds__(THREADS) void consumer_line(const char* in, unsigned bytes, unsigned* sink) {
    if (bytes == 0 || threadIdx.x >= 8) return;
    const u32x4_t r = *(const u32x4_t*)(in + (size_t)blockIdx.x * (bytes / WGS) + threadIdx.x * 16);
    if ((r.x ^ r.w) == 0x9e3779b9u) sink[0] = 1;
}

__global__ __launch_bounds__(THREADS) void consumer_all(const char* in, unsigned bytes, unsigned shift, unsigned* sink) {
    const unsigned cb = bytes / WGS;   // a multiple of 16 for every B of the table
    const char* p = in + (size_t)((blockIdx.x + shift) % WGS) * cb;
    unsigned acc = 0, i = threadIdx.x * 16;
    for (; i + 3 * THREADS * 16 < cb; i += 4 * THREADS * 16) {
        u32x4_t r[4];
#pragma unroll
        for (int d = 0; d < 4; ++d) r[d] = *(const u32x4_t*)(p + i + d * THREADS * 16);
#pragma unroll
        for (int d = 0; d < 4; ++d) acc += r[d].x ^ r[d].w;
    }
    for (; i < cb; i += THREADS * 16) { const u32x4_t r = *(const u32x4_t*)(p + i); acc += r.y ^ r.z; }
    if (acc == 0x9e3779b9u) sink[0] = 1;
}

typedef void (*producer_fn)(char*, unsigned, unsigned);
static const char* form_name[3] = {"row16", "lpr32", "attn8"};
static const char* policy_name[3] = {"plain", "nt", "sc1"};
static producer_fn producers[3][3] = {
    {producer<ROW16, AUX_PLAIN>, producer<ROW16, AUX_NT>, producer<ROW16, AUX_SC1>},
    {producer<LPR32, AUX_PLAIN>, producer<LPR32, AUX_NT>, producer<LPR32, AUX_SC1>},
    {producer<ATTN8, AUX_PLAIN>, producer<ATTN8, AUX_NT>, producer<ATTN8, AUX_SC1>}};

// consumer: -1 none (producers only), 0 line, 1 all, 2 all_shift
static void time_graph(hipStream_t s, producer_fn prod, int consumer, char* const* bufs, unsigned bytes, unsigned* sink, int n, float* best,
                       float* worst) {
    hipGraph_t g; hipGraphExec_t ge;
    CHECK(hipStreamBeginCapture(s, hipStreamCaptureModeGlobal));
    for (int i = 0; i < n; ++i) {
        char* b = bufs[i & 1];
        hipLaunchKernelGGL(prod, dim3(WGS), dim3(THREADS), 0, s, b, bytes, (unsigned)(i + 1));
        if (consumer == 0) hipLaunchKernelGGL(consumer_line, dim3(WGS), dim3(THREADS), 0, s, (const char*)b, bytes, sink);
        if (consumer >= 1) hipLaunchKernelGGL(consumer_all, dim3(WGS), dim3(THREADS), 0, s, (const char*)b, bytes, consumer == 2 ? 1u : 0u, sink);
    }
    CHECK(hipStreamEndCapture(s, &g));
    CHECK(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
    CHECK(hipGraphLaunch(ge, s)); CHECK(hipStreamSynchronize(s));
    *best = 1e30f; *worst = 0.f;
    for (int r = 0; r < 5; ++r) {
        CHECK(hipEventRecord(e0, s));
        CHECK(hipGraphLaunch(ge, s));
        CHECK(hipEventRecord(e1, s));
        CHECK(hipEventSynchronize(e1));
        float ms; CHECK(hipEventElapsedTime(&ms, e0, e1));
        const float us = ms * 1000.f / n;
        if (us < *best) *best = us;
        if (us > *worst) *worst = us;
    }
    CHECK(hipEventDestroy(e0)); CHECK(hipEventDestroy(e1));
    CHECK(hipGraphExecDestroy(ge)); CHECK(hipGraphDestroy(g));
}

int main(int argc, char** argv) {
    const unsigned sizes[7] = {0u, 1638400u, 6553600u, 13107200u, 26214400u, 52428800u, 104857600u};   // multiples of 32 rows
    const unsigned maxb = sizes[6];
    char* bufs[2]; unsigned* sink;
    CHECK(hipMalloc(&bufs[0], maxb)); CHECK(hipMalloc(&bufs[1], maxb)); CHECK(hipMalloc(&sink, 64));
    hipStream_t s; CHECK(hipStreamCreate(&s));
    // every form and policy writes every word of the range and nothing after it
    {
        const unsigned b = sizes[1], pad = 65536;
        std::vector<uint32_t> h((b + pad) / 4);
        for (int f = 0; f < 3; ++f)
            for (int p = 0; p < 3; ++p) {
                CHECK(hipMemsetAsync(bufs[0], 0xff, b + pad, s));
                hipLaunchKernelGGL(producers[f][p], dim3(WGS), dim3(THREADS), 0, s, bufs[0], b, 0x3f803f80u);
                CHECK(hipMemcpyAsync(h.data(), bufs[0], b + pad, hipMemcpyDeviceToHost, s));
                CHECK(hipStreamSynchronize(s));
                for (size_t i = 0; i < h.size(); ++i)
                    if (h[i] != (i < b / 4 ? 0x3f803f80u : 0xffffffffu)) { fprintf(stderr, "coverage %s %s word %zu = %08x\n", form_name[f], policy_name[p], i, h[i]); return 1; }
            }
    }
    FILE* csv = argc > 1 ? fopen(argv[1], "w") : nullptr;
    if (argc > 1 && !csv) { fprintf(stderr, "cannot write %s\n", argv[1]); return 1; }
    const char* header = "B,form,policy,consumer,pair_us,producer_us,pair_spread_us\n";
    printf("%s", header); if (csv) fprintf(csv, "%s", header);
    static const char* consumer_name[3] = {"line", "all", "all_shift"};
    const int n = 16;
    for (unsigned b : sizes)
        for (int f = 0; f < 3; ++f)
            for (int p = 0; p < 3; ++p) {
                float prod_best, prod_worst;
                time_graph(s, producers[f][p], -1, bufs, b, sink, n, &prod_best, &prod_worst);
                for (int c = 0; c < 3; ++c) {
                    float best, worst;
                    time_graph(s, producers[f][p], c, bufs, b, sink, n, &best, &worst);
                    char line[256];
                    snprintf(line, sizeof line, "%u,%s,%s,%s,%.2f,%.2f,%.2f\n", b, form_name[f], policy_name[p], consumer_name[c], best, prod_best, worst - best);
                    printf("%s", line); if (csv) fprintf(csv, "%s", line);
                }
                fflush(stdout);
            }
    if (csv) fclose(csv);
    return 0;
}
