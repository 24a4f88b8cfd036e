// tools/lds_residency.hip -- how many workgroups of a given LDS size one CU of gfx950 (MI355X) holds at once, measured: the
// LDS allocation granule the library's accounting (PTRS_LDS_GRANULE, lds_alloc in ptrs_hip.hip) rests on.
//
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -o /tmp/lds_residency tools/lds_residency.hip && timeout -k 10 120 /tmp/lds_residency > profiles/lds_residency.json
//
// A workgroup of 256 threads (one wave per SIMD, a handful of registers: nothing but LDS limits how many a CU holds, up to the
// 8 the wave slots allow) touches a B-byte dynamic LDS array and runs a fixed-length dependent chain: 4 v_fma_f32 and an
// s_sleep per step, so that a wave issues for a small part of its time and seven waves on a SIMD take as long as one.  It waits
// for nothing and for nobody.  A launch of k x CUs workgroups then takes one chain length while k workgroups per CU are
// resident, and two once k exceeds what fits.  Timed with events, median of 20 launches, for k = 4..7 and B around the sizes
// the LDS-form traversal kernels have had (26 624 = 8-entry column + 640 vectors, 27 136 = 9 + 544, 26 880 = 9 + 528).
// Reported: the times, the residency inferred per B, and the allocation granules (multiples of 128 B) that explain all of them
// under residency = floor(163 840 / roundup(B, granule)).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); std::exit(1); } } while (0)

__global__ __launch_bounds__(256) void k_chain(float *out, int steps, unsigned lds_bytes) {
    extern __shared__ float lds[];
    const unsigned n = lds_bytes / 4u; // whole dwords of the array; the last one is touched by lane 0 below
    for (unsigned i = threadIdx.x; i < n; i += 256u) lds[i] = (float)i;
    __syncthreads();
    float a = 1.0f + (float)threadIdx.x * 1e-3f + lds[(threadIdx.x * 61u) % n];
    const float b = 0.9999f, c = 1e-7f;
    for (int i = 0; i < steps; ++i) {
        asm volatile("v_fma_f32 %0, %0, %1, %2\n\tv_fma_f32 %0, %0, %1, %2\n\tv_fma_f32 %0, %0, %1, %2\n\tv_fma_f32 %0, %0, %1, %2\n\ts_sleep 2" : "+v"(a) : "v"(b), "v"(c));
    }
    if (threadIdx.x == 0) a += lds[n - 1u];
    out[blockIdx.x * 256u + threadIdx.x] = a;
}

static double median_ms(int blocks, unsigned bytes, int steps, float *out, hipEvent_t e0, hipEvent_t e1) {
    std::vector<float> t;
    hipLaunchKernelGGL(k_chain, dim3(blocks), dim3(256), bytes, 0, out, 50, bytes); // warm-up (clocks, code)
    CHECK(hipDeviceSynchronize());
    for (int r = 0; r < 20; ++r) {
        CHECK(hipEventRecord(e0, 0));
        hipLaunchKernelGGL(k_chain, dim3(blocks), dim3(256), bytes, 0, out, steps, bytes);
        CHECK(hipEventRecord(e1, 0));
        CHECK(hipDeviceSynchronize());
        float ms = 0.0f; CHECK(hipEventElapsedTime(&ms, e0, e1));
        t.push_back(ms);
    }
    std::sort(t.begin(), t.end());
    return 0.5 * ((double)t[9] + (double)t[10]);
}

int main(int argc, char **argv) {
    const int steps = argc > 1 ? std::atoi(argv[1]) : 3000;
    const unsigned lds_per_cu = 163840u;
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, 0));
    const int cus = prop.multiProcessorCount;
    float *out;
    CHECK(hipMalloc(&out, (size_t)cus * 8 * 256 * 4));
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
    const unsigned sizes[] = {26624u, 26880u, 26881u, 27136u, 28160u};
    const int n_sizes = (int)(sizeof(sizes) / sizeof(sizes[0])), k0 = 4, k1 = 7;
    const double chain_ms = median_ms(cus, 1024u, steps, out, e0, e1); // one small workgroup per CU: the chain by itself
    std::printf("{\"device\": \"%s\", \"arch\": \"%s\", \"cus\": %d, \"lds_per_cu\": %u, \"steps\": %d, \"chain_ms\": %.4f,\n \"what\": \"median of 20 launches of k x CUs workgroups of 256 threads with B bytes of dynamic LDS, each one fixed-length chain; resident = largest k whose launch takes less than 1.5 chains\",\n \"rows\": [\n",
                prop.name, prop.gcnArchName, cus, lds_per_cu, steps, chain_ms);
    int resident[8];
    for (int s = 0; s < n_sizes; ++s) {
        int occ_api = 0;
        CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ_api, k_chain, 256, sizes[s]));
        resident[s] = k0 - 1; // "fewer than k0" if even the first launch takes two chains
        bool open = true;
        std::printf("  {\"lds_bytes\": %u, \"occupancy_api\": %d, \"ms_by_k\": {", sizes[s], occ_api);
        for (int k = k0; k <= k1; ++k) {
            const double ms = median_ms(cus * k, sizes[s], steps, out, e0, e1);
            if (open && ms < 1.5 * chain_ms) resident[s] = k; else open = false;
            std::printf("%s\"%d\": %.4f", k == k0 ? "" : ", ", k, ms);
        }
        std::printf("}, \"resident_wgs_per_cu\": %d, \"resident_is_lower_bound\": %s}%s\n", resident[s], resident[s] == k1 ? "true" : "false", s + 1 < n_sizes ? "," : "");
    }
    std::printf(" ],\n \"granules_consistent\": [");
    int first_fit = 0, n_fit = 0; bool has_1280 = false;
    for (unsigned g = 128u; g <= 8192u; g += 128u) {
        bool ok = true;
        for (int s = 0; s < n_sizes && ok; ++s) {
            const unsigned fit = lds_per_cu / ((sizes[s] + g - 1u) / g * g);
            ok = resident[s] == k1 ? fit >= (unsigned)k1 : (resident[s] < k0 ? fit < (unsigned)k0 : fit == (unsigned)resident[s]);
        }
        if (ok) { std::printf("%s%u", n_fit ? ", " : "", g); if (!n_fit) first_fit = (int)g; ++n_fit; has_1280 = has_1280 || g == 1280u; }
    }
    // 1 280 B (320 dwords) is what LLVM's AMDGPU target description states for parts with 160 KB of LDS: named where the measurement allows it.
    std::printf("],\n \"granule\": %d\n}\n", has_1280 ? 1280 : first_fit);
    return 0;
}
