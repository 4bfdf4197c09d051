// The yardstick of k_bgzf_crc (profiles/bgzf_crc.md): a pass that only READS the same amount of text -- 16-byte loads, an XOR, one
// store per workgroup.  hipcc --offload-arch=gfx950 -O3 -o profiles/microbench/read_only profiles/microbench/read_only.hip
//     read_only [MB of text, default 3133]
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
__global__ __launch_bounds__(256) void k_read(const uint4* __restrict__ p, size_t n16, unsigned* __restrict__ out) {
    unsigned v = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (size_t)gridDim.x * 256) { const uint4 w = p[i]; v ^= w.x ^ w.y ^ w.z ^ w.w; }
    for (int d = 32; d >= 1; d >>= 1) v ^= (unsigned)__shfl_xor((int)v, d, 64);
    if ((threadIdx.x & 63) == 0) atomicXor(&out[blockIdx.x & 1023], v);
}
int main(int argc, char** argv) {
    const size_t mb = argc > 1 ? (size_t)atoll(argv[1]) : 3133, n = mb * 1000000 / 16 * 16;
    uint4* d = nullptr; unsigned* o = nullptr;
    if (hipMalloc((void**)&d, n) != hipSuccess || hipMalloc((void**)&o, 4096) != hipSuccess) { fprintf(stderr, "allocation failed\n"); return 1; }
    hipMemset(d, 0x41, n); hipMemset(o, 0, 4096);
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    float best = 1e30f;
    for (int r = 0; r < 6; r++) {
        hipEventRecord(e0, 0);
        hipLaunchKernelGGL(k_read, dim3(256 * 8), dim3(256), 0, 0, d, n / 16, o);
        hipEventRecord(e1, 0);
        if (hipEventSynchronize(e1) != hipSuccess) { fprintf(stderr, "kernel failed\n"); return 1; }
        float ms = 0; hipEventElapsedTime(&ms, e0, e1);
        if (r && ms < best) best = ms;
    }
    printf("read only: %.1f MB in %.3f ms = %.1f GB/s\n", n / 1e6, best, n / best / 1e6);
    hipFree(d); hipFree(o);
    return 0;
}
