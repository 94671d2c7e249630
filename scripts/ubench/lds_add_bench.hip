// ubench: what does one wave-instruction of ds_add_f64 (no return) cost, by the addresses its 64 lanes carry? The forward sweeps'
// source walk (k_xfwd, hank_xsweep.h) adds every source's two lottery parts into the LDS tile with it, and the instruction is not in
// the LDS tables we have. One workgroup of 768 threads per CU, LDS only, nothing between workgroups; W of the 12 waves issue
// (1, 3, 11), each into a 4 KiB region of its own, R x 16 adds in straight-line code (the instruction's offset field walks four
// images 256 B apart: the banks stay what the pattern says). Lane l adds to double index idx(l) of its wave's region:
//   a    l * 6                       consecutive rows of the [lane][SL = 6] tile (48-byte stride): today's common case
//   b    l                           the same rows in a slot-major plane (8-byte stride)
//   c m  (l / m) * S                 runs of m consecutive lanes on ONE address: today's flat unit (S = 6), and in a plane (S = 1)
//   d m  ((4 (l % 16) + l / 16) / m) * S   the same 64 sources dealt four apart inside each 16-lane group (lane g*16 + j takes source 4j + g)
//   g G  l % G + (l / G) * 32        lanes l and l + G on one bank at different addresses: which G conflicts tells the lane-group size
// Time: HIP events around the launch (ns per wave-instruction and wave = launch time / (R * 16)) and s_memtime around the loop
// (the slowest issuing wave of the chip). The tile's sum is checked against the number of adds. Run it under a time limit:
//   hipcc --offload-arch=gfx950 -O3 -o lds_add_bench lds_add_bench.hip && timeout -k 10 120 ./lds_add_bench
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>
constexpr int NT = 768, NW = NT / 64, REG = 512, U = 16;      // threads, waves, doubles per wave region, adds per trip
__device__ __forceinline__ void add(double *p) { __hip_atomic_fetch_add(p, 1.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __host__ inline int lane_idx(int pat, int m, int S, int l) {
    switch (pat) {
    case 0: return l * 6;
    case 1: return l;
    case 2: return (l / m) * S;
    case 3: return ((4 * (l % 16) + l / 16) / m) * S;
    default: return l % m + (l / m) * 32;
    }
}
__global__ void __launch_bounds__(NT) k(int pat, int m, int S, int W, int R, unsigned long long *ticks, double *sums) {
    __shared__ double tile[NW * REG];
    for (int i = threadIdx.x; i < NW * REG; i += NT) tile[i] = 0.0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (wv < W) {
        double *p = tile + wv * REG + lane_idx(pat, m, S, lane);
        const unsigned long long t0 = __builtin_readcyclecounter();
        for (int r = 0; r < R; r++) {
#pragma unroll
            for (int u = 0; u < U; u++) add(p + (u & 3) * 32);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        const unsigned long long t1 = __builtin_readcyclecounter();
        if (lane == 0) ticks[blockIdx.x * NW + wv] = t1 - t0;
    }
    __syncthreads();
    double s = 0.0;
    for (int i = threadIdx.x; i < NW * REG; i += NT) s += tile[i];
    __shared__ double red[NT];
    red[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) { double a = 0.0; for (int i = 0; i < NT; i++) a += red[i]; sums[blockIdx.x] = a; }
}
int main() {
    int ncu = 256; hipDeviceProp_t pr;
    if (hipGetDeviceProperties(&pr, 0) != hipSuccess) { printf("no device\n"); return 1; }
    ncu = pr.multiProcessorCount;
    unsigned long long *ticks; double *sums; const int R = 4096;
    hipMalloc(&ticks, sizeof(unsigned long long) * ncu * NW); hipMalloc(&sums, sizeof(double) * ncu);
    std::vector<unsigned long long> ht(ncu * NW); std::vector<double> hsum(ncu);
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    struct Case { const char *name; int pat, m, S; };
    const Case cases[] = {
        {"a  rows, 48-byte stride        ", 0, 1, 6}, {"b  rows, 8-byte stride         ", 1, 1, 1},
        {"c2 runs of 2, 48-byte stride   ", 2, 2, 6}, {"d2 dealt 4 apart, 48-byte     ", 3, 2, 6},
        {"c3 runs of 3, 48-byte stride   ", 2, 3, 6}, {"d3 dealt 4 apart, 48-byte     ", 3, 3, 6},
        {"c4 runs of 4, 48-byte stride   ", 2, 4, 6}, {"d4 dealt 4 apart, 48-byte     ", 3, 4, 6},
        {"c2 runs of 2, 8-byte stride    ", 2, 2, 1}, {"d2 dealt 4 apart, 8-byte      ", 3, 2, 1},
        {"c3 runs of 3, 8-byte stride    ", 2, 3, 1}, {"d3 dealt 4 apart, 8-byte      ", 3, 3, 1},
        {"c4 runs of 4, 8-byte stride    ", 2, 4, 1}, {"d4 dealt 4 apart, 8-byte      ", 3, 4, 1},
        {"c64 all lanes on one address   ", 2, 64, 1},
        {"g8  lanes l, l+8 on one bank   ", 4, 8, 1}, {"g16 lanes l, l+16 on one bank  ", 4, 16, 1}, {"g32 lanes l, l+32 on one bank  ", 4, 32, 1},
    };
    printf("%d CUs, clockRate %d kHz; %d threads per workgroup, %d x %d adds per issuing wave\n", ncu, pr.clockRate, NT, R, U);
    printf("pattern                          waves   ns/instr/wave  ticks/instr/wave  ticks/instr/CU   sum\n");
    for (const Case &c : cases) for (int W : {1, 3, 11}) {
        hipLaunchKernelGGL(k, dim3(ncu), dim3(NT), 0, 0, c.pat, c.m, c.S, W, 64, ticks, sums);      // warm-up
        hipDeviceSynchronize();
        hipEventRecord(e0, 0);
        hipLaunchKernelGGL(k, dim3(ncu), dim3(NT), 0, 0, c.pat, c.m, c.S, W, R, ticks, sums);
        hipEventRecord(e1, 0);
        if (hipDeviceSynchronize() != hipSuccess) { printf("launch failed\n"); return 1; }
        float ms = 0; hipEventElapsedTime(&ms, e0, e1);
        hipMemcpy(ht.data(), ticks, sizeof(unsigned long long) * ncu * NW, hipMemcpyDeviceToHost);
        hipMemcpy(hsum.data(), sums, sizeof(double) * ncu, hipMemcpyDeviceToHost);
        unsigned long long mx = 0; for (int b = 0; b < ncu; b++) for (int w = 0; w < W; w++) mx = ht[b * NW + w] > mx ? ht[b * NW + w] : mx;
        bool ok = true; for (int b = 0; b < ncu; b++) ok = ok && hsum[b] == (double)W * R * U * 64;
        const double n = (double)R * U;
        printf("%s  %2d      %8.2f       %8.2f         %8.2f      %s\n", c.name, W, 1e6 * ms / n, mx / n, mx / n / W, ok ? "ok" : "WRONG");
    }
    return 0;
}
