// What a handover between two waves of one workgroup costs (the two-wave k_solo
// proposal): wave 0 posts a request in an LDS mailbox and waits for wave 1's reply, as an edit wave
// would hand an op's settle work to a second wave and collect the result. The workgroup is shaped as
// k_solo's: four waves that each claim a whole SIMD's register file (so waves 0 and 1 sit on
// different SIMDs; the SIMD ids are printed), s_setprio 3, waves 2 and 3 parked at the barrier.
// s_memtime on wave 0 around ITERS dependent round trips (each request's data comes from the
// previous reply), for every combination of
//   wait    : spin      poll the ticket back to back
//             sleep1    s_sleep 1 between polls (64 cycles)
//             sleep4    s_sleep 4 between polls (the bounded spin of Engine::take_credit)
//   payload : ticket    the ticket word alone
//             8w        + 8 words each way, one ds_write of lanes 0..7 (an op's seq / msn / flags /
//                       pushes there, heap size / top / status / row mask back)
//             8w+4v     + four 64-lane vectors each way (the level vectors crossing after a block
//                       split or a pack)
// Every wait is bounded (SPIN_MAX polls): a side that times out leaves its loop, the other side then
// times out too, and the run is reported as failed. No barrier inside a loop.
// Last, what the polling costs the OTHER wave: wave 0 runs a dependent ds_read chain (the lone
// wave's LDS round trip) while wave 1 is parked at the barrier, and while wave 1 polls a ticket in
// each of the three ways.
// Build: hipcc --offload-arch=gfx950 -O3 duo_rt.hip -o duo_rt
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

typedef uint32_t u32;
typedef uint64_t u64;

#define SPIN_MAX (1u << 16)
#define N_WAIT 3
#define N_PAY 3
#define N_RT (N_WAIT * N_PAY)
#define N_CHAIN 4
#define N_OUT (N_RT + N_CHAIN + 4)

// mailbox words
enum : u32 { MB_REQ = 0, MB_ACK = 1, MB_REQ8 = 64, MB_ACK8 = 128, MB_REQV = 256, MB_ACKV = 512, MB_WORDS = 1024 };

template <int SLEEP>
__device__ __forceinline__ bool wait_ticket(u32* w, u32 want) {
    for (u32 spin = 0; spin < SPIN_MAX; spin++) {
        const u32 v = __builtin_amdgcn_readfirstlane(__hip_atomic_load(w, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP));
        if (v == want) return true;
        if (SLEEP) __builtin_amdgcn_s_sleep(SLEEP);
    }
    return false;
}
__device__ __forceinline__ void post_ticket(u32* w, u32 v) {
    if (threadIdx.x % 64 == 0) __hip_atomic_store(w, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// one side of ITERS round trips; returns wave 0's cycles (0 on the other side), ~0 on a timeout
template <int SLEEP, int PAY>
__device__ __forceinline__ u64 round_trips(u32* mb, u32 wave, int iters, u32& x) {
    const u32 L = threadIdx.x & 63u;
    u32* mine = wave == 0 ? mb + MB_REQ : mb + MB_ACK;
    u32* theirs = wave == 0 ? mb + MB_ACK : mb + MB_REQ;
    const u32 out8 = wave == 0 ? MB_REQ8 : MB_ACK8, in8 = wave == 0 ? MB_ACK8 : MB_REQ8;
    const u32 outv = wave == 0 ? MB_REQV : MB_ACKV, inv = wave == 0 ? MB_ACKV : MB_REQV;
    bool ok = true;
    const u64 t0 = __builtin_amdgcn_s_memtime();
    for (int i = 1; i <= iters; i++) {
        if (wave == 1) {
            ok = wait_ticket<SLEEP>(theirs, (u32)i);
            if (!ok) break;
            if (PAY >= 1) x += __builtin_amdgcn_readfirstlane(mb[in8 + (L & 7u)]);
            if (PAY >= 2)
                for (u32 v = 0; v < 4; v++) x += __builtin_amdgcn_readlane(mb[inv + 64 * v + L], 63);
        }
        if (PAY >= 1 && L < 8) mb[out8 + L] = x + L;
        if (PAY >= 2)
            for (u32 v = 0; v < 4; v++) mb[outv + 64 * v + L] = x + v + L;
        post_ticket(mine, (u32)i);
        if (wave == 0) {
            ok = wait_ticket<SLEEP>(theirs, (u32)i);
            if (!ok) break;
            if (PAY >= 1) x += __builtin_amdgcn_readfirstlane(mb[in8 + (L & 7u)]);
            if (PAY >= 2)
                for (u32 v = 0; v < 4; v++) x += __builtin_amdgcn_readlane(mb[inv + 64 * v + L], 63);
        }
    }
    const u64 t1 = __builtin_amdgcn_s_memtime();
    return !ok ? ~0ull : wave == 0 ? t1 - t0 : 0ull;
}

// wave 0: a dependent ds_read chain, then the ticket that releases wave 1; wave 1: parked (POLL < 0)
// or polling that ticket
template <int POLL>
__device__ __forceinline__ u64 chain_beside(u32* mb, u32* chain, u32 wave, int iters, u32& x) {
    u64 t = 0;
    if (wave == 0) {
        u32 y = x & 1023u;
        const u64 t0 = __builtin_amdgcn_s_memtime();
        for (int i = 0; i < iters; i++) y = chain[y & 1023u];
        t = __builtin_amdgcn_s_memtime() - t0;
        x += y;
        post_ticket(mb + MB_REQ, 1u);
    } else if constexpr (POLL >= 0) {
        // (the chain takes ~iters * 130 cycles: bounded by the same SPIN_MAX polls, then it gives up)
        if (!wait_ticket<POLL>(mb + MB_REQ, 1u)) x++;
    }
    return t;
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void k(u64* out, int iters, int chain_iters, u32 seed) {
    __shared__ u32 mb[MB_WORDS];
    __shared__ u32 chain[1024];
    asm volatile("" ::: "v255", "a255");  // a whole SIMD's registers per wave: one wave per SIMD
    const u32 wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), L = threadIdx.x & 63u;
    for (u32 i = threadIdx.x; i < 1024; i += 256) {
        chain[i] = (i * 7u + 13u + seed) & 1023u;
        mb[i] = 0;
    }
    __syncthreads();
    __builtin_amdgcn_s_setprio(3);
    const u32 hwid = __builtin_amdgcn_s_getreg(4 | (31 << 11));  // HW_REG_HW_ID: SIMD id in bits 5:4
    u64 t[N_RT + N_CHAIN];
    u32 x = seed;
    int n = 0;
    auto between = [&]() {
        __syncthreads();
        if (threadIdx.x < 2) mb[threadIdx.x] = 0;
        __syncthreads();
    };
#define RT(S, P)                                              \
    t[n] = 0;                                                 \
    if (wave < 2) t[n] = round_trips<S, P>(mb, wave, iters, x); \
    n++;                                                      \
    between();
    RT(0, 0) RT(0, 1) RT(0, 2) RT(1, 0) RT(1, 1) RT(1, 2) RT(4, 0) RT(4, 1) RT(4, 2)
#define CH(P)                                                          \
    t[n] = 0;                                                          \
    if (wave < 2) t[n] = chain_beside<P>(mb, chain, wave, chain_iters, x); \
    n++;                                                               \
    between();
    CH(-1) CH(0) CH(1) CH(4)
    __builtin_amdgcn_s_setprio(0);
    if (wave < 2 && L == 0) {
        u64* o = out + ((u64)blockIdx.x * 2 + wave) * N_OUT;
        for (int i = 0; i < N_RT + N_CHAIN; i++) o[i] = t[i];
        o[N_RT + N_CHAIN] = (hwid >> 4) & 3u;
        o[N_RT + N_CHAIN + 1] = x;
    }
}

int main() {
    const int nb = 8, iters = 2000, chain_iters = 4000;
    const char* waits[N_WAIT] = {"spin", "sleep1", "sleep4"};
    const char* pays[N_PAY] = {"ticket", "8w", "8w+4v"};
    const char* polls[N_CHAIN] = {"parked at the barrier", "polling, spin", "polling, sleep1", "polling, sleep4"};
    u64* d;
    if (hipMalloc(&d, nb * 2 * N_OUT * 8) != hipSuccess) return 1;
    static u64 h[nb * 2 * N_OUT];
    for (int rep = 0; rep < 2; rep++) {  // (the second launch is the one reported)
        hipMemset(d, 0, sizeof h);
        hipLaunchKernelGGL(k, dim3(nb), dim3(256), 0, 0, d, iters, chain_iters, (u32)(rep * 5 + 3));
        if (hipDeviceSynchronize() != hipSuccess) {
            printf("kernel failed\n");
            return 1;
        }
    }
    hipMemcpy(h, d, sizeof h, hipMemcpyDeviceToHost);
    printf("SIMD of wave 0 / wave 1 per workgroup:");
    for (int b = 0; b < nb; b++)
        printf(" %llu/%llu", (unsigned long long)h[(b * 2) * N_OUT + N_RT + N_CHAIN], (unsigned long long)h[(b * 2 + 1) * N_OUT + N_RT + N_CHAIN]);
    printf("\n");
    for (int i = 0; i < N_RT; i++) {
        double s = 0, lo = 1e30, hi = 0;
        int timeouts = 0;
        for (int b = 0; b < nb; b++) {
            const u64 c0 = h[(b * 2) * N_OUT + i], c1 = h[(b * 2 + 1) * N_OUT + i];
            if (c0 == ~0ull || c1 == ~0ull) {
                timeouts++;
                continue;
            }
            const double c = (double)c0 / iters;
            s += c;
            lo = c < lo ? c : lo;
            hi = c > hi ? c : hi;
        }
        if (timeouts == nb) {
            printf("round trip %-6s %-6s all timed out\n", waits[i / N_PAY], pays[i % N_PAY]);
            continue;
        }
        printf("round trip %-6s %-6s %8.1f cycles (min %.1f, max %.1f over %d workgroups, %d timed out)\n", waits[i / N_PAY],
               pays[i % N_PAY], s / (nb - timeouts), lo, hi, nb - timeouts, timeouts);
    }
    for (int i = 0; i < N_CHAIN; i++) {
        double s = 0;
        for (int b = 0; b < nb; b++) s += (double)h[(b * 2) * N_OUT + N_RT + i] / chain_iters;
        printf("wave 0 dependent ds_read, wave 1 %-22s %7.1f cycles per read\n", polls[i], s / nb);
    }
    return 0;
}
