// Price of a polled tagged hand-over by the number of poll rounds in flight (development tool, not part of the library):
// how long after a producer's (value, tag) store does a resident consumer see it, when the consumer polls serially (one round
// of agent-scope loads, wait, s_sleep 1, the next) or keeps K = 2, 4, 8 rounds in flight a fraction of a round trip apart,
// consumed oldest first (the question of profiles/NOTEBOOK.md §20)?
//
//   make -C tools/microbench ../bin/poll_stagger && tools/bin/poll_stagger [trials]
//
// One launch per trial, two one-wave workgroups: block 0 waits a pseudo-random delay (so that the store meets every phase of the
// consumer's rounds), stores WORDS tagged words per lane and stamps the clock; block 1 (dispatched behind block 0, so it never
// holds a slot block 0 needs) polls them and stamps it when every tag matches.  Reported: the median and the mean of
// detect - store in s_memrealtime ticks (the constant 100 MHz clock both workgroups share: 10 ns; s_memtime is per XCD) and the
// rounds consumed.  Every wait is bounded: the producer's delay by its tick count and an iteration limit, the consumer by a spin limit — a consumer that runs out reports a time-out and the trial is
// dropped; nothing here can wait without a bound.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); exit(1); } } while (0)

typedef unsigned long long u64;
constexpr int WORDS = 4;            // 8-byte loads per lane and round, as the attention role's q words
constexpr unsigned kSpinLimit = 1u << 16;

struct Out {
    u64 t_store, t_detect;
    unsigned rounds, timed_out;
};

__device__ __forceinline__ void round_load(u64 (&w)[WORDS], const u64* p) {
#pragma unroll
    for (int j = 0; j < WORDS; ++j) w[j] = __hip_atomic_load(p + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ bool round_ok(const u64 (&w)[WORDS], unsigned tag) {
    bool ok = true;
#pragma unroll
    for (int j = 0; j < WORDS; ++j) ok = ok && (unsigned)(w[j] >> 32) == tag;
    return __builtin_amdgcn_ballot_w64(!ok) == 0;
}

// K rounds in flight, first issues GAP x 64 clocks apart; K == 1: the serial poll of the library
template <int K, int GAP>
__global__ __launch_bounds__(64) void trial_kernel(u64* words, Out* out, unsigned tag, unsigned delay_ticks) {
    const int lane = threadIdx.x;
    if (blockIdx.x == 0) {  // producer
        const u64 t0 = __builtin_amdgcn_s_memrealtime();
        for (int i = 0; i < (1 << 20) && __builtin_amdgcn_s_memrealtime() - t0 < delay_ticks; ++i) __builtin_amdgcn_s_sleep(1);
#pragma unroll
        for (int j = 0; j < WORDS; ++j)
            __hip_atomic_store(words + lane * WORDS + j, ((u64)tag << 32) | (unsigned)(lane + j), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (lane == 0) out->t_store = __builtin_amdgcn_s_memrealtime();
        return;
    }
    const u64* p = words + lane * WORDS;
    u64 r[K][WORDS];
#pragma unroll
    for (int s = 0; s < K; ++s) {
        round_load(r[s], p);
        if (s + 1 < K) __builtin_amdgcn_s_sleep(GAP);
    }
    unsigned spins = 0, timed_out = 0;
    for (bool done = false; !done;) {
#pragma unroll
        for (int s = 0; s < K; ++s) {  // slot s holds the oldest round in flight
            const bool ok = round_ok(r[s], tag);
            if (ok || spins >= kSpinLimit) {
                timed_out = !ok;
                done = true;
                break;
            }
            ++spins;
            round_load(r[s], p);
            __builtin_amdgcn_s_sleep(1);
        }
    }
    const u64 t1 = __builtin_amdgcn_s_memrealtime();
    if (lane == 0) {
        out->t_detect = t1;
        out->rounds = spins + 1;
        out->timed_out = timed_out;
    }
}

template <int K, int GAP>
static void run(const char* name, int trials, u64* d_words, Out* d_out, unsigned& tag) {
    std::vector<double> dt;
    double rounds = 0;
    int dropped = 0, timeouts = 0;
    for (int t = 0; t < trials; ++t) {
        ++tag;
        const unsigned delay = 300u + (unsigned)((t * 37) % 241);  // 3.0 .. 5.4 us: well behind the consumer's first rounds, every phase
        hipLaunchKernelGGL((trial_kernel<K, GAP>), dim3(2), dim3(64), 0, 0, d_words, d_out, tag, delay);
        CK(hipDeviceSynchronize());
        Out o;
        CK(hipMemcpy(&o, d_out, sizeof(o), hipMemcpyDeviceToHost));
        if (o.timed_out || o.t_detect < o.t_store) {
            ++dropped;
            timeouts += o.timed_out != 0;
            continue;
        }
        dt.push_back((double)(o.t_detect - o.t_store));
        rounds += o.rounds;
    }
    if (dt.empty()) {
        printf("%-22s no valid trial (%d dropped, %d of them timed out)\n", name, dropped, timeouts);
        return;
    }
    std::sort(dt.begin(), dt.end());
    double mean = 0;
    for (double v : dt) mean += v;
    mean /= dt.size();
    printf("%-22s trials %4zu dropped %d  store->detect ticks: median %.0f mean %.1f p10 %.0f p90 %.0f  rounds mean %.1f\n", name, dt.size(), dropped,
           dt[dt.size() / 2], mean, dt[dt.size() / 10], dt[dt.size() * 9 / 10], rounds / dt.size());
}

int main(int argc, char** argv) {
    const int trials = argc > 1 ? atoi(argv[1]) : 400;
    u64* d_words;
    Out* d_out;
    CK(hipMalloc(&d_words, 64 * WORDS * sizeof(u64)));
    CK(hipMemset(d_words, 0, 64 * WORDS * sizeof(u64)));
    CK(hipMalloc(&d_out, sizeof(Out)));
    unsigned tag = 0;
    for (int rep = 0; rep < 2; ++rep) {  // (the first repetition also warms the code objects up)
        run<1, 1>("serial (1 in flight)", trials, d_words, d_out, tag);
        run<2, 22>("2 in flight, gap 22", trials, d_words, d_out, tag);
        run<4, 11>("4 in flight, gap 11", trials, d_words, d_out, tag);
        run<8, 5>("8 in flight, gap 5", trials, d_words, d_out, tag);
    }
    CK(hipFree(d_words));
    CK(hipFree(d_out));
    return 0;
}
