// merlin_levels.hip -- per-level scores of a rollout (merlin_level_scores): prioritized level replay ranks a level by
// how much the value function still errs on it, so the update reduces the [T][N] un-normalised GAE advantages by the
// level each env was in when it acted.
//
// A step adds llrint(f * 2^24), f = min(|a| or max(a, 0), 32768), to sum[level] and 1 to count[level]: 64-bit
// integers, so the result does not depend on the order of the additions and a test can hold the kernel to a
// restatement exactly.  T N <= 2^24 steps of at most 2^39 each stay inside an int64.
//
// The thing to design for is contention: a million steps land on a few hundred addresses.  Three stages of
// pre-reduction, none of them a float atomic:
//   1. a thread owns one env column and walks its steps of a slab in order.  An env changes level only when it
//      resets, so the thread adds a whole run of steps in registers and hands on one (sum, count) per run -- per
//      episode, not per step.  The loads of a row are coalesced across the block's 256 columns.
//   2. L <= LV_LDS_BINS: the run goes to the block's LDS bins (ds 64-bit integer adds); after the slab the block
//      adds its non-empty bins to global memory, one 64-bit vector atomic per bin and block.
//   3. L beyond the LDS budget: the run goes to global memory directly (64-bit vector atomics); with more levels
//      than the LDS holds, the runs of a block rarely meet on an address.
// Grid = (column tiles, step slabs), about one block per CU.
#include <math.h>

#include <algorithm>

#include "merlin_internal.h"

namespace merlin {
namespace {

constexpr int LV_BLK = 256;
constexpr int LV_LDS_BINS = 2048;  // 2048 x (8 + 4) B = 24 KB of LDS per block
constexpr int LV_TARGET_BLOCKS = 256;

typedef unsigned long long u64;

__host__ __device__ __forceinline__ int64_t level_step_score(float a, int kind) {
    const float f = fminf(kind == 0 ? fabsf(a) : fmaxf(a, 0.0f), 32768.0f);  // fminf / fmaxf: a NaN operand loses
    return (int64_t)llrint((double)f * 16777216.0);
}

__global__ __launch_bounds__(LV_BLK) void k_level_zero(int64_t *__restrict__ sum, int64_t *__restrict__ count, int L) {
    const int l = blockIdx.x * LV_BLK + threadIdx.x;
    if (l < L) {
        sum[l] = 0;
        count[l] = 0;
    }
}

template <bool LDS>
__global__ __launch_bounds__(LV_BLK) void k_level_scores(const float *__restrict__ adv, const int32_t *__restrict__ level,
                                                         int T, int N, int rows_per_slab, int L, int kind,
                                                         u64 *__restrict__ sum, u64 *__restrict__ count) {
    __shared__ u64 bsum[LDS ? LV_LDS_BINS : 1];
    __shared__ uint32_t bcnt[LDS ? LV_LDS_BINS : 1];
    if (LDS) {
        for (int l = threadIdx.x; l < L; l += LV_BLK) {
            bsum[l] = 0ull;
            bcnt[l] = 0u;
        }
        __syncthreads();
    }
    const int64_t i = (int64_t)blockIdx.x * LV_BLK + threadIdx.x;
    if (i < (int64_t)N) {
        const int t0 = blockIdx.y * rows_per_slab, t1 = min(T, t0 + rows_per_slab);
        int cur = -1;  // the run's level; -1: none (a skipped step ends a run)
        u64 s = 0ull;
        uint32_t c = 0u;
        auto flush = [&]() {
            if (c) {
                if (LDS) {
                    atomicAdd(&bsum[cur], s);
                    atomicAdd(&bcnt[cur], c);
                } else {
                    atomicAdd(sum + cur, s);
                    atomicAdd(count + cur, (u64)c);
                }
            }
        };
        for (int r = t0; r < t1; r++) {
            const size_t row = (size_t)r * (size_t)N + (size_t)i;
            const int lv = level[row];
            const bool in = lv >= 0 && lv < L;
            const int key = in ? lv : -1;
            if (key != cur) {
                flush();
                cur = key;
                s = 0ull;
                c = 0u;
            }
            if (in) {
                s += (u64)level_step_score(adv[row], kind);
                c += 1u;
            }
        }
        flush();
    }
    if (LDS) {
        __syncthreads();
        for (int l = threadIdx.x; l < L; l += LV_BLK) {
            const uint32_t c = bcnt[l];
            if (c) {
                atomicAdd(sum + l, bsum[l]);
                atomicAdd(count + l, (u64)c);
            }
        }
    }
}

}  // namespace

hipError_t launch_level_scores(const float *adv, const int32_t *level, int T, int N, int L, int kind, int64_t *sum,
                               int64_t *count, int accumulate, hipStream_t s) {
    if (!accumulate) {
        hipLaunchKernelGGL(k_level_zero, dim3((L + LV_BLK - 1) / LV_BLK), dim3(LV_BLK), 0, s, sum, count, L);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (T <= 0 || N <= 0) return hipSuccess;
    const int gx = (N + LV_BLK - 1) / LV_BLK;  // T N <= 2^24: at most 65,536 column tiles
    const int slabs = std::max(1, std::min(T, LV_TARGET_BLOCKS / gx));
    const int rows_per_slab = (T + slabs - 1) / slabs;
    const int gy = (T + rows_per_slab - 1) / rows_per_slab;
    u64 *us = reinterpret_cast<u64 *>(sum), *uc = reinterpret_cast<u64 *>(count);
    if (L <= LV_LDS_BINS)
        hipLaunchKernelGGL(k_level_scores<true>, dim3(gx, gy), dim3(LV_BLK), 0, s, adv, level, T, N, rows_per_slab, L,
                           kind, us, uc);
    else
        hipLaunchKernelGGL(k_level_scores<false>, dim3(gx, gy), dim3(LV_BLK), 0, s, adv, level, T, N, rows_per_slab, L,
                           kind, us, uc);
    return hipGetLastError();
}

void level_scores_host(const float *adv, const int32_t *level, int T, int N, int L, int kind, int64_t *sum,
                       int64_t *count, int accumulate) {
    if (!accumulate)
        for (int l = 0; l < L; l++) sum[l] = count[l] = 0;
    const int64_t n = (int64_t)T * N;
    for (int64_t k = 0; k < n; k++) {
        const int lv = level[k];
        if (lv < 0 || lv >= L) continue;
        sum[lv] += level_step_score(adv[k], kind);
        count[lv] += 1;
    }
}

}  // namespace merlin
