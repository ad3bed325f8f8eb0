// merlin_epstats.hip -- finished episodes of a rollout summed by env class (merlin_episode_class_stats): the
// per-difficulty return curves of a run on a mixed-task vector env, without pulling [T][N] masks to the host.
//
// The rollout's rows are [T][N] (row t*N + i = env i at step t) and a class belongs to an env, so a thread owns one
// env column: its class is fixed, its loads are coalesced across the block's 256 columns, and it adds its own rows in
// step order.  Grid = (column tiles, step slabs).
//   k_eps_partial  per block: every thread's (episodes, sum return, sum return^2, sum length) over its rows of the
//                  slab, then per class c a wave64 shuffle-down reduction (lanes of other classes add 0),
//                  the 4 waves' results added in wave order, written to partial[block][c][4].
//   k_eps_fold     one block: per entry (c, k), 8 groups of threads add the blocks' partials (group j blocks j, j + 8,
//                  ... in order), the 8 group sums are added in group order and written (or, accumulate, added) to
//                  out[c][k].
// fp64 throughout, no atomics: the order of every addition is fixed by the launch shape, which depends only on
// (T, N), so two calls on the same input give the same bits.  A 4096 x 256 rollout is a 4-MB read of `done` plus the
// finished rows' return / length: memory time is a few microseconds, the two launches dominate.
#include <algorithm>

#include "merlin_internal.h"

namespace merlin {
namespace {

constexpr int EPS_BLK = 256;
constexpr int EPS_TARGET_BLOCKS = 256;
static_assert(EPS_TARGET_BLOCKS <= EPS_MAX_BLOCKS, "the workspace holds EPS_MAX_BLOCKS partials");

__global__ __launch_bounds__(EPS_BLK) void k_eps_partial(const float *__restrict__ done, const double *__restrict__ ep_ret,
                                                        const int32_t *__restrict__ ep_len,
                                                        const uint8_t *__restrict__ cls, int T, int N, int col0,
                                                        int rows_per_slab, int n_classes,
                                                        double *__restrict__ partial) {
    __shared__ double red[EPS_BLK / 64][EPS_MAX_CLASSES][4];
    const int t = threadIdx.x;
    const int64_t i = (int64_t)col0 + (int64_t)blockIdx.x * EPS_BLK + t;
    const bool live = i < (int64_t)N;
    const int c_mine = live ? (int)cls[i] : EPS_MAX_CLASSES;  // >= n_classes: contributes to no class
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    if (live && c_mine < n_classes) {
        const int t0 = blockIdx.y * rows_per_slab;
        const int t1 = min(T, t0 + rows_per_slab);
        for (int r = t0; r < t1; r++) {
            const size_t row = (size_t)r * (size_t)N + (size_t)i;
            if (done[row] != 0.0f) {
                const double x = ep_ret[row];
                acc[0] += 1.0;
                acc[1] += x;
                acc[2] += x * x;
                acc[3] += (double)ep_len[row];
            }
        }
    }
    for (int c = 0; c < n_classes; c++) {
        const bool mine = c == c_mine;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            double v = mine ? acc[k] : 0.0;
            for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
            if ((t & 63) == 0) red[t >> 6][c][k] = v;
        }
    }
    __syncthreads();
    if (t < n_classes * 4) {
        const int c = t >> 2, k = t & 3;
        double s = red[0][c][k];
        for (int w = 1; w < EPS_BLK / 64; w++) s += red[w][c][k];
        const size_t b = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
        partial[b * (EPS_MAX_CLASSES * 4) + t] = s;
    }
}

constexpr int FOLD_GROUPS = 8;
constexpr int FOLD_BLK = FOLD_GROUPS * EPS_MAX_CLASSES * 4;

// entry e = (class, k) of the result: group j < 8 adds the partials of blocks j, j + 8, ... in that order, then the 8
// group sums are added in group order (one thread per entry walking every block waited a load latency per block)
__global__ __launch_bounds__(FOLD_BLK) void k_eps_fold(const double *__restrict__ partial, int nblocks, int n_classes,
                                                       double *__restrict__ out, int accumulate) {
    __shared__ double red[FOLD_GROUPS][EPS_MAX_CLASSES * 4];
    const int e = threadIdx.x % (EPS_MAX_CLASSES * 4), j = threadIdx.x / (EPS_MAX_CLASSES * 4);
    double s = 0.0;
    if (e < n_classes * 4) {
#pragma unroll 4
        for (int b = j; b < nblocks; b += FOLD_GROUPS) s += partial[(size_t)b * (EPS_MAX_CLASSES * 4) + e];
    }
    red[j][e] = s;
    __syncthreads();
    if (j == 0 && e < n_classes * 4) {
        double v = red[0][e];
        for (int g = 1; g < FOLD_GROUPS; g++) v += red[g][e];
        out[e] = accumulate ? out[e] + v : v;
    }
}

}  // namespace

hipError_t launch_episode_class_stats(const float *done, const double *ep_ret, const int32_t *ep_len,
                                      const uint8_t *cls, int T, int N, int n_classes, double *out, int accumulate,
                                      double *partial, hipStream_t s) {
    if (n_classes <= 0) return hipSuccess;
    if (T <= 0 || N <= 0) {
        hipLaunchKernelGGL(k_eps_fold, dim3(1), dim3(FOLD_BLK), 0, s, (const double *)partial, 0, n_classes, out,
                           accumulate);
        return hipGetLastError();
    }
    // column tiles x step slabs: about EPS_TARGET_BLOCKS blocks (one per CU; each thread then adds a run of rows, and
    // the fold has few partials to add), never more than EPS_MAX_BLOCKS (the workspace); more than EPS_MAX_BLOCKS
    // column tiles (over 262,144 envs) go in several rounds, each folded into out after the one before
    const int64_t tiles = ((int64_t)N + EPS_BLK - 1) / EPS_BLK;
    for (int64_t tile0 = 0; tile0 < tiles; tile0 += EPS_MAX_BLOCKS) {
        const int gx = (int)std::min<int64_t>(tiles - tile0, EPS_MAX_BLOCKS);
        const int slabs = std::max(1, std::min(T, EPS_TARGET_BLOCKS / gx));
        const int rows_per_slab = (T + slabs - 1) / slabs;
        const int gy = (T + rows_per_slab - 1) / rows_per_slab;
        hipLaunchKernelGGL(k_eps_partial, dim3(gx, gy), dim3(EPS_BLK), 0, s, done, ep_ret, ep_len, cls, T, N,
                           (int)(tile0 * EPS_BLK), rows_per_slab, n_classes, partial);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_eps_fold, dim3(1), dim3(FOLD_BLK), 0, s, (const double *)partial, gx * gy, n_classes, out,
                           (accumulate || tile0 > 0) ? 1 : 0);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace merlin
