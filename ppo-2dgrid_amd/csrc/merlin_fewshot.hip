// merlin_fewshot.hip -- the two reductions of few-shot evaluation (src/distribution_over_tasks.py:97-128, :200-203).
//
// group clip + SGD: clip_grad_norm_(fast.parameters(), max_norm) then SGD(lr).step() for G independent
// parameter sets at once.  Tensor i is float[G][numel[i]] (merlin.batched_policy.stack_params); each task's
// slice is cut into GS_CHUNK-element blocks, grid = (blocks per task, G).
//   k_gs_sumsq   per (task, block): sum of squared gradients, f64 partial at partial[task * nblk + block].
//   k_gs_step    per (task, block): the task's norm from its nblk partials (every block of a task sums the same
//                partials in the same order, so all agree bit for bit), coef = min(max_norm / (norm + 1e-6), 1)
//                with a NaN kept (k_opt_adam), g *= coef written back, p -= lr * g.
// No atomics; a task reads only its own partials, so a NaN gradient stays inside its task.
// Bytes per parameter: 4 (grad, pass 1) + 8 read + 8 written (pass 2).
//
// episode loss: n episodes stored [T][n], episode i of length[i] steps.  One thread per episode (rows are
// coalesced across episodes), three passes over its own steps only:
//   1. GAE backwards in k_gae_thread's fp32 order with the bootstrap masked at the last step (the value after
//      the episode never enters), advantages to the workspace, their sum in f64;
//   2. the unbiased variance about the f64 mean;
//   3. adv_n = (adv - mean) / (std + 1e-8) in fp32 (zeros for a 1-step episode), ret = value + adv_n,
//      loss = -mean(new_logp) + 0.5 mean((new_value - ret)^2), both sums in f64.
// Rows t >= length[i] are neither read nor written.
#include "merlin_internal.h"

namespace merlin {
namespace {

constexpr int GS_BLK = 256;
constexpr int GS_PER_THREAD = 4;
constexpr int GS_CHUNK = GS_BLK * GS_PER_THREAD;

struct GroupList {
    int n;
    int blk0[OPT_MAX_TENSORS + 1];  // first block of tensor i within a task; blk0[n] = blocks per task
    int64_t numel[OPT_MAX_TENSORS];
    float *p[OPT_MAX_TENSORS];
    float *g[OPT_MAX_TENSORS];
};

__device__ __forceinline__ int gs_tensor_of(const GroupList &L, int b) {
    int i = 0;
    while (i + 1 < L.n && L.blk0[i + 1] <= b) i++;
    return i;
}

__device__ double gs_block_sum(double x, double *red) {
    const int t = threadIdx.x;
    for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
    if ((t & 63) == 0) red[t >> 6] = x;
    __syncthreads();
    double s = 0.0;
    if (t == 0)
        for (int w = 0; w < GS_BLK / 64; w++) s += red[w];
    return s;  // valid in thread 0
}

__global__ __launch_bounds__(GS_BLK) void k_gs_sumsq(GroupList L, double *__restrict__ partial) {
    __shared__ double red[GS_BLK / 64];
    const int b = blockIdx.x, task = blockIdx.y, i = gs_tensor_of(L, b);
    const int64_t n = L.numel[i], base = (int64_t)(b - L.blk0[i]) * GS_CHUNK;
    const float *g = L.g[i] + (int64_t)task * n;
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < GS_PER_THREAD; k++) {
        const int64_t e = base + k * GS_BLK + threadIdx.x;
        if (e < n) {
            const float x = g[e];
            acc += x * x;
        }
    }
    const double s = gs_block_sum((double)acc, red);
    if (threadIdx.x == 0) partial[(int64_t)task * gridDim.x + b] = s;
}

__global__ __launch_bounds__(GS_BLK) void k_gs_step(GroupList L, const double *__restrict__ partial, float lr,
                                                   float max_norm, float *__restrict__ norm_out) {
    __shared__ double red[GS_BLK / 64];
    __shared__ float coef_s;
    const int b = blockIdx.x, task = blockIdx.y, nblk = gridDim.x;
    const double *mine = partial + (int64_t)task * nblk;
    double x = 0.0;
    for (int j = threadIdx.x; j < nblk; j += GS_BLK) x += mine[j];
    const double tot = gs_block_sum(x, red);
    if (threadIdx.x == 0) {
        const float norm = (float)sqrt(tot);
        const float c = max_norm / (norm + 1e-6f);
        coef_s = (c != c) ? c : (c < 1.0f ? c : 1.0f);  // torch.clamp(max=1) keeps a NaN coefficient
        if (b == 0 && norm_out) norm_out[task] = norm;
    }
    __syncthreads();
    const float coef = coef_s;
    const int i = gs_tensor_of(L, b);
    const int64_t n = L.numel[i], base = (int64_t)(b - L.blk0[i]) * GS_CHUNK;
    float *__restrict__ p = L.p[i] + (int64_t)task * n;
    float *__restrict__ g = L.g[i] + (int64_t)task * n;
    float rg[GS_PER_THREAD], rp[GS_PER_THREAD];
#pragma unroll
    for (int k = 0; k < GS_PER_THREAD; k++) {  // all loads in flight before the arithmetic
        const int64_t e = base + k * GS_BLK + threadIdx.x;
        if (e < n) {
            rg[k] = g[e];
            rp[k] = p[e];
        }
    }
#pragma unroll
    for (int k = 0; k < GS_PER_THREAD; k++) {
        const int64_t e = base + k * GS_BLK + threadIdx.x;
        if (e < n) {
            const float gr = rg[k] * coef;
            g[e] = gr;
            p[e] = rp[k] - lr * gr;
        }
    }
}

constexpr int EL_BLK = 64;

__global__ __launch_bounds__(EL_BLK) void k_episode_loss(const float *__restrict__ rew, const float *__restrict__ val,
                                                        const float *__restrict__ nlp, const float *__restrict__ nval,
                                                        const int32_t *__restrict__ length, float *adv,
                                                        float *__restrict__ loss, int T, int N, float gf, float glf) {
    const int i = blockIdx.x * EL_BLK + threadIdx.x;
    if (i >= N) return;
    const size_t n = (size_t)N;
    int len = length[i];
    len = len < 1 ? 1 : (len > T ? T : len);  // never outside the [T][n] buffers
    // pass 1: k_gae_thread's recurrence; done = 1 at the episode's last step only, nothing after it
    float vnext = 0.0f, gae = 0.0f;
    double s1 = 0.0;
    for (int t = len - 1; t >= 0; t--) {
        const size_t k = (size_t)t * n + i;
        const float v = val[k];
        const float mask = (t == len - 1) ? 0.0f : 1.0f;
        const float delta = (rew[k] + (gf * vnext) * mask) - v;
        gae = delta + (glf * mask) * gae;
        adv[k] = gae;
        s1 += (double)gae;
        vnext = v;
    }
    const double mean = s1 / (double)len;
    // pass 2: this thread reads back what it wrote
    double s2 = 0.0;
    for (int t = 0; t < len; t++) {
        const double d = (double)adv[(size_t)t * n + i] - mean;
        s2 += d * d;
    }
    const float mf = (float)mean;
    const float denom = (float)sqrt(len > 1 ? s2 / (double)(len - 1) : 0.0) + 1e-8f;  // adv.std() + 1e-8 in f32
    // pass 3
    double slp = 0.0, sv = 0.0;
    for (int t = 0; t < len; t++) {
        const size_t k = (size_t)t * n + i;
        const float an = len > 1 ? (adv[k] - mf) / denom : 0.0f;
        const float ret = val[k] + an;
        const float err = nval[k] - ret;
        slp += (double)nlp[k];
        sv += (double)err * (double)err;
    }
    loss[i] = (float)(-slp / (double)len + 0.5 * (sv / (double)len));
}

}  // namespace

int64_t group_blocks(int n, const int64_t *numel) {
    int64_t b = 0;
    for (int i = 0; i < n; i++) b += (numel[i] + GS_CHUNK - 1) / GS_CHUNK;
    return b;
}

hipError_t launch_group_clip_sgd(int n, float *const *params, float *const *grads, const int64_t *numel, int G,
                                 float lr, float max_norm, float *norm_out, double *partial, hipStream_t s) {
    GroupList L{};
    L.n = n;
    int blocks = 0;
    for (int i = 0; i < n; i++) {
        L.blk0[i] = blocks;
        L.numel[i] = numel[i];
        L.p[i] = params[i];
        L.g[i] = grads[i];
        blocks += (int)((numel[i] + GS_CHUNK - 1) / GS_CHUNK);
    }
    L.blk0[n] = blocks;
    if (blocks == 0 || G <= 0) return hipSuccess;
    const dim3 grid((unsigned)blocks, (unsigned)G);
    hipLaunchKernelGGL(k_gs_sumsq, grid, dim3(GS_BLK), 0, s, L, partial);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_gs_step, grid, dim3(GS_BLK), 0, s, L, (const double *)partial, lr, max_norm, norm_out);
    return hipGetLastError();
}

hipError_t launch_episode_loss(const float *rew, const float *val, const float *nlp, const float *nval,
                               const int32_t *length, int T, int N, double gamma, double lam, float *adv_ws,
                               float *loss, hipStream_t s) {
    if (N <= 0) return hipSuccess;
    const float gf = (float)gamma;
    const float glf = (float)(gamma * lam);  // as launch_gae
    hipLaunchKernelGGL(k_episode_loss, dim3((N + EL_BLK - 1) / EL_BLK), dim3(EL_BLK), 0, s, rew, val, nlp, nval, length,
                       adv_ws, loss, T, N, gf, glf);
    return hipGetLastError();
}

}  // namespace merlin
