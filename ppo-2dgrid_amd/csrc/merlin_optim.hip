// merlin_optim.hip -- the optimizer step of PPO.update (src/ppo.py:153-156):
//   clip_grad_norm_(params, max_norm)  then  Adam.step()
// in two launches over all parameter tensors at once (torch's chain is ~10 launches: foreach
// norm + its cleanup, stack, vector_norm, coefficient, clamp, foreach mul, step-count add,
// fused Adam).  The tensors are passed by value in the kernel arguments (pointer lists, at most
// OPT_MAX_TENSORS), each cut into OPT_CHUNK-element blocks.
//   k_opt_sumsq   per block: sum of squared gradients (f64 partial); the first block of a tensor
//                 advances its Adam step counter (f32, torch's on-device `step` state).
//   k_opt_adam    per block: the global norm from the partials (every block sums the same
//                 partials in the same order, so all agree bit for bit), the clip coefficient
//                 min(max_norm / (norm + 1e-6), 1) applied to the gradient (written back, as
//                 clip_grad_norm_ does), then torch's fused-Adam arithmetic on (p, m, v).
// Bytes per parameter: 4 (grad, pass 1) + 16 read + 16 written (pass 2).
//
// The chained form (launch_clip_adam with an OptChain; merlin/fast_step.py's weight-only chain) has the same two
// launches take over their neighbours in the benched step, with the same arithmetic on the parameters:
//   k_opt_sumsq   block 0 also zeroes two short word lists by plain stores (the next step's operand scales and the
//                 fc1 weight scale, which k_opt_adam then rebuilds) -- launches of their own before;
//   k_opt_adam    writes each stepped value to the element's (at most two) slots of the derived-weight buffer D as
//                 well (an indexed gather of all parameters before), folds |p| of the tensors that have a scale word
//                 into it (one atomicMax of float bits per wave; a pass over D's copy before), and block 0 adds the
//                 norm to the update's running total (two torch launches before).
#include "merlin_internal.h"

namespace merlin {
namespace {

constexpr int OPT_BLK = 256;
constexpr int OPT_PER_THREAD = 4;  // ~730 blocks for the 745k parameters: fills the chip
constexpr int OPT_CHUNK = OPT_BLK * OPT_PER_THREAD;

struct OptList {
    int n;
    int blk0[OPT_MAX_TENSORS + 1];  // first block of tensor i; blk0[n] = total blocks
    int64_t numel[OPT_MAX_TENSORS];
    float *p[OPT_MAX_TENSORS];
    float *g[OPT_MAX_TENSORS];
    float *m[OPT_MAX_TENSORS];
    float *v[OPT_MAX_TENSORS];
    float *step[OPT_MAX_TENSORS];
};

__device__ __forceinline__ int tensor_of(const OptList &L, int b) {
    int i = 0;
    while (i + 1 < L.n && L.blk0[i + 1] <= b) i++;
    return i;
}

__device__ double block_sum(double x, double *red) {
    const int t = threadIdx.x;
    for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
    if ((t & 63) == 0) red[t >> 6] = x;
    __syncthreads();
    double s = 0.0;
    if (t == 0)
        for (int w = 0; w < OPT_BLK / 64; w++) s += red[w];
    return s;  // valid in thread 0
}

template <bool CHAIN>
__global__ __launch_bounds__(OPT_BLK) void k_opt_sumsq(OptList L, double *partial, OptChain C) {
    __shared__ double red[OPT_BLK / 64];
    const int b = blockIdx.x, i = tensor_of(L, b);
    if (CHAIN && b == 0) {
        for (int z = 0; z < 2; z++)
            for (int j = threadIdx.x; j < C.n_zero[z]; j += OPT_BLK) C.zero[z][j] = 0u;
    }
    const int64_t base = (int64_t)(b - L.blk0[i]) * OPT_CHUNK, n = L.numel[i];
    const float *g = L.g[i];
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < OPT_PER_THREAD; k++) {
        const int64_t e = base + k * OPT_BLK + threadIdx.x;
        if (e < n) {
            const float x = g[e];
            acc += x * x;
        }
    }
    const double s = block_sum((double)acc, red);
    if (threadIdx.x == 0) {
        partial[b] = s;
        if (b == L.blk0[i] && L.step[i]) L.step[i][0] += 1.0f;
    }
}

template <bool CHAIN>
__global__ __launch_bounds__(OPT_BLK) void k_opt_adam(OptList L, const double *partial, int nblk, double lr, double beta1,
                                                     double beta2, double eps, float max_norm, float *norm_out,
                                                     OptChain C) {
    __shared__ double red[OPT_BLK / 64];
    __shared__ float coef_s;
    double x = 0.0;
    for (int j = threadIdx.x; j < nblk; j += OPT_BLK) x += partial[j];
    const double tot = block_sum(x, red);
    if (threadIdx.x == 0) {
        const float norm = (float)sqrt(tot);
        float c = max_norm / (norm + 1e-6f);
        // torch.clamp(max=1) keeps a NaN coefficient (non-finite norm): every gradient and
        // parameter then turns NaN, as with clip_grad_norm_, instead of a partly hidden step
        coef_s = (c != c) ? c : (c < 1.0f ? c : 1.0f);
        if (blockIdx.x == 0 && norm_out) norm_out[0] = norm;
        if (CHAIN && blockIdx.x == 0 && C.total) C.total[0] = C.total[0] + (double)norm;
    }
    __syncthreads();
    const float coef = coef_s;
    const int b = blockIdx.x, i = tensor_of(L, b);
    const int64_t base = (int64_t)(b - L.blk0[i]) * OPT_CHUNK, n = L.numel[i];
    // torch fused Adam (ATen fused_adam_utils.cuh adam_math, no weight decay / amsgrad / maximize):
    // lr, beta1, beta2, eps are doubles there, so the moment updates and the bias corrections are
    // evaluated in double and rounded to fp32 once, step_size / denom / the parameter in fp32
    const double stepc = (double)L.step[i][0];
    const float bc1 = (float)(1.0 - pow(beta1, stepc));
    const float bc2_sqrt = (float)sqrt(1.0 - pow(beta2, stepc));
    const float step_size = (float)(lr / (double)bc1);
    float *__restrict__ p = L.p[i];
    float *__restrict__ g = L.g[i];
    float *__restrict__ m = L.m[i];
    float *__restrict__ v = L.v[i];
    float rg[OPT_PER_THREAD], rm[OPT_PER_THREAD], rv[OPT_PER_THREAD], rp[OPT_PER_THREAD];
    // chained: the element's slots in D (its index in the flat parameter buffer -> two slot numbers, -1: none)
    int2 rs[OPT_PER_THREAD];
    const int2 *__restrict__ slots = CHAIN ? C.slots + (L.p[i] - C.flat) : nullptr;
    uint32_t am = 0u;
#pragma unroll
    for (int k = 0; k < OPT_PER_THREAD; k++) {  // all loads in flight before the arithmetic
        const int64_t e = base + k * OPT_BLK + threadIdx.x;
        if (e < n) {
            rg[k] = g[e];
            rm[k] = m[e];
            rv[k] = v[e];
            rp[k] = p[e];
            if (CHAIN) rs[k] = slots[e];
        }
    }
#pragma unroll
    for (int k = 0; k < OPT_PER_THREAD; k++) {
        const int64_t e = base + k * OPT_BLK + threadIdx.x;
        if (e < n) {
            const float gr = rg[k] * coef;
            const float ma = (float)(beta1 * (double)rm[k] + (1.0 - beta1) * (double)gr);
            const float va = (float)(beta2 * (double)rv[k] + (1.0 - beta2) * (double)gr * (double)gr);
            const float denom = (float)((double)(sqrtf(va) / bc2_sqrt) + eps);
            g[e] = gr;
            m[e] = ma;
            v[e] = va;
            const float pn = rp[k] - step_size * ma / denom;
            p[e] = pn;
            if (CHAIN) {
                if (rs[k].x >= 0) C.D[rs[k].x] = pn;
                if (rs[k].y >= 0) C.D[rs[k].y] = pn;
                am = max(am, __float_as_uint(pn) & 0x7fffffffu);
            }
        }
    }
    if (CHAIN && C.amax_slot[i] >= 0) {  // (block-uniform) max |p| of a scaled tensor, as float bits
        // per wave, then per block, and the atomic only where the block's maximum is above the word (it only grows):
        // same-address atomics serialise at the memory side -- one per wave, 2,304 on fc1's two words, took ~25 us
        __shared__ uint32_t amr[OPT_BLK / 64];
        for (int o = 32; o > 0; o >>= 1) am = max(am, (uint32_t)__shfl_xor((int)am, o));
        if ((threadIdx.x & 63) == 0) amr[threadIdx.x >> 6] = am;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t *w = C.amax + C.amax_slot[i];
            for (int q = 1; q < OPT_BLK / 64; q++) am = max(am, amr[q]);
            if (am && am > __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(w, am);
        }
    }
}

}  // namespace

int64_t opt_blocks(int n, const int64_t *numel) {
    int64_t b = 0;
    for (int i = 0; i < n; i++) b += (numel[i] + OPT_CHUNK - 1) / OPT_CHUNK;
    return b;
}

hipError_t launch_clip_adam(int n, float *const *params, float *const *grads, float *const *exp_avg,
                            float *const *exp_avg_sq, float *const *steps, const int64_t *numel, double lr, double beta1,
                            double beta2, double eps, float max_norm, float *norm_out, double *partial, hipStream_t s,
                            const OptChain *chain) {
    OptList L{};
    L.n = n;
    int blocks = 0;
    for (int i = 0; i < n; i++) {
        L.blk0[i] = blocks;
        L.numel[i] = numel[i];
        L.p[i] = params[i];
        L.g[i] = grads[i];
        L.m[i] = exp_avg[i];
        L.v[i] = exp_avg_sq[i];
        L.step[i] = steps[i];
        blocks += (int)((numel[i] + OPT_CHUNK - 1) / OPT_CHUNK);
    }
    L.blk0[n] = blocks;
    if (blocks == 0) return hipSuccess;
    if (chain) {
        hipLaunchKernelGGL(k_opt_sumsq<true>, dim3((unsigned)blocks), dim3(OPT_BLK), 0, s, L, partial, *chain);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_opt_adam<true>, dim3((unsigned)blocks), dim3(OPT_BLK), 0, s, L, (const double *)partial,
                           blocks, lr, beta1, beta2, eps, max_norm, norm_out, *chain);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(k_opt_sumsq<false>, dim3((unsigned)blocks), dim3(OPT_BLK), 0, s, L, partial, OptChain{});
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_opt_adam<false>, dim3((unsigned)blocks), dim3(OPT_BLK), 0, s, L, (const double *)partial, blocks,
                       lr, beta1, beta2, eps, max_norm, norm_out, OptChain{});
    return hipGetLastError();
}

}  // namespace merlin
