// merlin_gemm.hip -- fc1 of both towers (src/actor_critic.py:31-41, Linear(576, 512) -> ReLU) in
// fp32 on the bf16 matrix cores: forward with the bias + ReLU epilogue, the input gradient and the
// split-K weight gradient of PPO.update's minibatch step (src/ppo.py:141-156).
//
// gfx950 has no reduced-precision f32 MFMA (no xf32) and its f32-input MFMA runs at 1/16 of the
// bf16 rate.  An fp32 value x is stored as three bf16 planes x = x0 + x1 + x2, EXACTLY: x0 =
// bf16(x) (round to nearest), x1 = bf16(x - x0), x2 = bf16(x - x0 - x1); each subtraction is exact
// in fp32 and each plane takes the next 8 of the 24 significand bits, so nothing is lost.  A
// product a*b is then sum_{i+j<=2} a_i*b_j, six bf16 MFMAs with fp32 accumulation (x6_mma6 in
// merlin_x6_tile.h says what is left out and in which order they are summed).  So these GEMMs
// compute fp32 products at 16/6 of the f32 MFMA rate (tests/test_gpu_gemm.py measures the error
// against float64 beside hipBLASLt's fp32 GEMM on the same operands).
//
// The activations (fc1's input rows a3 and output gradient dz, the big operands) are read as fp32
// and split in registers while they are staged into LDS; the weights are split once per call into
// "x6 planes" (merlin_x6.h: bf16 [R][C/8][3][8]).
//
// What lives where: merlin_x6_tile.h holds the two shared bodies (x6_nt_body, x6_tn_body) and every
// piece of them -- stagers, pipeline, six-product step, epilogue, launches.  This file has the plane
// split / join, the slab fold, the kernels on the 16x16x32 MFMA (k_x6_nt a wrapper of x6_nt_body;
// k_x6_tn, whose <128,192,2,4> is the weight gradient fc1 selects, with its own text: see there) and
// the library's x6 entry points; merlin_gemm2.hip has the kernels on the 32x32x16 MFMA (its own
// translation unit: built without SLP vectorisation).
//
//   k_x6_nt  C[t][m][n] = epi(sum_k A[t][m][k] B[t][n][k]), A fp32 [M][K], B planes [N][K]
//            (forward with B = W4, input gradient with B = W4^T); k steps of 32, each step's six
//            products in a fresh accumulator.
//   k_x6_tn  slab[s][t][m][n] = sum_{k in split s} A[t][k][m] B[t][k][n], A and B fp32 row-major
//            over the long reduction dimension k = the minibatch's frames (weight gradient dz^T
//            a3); k_x6_fold sums the slabs in split order.
#include "merlin_x6_tile.h"

namespace merlin {
namespace {

__global__ __launch_bounds__(256) void k_x6_split(const float4 *__restrict__ x, int64_t n4,
                                                  uint2 *__restrict__ planes) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n4; e += (int64_t)gridDim.x * 256)
        x6_store4(planes, e, x[e]);
}

// planes -> fp32 (tests: the planes must add back to the input exactly)
__global__ __launch_bounds__(256) void k_x6_join(const uint2 *__restrict__ planes, int64_t n4,
                                                 float4 *__restrict__ x) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n4; e += (int64_t)gridDim.x * 256) {
        const uint2 *s = planes + (e >> 1) * 6 + (e & 1);
        const uint2 a = s[0], b = s[2], c = s[4];
        x[e] = make_float4(x6_lo(a.x) + x6_lo(b.x) + x6_lo(c.x), x6_hi(a.x) + x6_hi(b.x) + x6_hi(c.x),
                           x6_lo(a.y) + x6_lo(b.y) + x6_lo(c.y), x6_hi(a.y) + x6_hi(b.y) + x6_hi(c.y));
    }
}

// the wave's 16 x 16 tiles: the fragments of the operand with fewer of them stay in registers
template <int BM, int BN, int WGM, int WGN>
constexpr int walk16 = (BM / WGM <= BN / WGN) ? X6_WALK_A : X6_WALK_B;

template <int BM, int BN, int WGM, int WGN, int EPI>
__global__ __launch_bounds__(64 * WGM * WGN) void k_x6_nt(const float4 *__restrict__ A, const u32x4 *__restrict__ B,
                                                          int64_t M, int N, int K, int64_t sA, int64_t sB,
                                                          const float *__restrict__ bias, float *__restrict__ C,
                                                          int64_t sC, int tiles_n) {
    x6_nt_body<Mfma16, BK, false, walk16<BM, BN, WGM, WGN>, const float4 *, const u32x4 *, BM, BN, WGM, WGN, EPI>(
        A, B, M, N, K, sA, sB, bias, C, sC, tiles_n);
}

// k_x6_tn's own fragment read and six-product step (x6_tr_frag and x6_mma6 on Mfma16, with bf16x8 fragments)
template <int RC>
__device__ __forceinline__ bf16x8 tr16_frag(const u32x4 *img, int col0, int lane) {
    // rows 8G + 4h + q, columns col0 + 4 * pp .. + 3 (G = lane >> 4, q = (lane >> 2) & 3, pp = lane & 3)
    const int G = lane >> 4, q = (lane >> 2) & 3, pp = lane & 3;
    const int chunk = (col0 >> 3) + (pp >> 1);
    bf16x4 v[2];
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const int row = 8 * G + 4 * h + q;
        const int off = (row * RC + (chunk ^ Mfma16::tr_swz<RC>(row))) * 16 + (pp & 1) * 8;
        v[h] = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4 *)((lds_char *)img + off));
    }
    return bf16x8{v[0][0], v[0][1], v[0][2], v[0][3], v[1][0], v[1][1], v[1][2], v[1][3]};
}
__device__ __forceinline__ f32x4 mma6(const bf16x8 a[3], const bf16x8 b[3], f32x4 acc) {
    f32x4 c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[2], b[0], f32x4{0.0f, 0.0f, 0.0f, 0.0f}, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1], b[1], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[2], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1], b[0], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[1], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[0], c, 0, 0, 0);
    return acc + c;
}

template <int BM, int BN, int WGM, int WGN>
__global__ __launch_bounds__(64 * WGM * WGN) void k_x6_tn(const float4 *__restrict__ A, const float4 *__restrict__ B,
                                                          int64_t Kd, int M, int N, int64_t sA, int64_t sB, int64_t kc,
                                                          int tiles_n, int tiles, int S, float *__restrict__ slab) {
    // Its own text, not x6_tn_body<Mfma16, BK, false, walk16<..>, ..>: on the shared body the selected
    // k_x6_tn<128,192,2,4> had the parent's instruction counts but another main-loop schedule and ran 1.6-1.8 % slower
    // at the update's shape.  Same algorithm as x6_tn_body, whose comments apply.
    constexpr int NT = 64 * WGM * WGN;
    constexpr int WTM = BM / WGM, WTN = BN / WGN;
    constexpr int FM = WTM / 16, FN = WTN / 16;
    constexpr int RCA = BM / 8, RCB = BN / 8;            // chunks (groups of 8 values) per image row
    constexpr int QA = BK * RCA, QB = BK * RCB;          // units per k step
    constexpr int UA = (QA + NT - 1) / NT, UB = (QB + NT - 1) / NT;
    static_assert(WTM % 16 == 0 && WTN % 16 == 0, "wave tile");
    constexpr int PSA = BK * RCA, PSB = BK * RCB;
    constexpr int STAGE = 3 * (PSA + PSB);
    __shared__ u32x4 lds[2 * STAGE];

    const int P = xcd_tile(blockIdx.x, gridDim.x);
    const int t = P / (S * tiles), s = (P / tiles) % S, L = P % tiles;
    const int tm = L / tiles_n, tn = L - tm * tiles_n;
    const int m0 = tm * BM, n0 = tn * BN;
    const int64_t k0 = (int64_t)s * kc, k1 = std::min<int64_t>(Kd, k0 + kc);
    const int64_t rowA = M / 4, rowB = N / 4;  // float4 per row
    A += t * sA + m0 / 4;
    B += t * sB + n0 / 4;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int wm = w / WGN, wn = w - (w / WGN) * WGN;

    int ka[UA], oa[UA], la[UA];
#pragma unroll
    for (int i = 0; i < UA; i++) {
        const int q = std::min(tid + i * NT, QA - 1);
        const int k = q / RCA, g = q - (q / RCA) * RCA;
        ka[i] = k;
        oa[i] = g * 2;
        la[i] = k * RCA + (g ^ Mfma16::tr_swz<RCA>(k));
    }
    int kb[UB], ob[UB], lb[UB];
#pragma unroll
    for (int i = 0; i < UB; i++) {
        const int q = std::min(tid + i * NT, QB - 1);
        const int k = q / RCB, g = q - (q / RCB) * RCB;
        kb[i] = k;
        ob[i] = g * 2;
        lb[i] = 3 * PSA + k * RCB + (g ^ Mfma16::tr_swz<RCB>(k));
    }
    const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float4 ra[UA][2], rb[UB][2];
    const float4 *pa[UA], *pb[UB];
#pragma unroll
    for (int i = 0; i < UA; i++) pa[i] = A + (k0 + ka[i]) * rowA + oa[i];
#pragma unroll
    for (int i = 0; i < UB; i++) pb[i] = B + (k0 + kb[i]) * rowB + ob[i];
    auto load = [&](int64_t kk) {
        if (kk + BK <= k1) {
            const int64_t da = (kk - k0) * rowA, db = (kk - k0) * rowB;
#pragma unroll
            for (int i = 0; i < UA; i++) {
                ra[i][0] = pa[i][da];
                ra[i][1] = pa[i][da + 1];
            }
#pragma unroll
            for (int i = 0; i < UB; i++) {
                rb[i][0] = pb[i][db];
                rb[i][1] = pb[i][db + 1];
            }
            return;
        }
#pragma unroll
        for (int i = 0; i < UA; i++) {
            const int64_t k = kk + ka[i];
            const float4 *src = A + std::min(k, k1 - 1) * rowA + oa[i];
            ra[i][0] = src[0];
            ra[i][1] = src[1];
        }
#pragma unroll
        for (int i = 0; i < UB; i++) {
            const int64_t k = kk + kb[i];
            const float4 *src = B + std::min(k, k1 - 1) * rowB + ob[i];
            rb[i][0] = src[0];
            rb[i][1] = src[1];
        }
    };
    auto store = [&](int buf, int64_t kk) {
        u32x4 *st = lds + buf * STAGE;
#pragma unroll
        for (int i = 0; i < UA; i++)
            if (QA % NT == 0 || i + 1 < UA || tid + i * NT < QA) {
                const bool in = kk + ka[i] < k1;
                u32x4 p0, p1, p2;
                split8(in ? ra[i][0] : zero, in ? ra[i][1] : zero, p0, p1, p2);
                st[la[i]] = p0;
                st[PSA + la[i]] = p1;
                st[2 * PSA + la[i]] = p2;
            }
#pragma unroll
        for (int i = 0; i < UB; i++)
            if (QB % NT == 0 || i + 1 < UB || tid + i * NT < QB) {
                const bool in = kk + kb[i] < k1;
                u32x4 p0, p1, p2;
                split8(in ? rb[i][0] : zero, in ? rb[i][1] : zero, p0, p1, p2);
                st[lb[i]] = p0;
                st[PSB + lb[i]] = p1;
                st[2 * PSB + lb[i]] = p2;
            }
    };

    f32x4 acc[FM][FN];
#pragma unroll
    for (int i = 0; i < FM; i++)
#pragma unroll
        for (int j = 0; j < FN; j++) acc[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    if (k0 < k1) {
        load(k0);
        store(0, k0);
        if (k0 + BK < k1) load(k0 + BK);
        __syncthreads();
    }
    int buf = 0;
    for (int64_t kk = k0; kk < k1; kk += BK, buf ^= 1) {
        if (kk + BK < k1) store(buf ^ 1, kk + BK);
        if (kk + 2 * BK < k1) load(kk + 2 * BK);
        const u32x4 *sAl = lds + buf * STAGE, *sBl = sAl + 3 * PSA;
        if constexpr (FM <= FN) {
            bf16x8 af[FM][3];
#pragma unroll
            for (int i = 0; i < FM; i++)
#pragma unroll
                for (int p = 0; p < 3; p++) af[i][p] = tr16_frag<RCA>(sAl + p * PSA, wm * WTM + i * 16, lane);
#pragma unroll
            for (int j = 0; j < FN; j++) {
                bf16x8 bf[3];
#pragma unroll
                for (int p = 0; p < 3; p++) bf[p] = tr16_frag<RCB>(sBl + p * PSB, wn * WTN + j * 16, lane);
#pragma unroll
                for (int i = 0; i < FM; i++) acc[i][j] = mma6(af[i], bf, acc[i][j]);
            }
        } else {
            bf16x8 bf[FN][3];
#pragma unroll
            for (int j = 0; j < FN; j++)
#pragma unroll
                for (int p = 0; p < 3; p++) bf[j][p] = tr16_frag<RCB>(sBl + p * PSB, wn * WTN + j * 16, lane);
#pragma unroll
            for (int i = 0; i < FM; i++) {
                bf16x8 af[3];
#pragma unroll
                for (int p = 0; p < 3; p++) af[p] = tr16_frag<RCA>(sAl + p * PSA, wm * WTM + i * 16, lane);
#pragma unroll
                for (int j = 0; j < FN; j++) acc[i][j] = mma6(af, bf[j], acc[i][j]);
            }
        }
        __syncthreads();
    }

    float *St = slab + ((int64_t)s * (gridDim.x / (S * tiles)) + t) * (int64_t)M * N;
    const int fr = lane & 15;
#pragma unroll
    for (int i = 0; i < FM; i++)
#pragma unroll
        for (int j = 0; j < FN; j++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int row = m0 + wm * WTM + i * 16 + 4 * (lane >> 4) + r;
                St[(int64_t)row * N + n0 + wn * WTN + j * 16 + fr] = acc[i][j][r];
            }
}

// out[e] = sum over s of slab[s][e] (e < total4 float4s), in split order
__global__ __launch_bounds__(256) void k_x6_fold(const float4 *__restrict__ slab, int S, int64_t total4,
                                                 float4 *__restrict__ out) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total4; e += (int64_t)gridDim.x * 256) {
        float4 a = slab[e];
        for (int s = 1; s < S; s++) {
            const float4 v = slab[(int64_t)s * total4 + e];
            a.x += v.x;
            a.y += v.y;
            a.z += v.z;
            a.w += v.w;
        }
        out[e] = a;
    }
}

template <int BM, int BN, int WGM, int WGN, class... Args>
hipError_t nt_launch(Args... args) {
    return x6_nt_launch<BM, BN, 64 * WGM * WGN>(k_x6_nt<BM, BN, WGM, WGN, 1>, k_x6_nt<BM, BN, WGM, WGN, 0>, args...);
}

template <int BM, int BN, int WGM, int WGN, class... Args>
hipError_t tn_launch(Args... args) {
    return x6_tn_launch<BK, BM, BN, 64 * WGM * WGN>(k_x6_tn<BM, BN, WGM, WGN>, args...);
}

}  // namespace

hipError_t launch_x6_split(const float *x, int64_t n, void *planes, hipStream_t s) {
    if (n % 8) return hipErrorInvalidValue;
    const int64_t n4 = n / 4;
    if (n4 <= 0) return hipSuccess;
    const int grid = (int)std::min<int64_t>((n4 + 255) / 256, 256 * 16);
    hipLaunchKernelGGL(k_x6_split, dim3(grid), dim3(256), 0, s, reinterpret_cast<const float4 *>(x), n4,
                       reinterpret_cast<uint2 *>(planes));
    return hipGetLastError();
}

hipError_t launch_x6_join(const void *planes, int64_t n, float *x, hipStream_t s) {
    if (n % 8) return hipErrorInvalidValue;
    const int64_t n4 = n / 4;
    if (n4 <= 0) return hipSuccess;
    const int grid = (int)std::min<int64_t>((n4 + 255) / 256, 256 * 16);
    hipLaunchKernelGGL(k_x6_join, dim3(grid), dim3(256), 0, s, reinterpret_cast<const uint2 *>(planes), n4,
                       reinterpret_cast<float4 *>(x));
    return hipGetLastError();
}

hipError_t launch_x6_gemm_nt(const float *A, const void *B, int64_t M, int N, int K, int T, int64_t a_stride,
                             int64_t b_stride, const float *bias, float *C, int64_t c_stride, int cfg, hipStream_t s) {
    if (M <= 0) return hipSuccess;
    if (K % BK || N <= 0) return hipErrorInvalidValue;
    // strides in values; B's planes: 3 chunks per 8 values
    if (a_stride % 4 || b_stride % 8) return hipErrorInvalidValue;
    if (cfg >= 20)  // the 32x32x16 MFMA kernels (merlin_gemm2.hip)
        return launch_x6_gemm_nt32(A, B, M, N, K, T, a_stride, b_stride, bias, C, c_stride, cfg, s);
    const float4 *a = reinterpret_cast<const float4 *>(A);
    const u32x4 *b = static_cast<const u32x4 *>(B);
    const int64_t sA = a_stride / 4, sB = b_stride / 8 * 3;
    switch (cfg) {
        case 0: return nt_launch<256, 128, 4, 2>(a, b, M, N, K, T, sA, sB, bias, C, c_stride, s);
        case 1: return nt_launch<128, 192, 2, 4>(a, b, M, N, K, T, sA, sB, bias, C, c_stride, s);
        case 2: return nt_launch<128, 128, 2, 2>(a, b, M, N, K, T, sA, sB, bias, C, c_stride, s);
        case 3: return nt_launch<256, 64, 4, 2>(a, b, M, N, K, T, sA, sB, bias, C, c_stride, s);
        default: return hipErrorInvalidValue;
    }
}

int x6_tn_max_splits() { return 64; }

hipError_t launch_x6_fold(const float *slab, int S, int64_t total, float *out, hipStream_t s) {
    if (total % 4) return hipErrorInvalidValue;
    const int64_t total4 = total / 4;
    const int grid = (int)std::min<int64_t>((total4 + 255) / 256, 256 * 8);
    hipLaunchKernelGGL(k_x6_fold, dim3(grid), dim3(256), 0, s, reinterpret_cast<const float4 *>(slab), S, total4,
                       reinterpret_cast<float4 *>(out));
    return hipGetLastError();
}

hipError_t launch_x6_gemm_tn(const float *A, const float *B, int64_t Kd, int M, int N, int T, int64_t a_stride,
                             int64_t b_stride, int splits, float *slab, float *out, int cfg, hipStream_t s) {
    if (M <= 0 || N <= 0) return hipSuccess;
    if (M % 8 || N % 8 || a_stride % 4 || b_stride % 4) return hipErrorInvalidValue;
    if (Kd <= 0) return zero_async(out, sizeof(float) * (size_t)T * M * N, s);
    const float4 *a = reinterpret_cast<const float4 *>(A), *b = reinterpret_cast<const float4 *>(B);
    const int64_t sA = a_stride / 4, sB = b_stride / 4;
    int S = 1;  // the slabs the kernel wrote
    hipError_t e;
    switch (cfg) {
        case 0: e = tn_launch<128, 192, 2, 4>(a, b, Kd, M, N, T, sA, sB, splits, slab, s, &S); break;
        case 1: e = tn_launch<128, 64, 2, 2>(a, b, Kd, M, N, T, sA, sB, splits, slab, s, &S); break;
        case 2: e = tn_launch<128, 192, 4, 2>(a, b, Kd, M, N, T, sA, sB, splits, slab, s, &S); break;
        // the 32x32x16 MFMA kernels (merlin_gemm2.hip: cfg >= 20, every other number is refused there)
        default: e = launch_x6_gemm_tn32(A, B, Kd, M, N, T, a_stride, b_stride, splits, slab, cfg, s, &S);
    }
    if (e != hipSuccess) return e;
    return launch_x6_fold(slab, S, (int64_t)T * M * N, out, s);
}

}  // namespace merlin
