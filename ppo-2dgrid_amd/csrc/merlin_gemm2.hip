// merlin_gemm2.hip -- fc1's GEMMs on the 32x32x16 bf16 MFMA, same exact three-plane fp32 products as merlin_gemm.hip
// (merlin_x6.h).  k_x6_nt32b, k_x6_tn32 and k_x6_tn32k16 instantiate the shared bodies (merlin_x6_tile.h: x6_nt_body,
// x6_tn_body) on Mfma32, each with what it picks; k_x6_nt32, which holds the three NT kernels fc1 selects, keeps its own
// text (see there).  Then the launches of their configurations.  Its own translation unit because it is built
// without SLP vectorisation (packed f32 adds beside MFMAs cost issue slots).
//
// Why a second family: k_x6_nt issues one 16x16x32 MFMA per 16 matrix-pipe cycles, of which the MFMA itself holds the
// SIMD's issue port for 8; the k step's other instructions (the A split, LDS stores and fragment reads, the per-step
// accumulator adds, addressing) come to ~2.8 per MFMA, more than the ~2 issue slots each MFMA leaves free, so the
// matrix pipe idled half the time (profiles: MFMA busy 49 %).  v_mfma_f32_32x32x16_bf16 does twice the work per
// instruction for the same 8-cycle issue hold, which doubles the free issue slots per FLOP.
//
//   k_x6_nt32      NT, k steps of 32 (two MFMA k halves).  ACC 1: split hi / lo accumulators, so the per-step adds go
//                  too; ACC 0: the step's twelve products in a fresh accumulator.  B's chunk offsets in 32 bits.
//   k_x6_nt32b     NT, k steps of 16, four waves and two blocks per CU.  The 8-wave kernels hold a whole CU (one
//                  block: 122-147 KB of LDS), and one barrier per k step keeps both waves of each SIMD in the same
//                  phase, so the matrix pipe idles while they split, stage and wait for fragments together.  Here a
//                  block is one wave per SIMD with a 61-74 KB two-stage LDS ring, two blocks share a CU, and the two
//                  waves of a SIMD come from different blocks: one's staging runs beside the other's MFMAs.  Per-step
//                  accumulators; both operands' offsets in 32 bits (256 registers per lane at two blocks per CU).
//   k_x6_tn32      TN, k steps of 32, split hi / lo accumulators.
//   k_x6_tn32k16   TN, k steps of 16 and a bigger block tile: 256 x 192 (both of fc1's weight-gradient dimensions in
//                  2 x 3 tiles) over 8 waves of 64 x 96.  Per MFMA it stages, splits and reads from LDS 35-65 % less
//                  than the 128 x 192 / 32-deep form (the split and the staging are per element of the tile's edges,
//                  the MFMAs per element of its area); two 43-KB LDS stages.  Per-step accumulators: 96 + 16
//                  registers instead of the 192 of split hi / lo sums.
#include "merlin_x6_tile.h"

namespace merlin {
namespace {

template <int BM, int BN, int WGM, int WGN, int EPI, int ACC>
__global__ __launch_bounds__(64 * WGM * WGN) void k_x6_nt32(const void *__restrict__ Av, const u32x4 *__restrict__ B,
                                                            int64_t M, int N, int K, int64_t sA, int64_t sB,
                                                            const float *__restrict__ bias, float *__restrict__ C,
                                                            int64_t sC, int tiles_n) {
    // Its own text, not x6_nt_body<Mfma32, BK, ACC == 1, X6_WALK_IJ, const float4 *, int, ..>: on the shared body the
    // selected input-gradient kernel k_x6_nt32<128,192,4,2,0,1> had the parent's instruction counts, but its column
    // tiles' fragment addresses sat in registers of their own instead of ds_read immediates (loop block 92
    // instructions against 85) and it ran 1.8-2 % slower.  Same algorithm as
    // x6_nt_body, whose comments apply.
    constexpr int NT = 64 * WGM * WGN;
    constexpr int WTM = BM / WGM, WTN = BN / WGN;
    constexpr int TM = WTM / 32, TN = WTN / 32;
    constexpr int UA = (BM * 4 + NT - 1) / NT;  // A fp32 units
    constexpr int CB = (BN * CPR + NT - 1) / NT;
    static_assert(WTM % 32 == 0 && WTN % 32 == 0, "wave tile of 32 x 32 MFMA tiles");
    constexpr int PSA = BM * 4, PSB = BN * 4 + 12;
    constexpr int STAGE = 3 * (PSA + PSB);
    __shared__ u32x4 lds[2 * STAGE];

    const int t = blockIdx.y;
    const int L = xcd_tile(blockIdx.x, gridDim.x);
    const int tm = L / tiles_n, tn = L - tm * tiles_n;
    const int64_t m0 = (int64_t)tm * BM;
    const int n0 = tn * BN;
    const int64_t rowA = K / 4;  // A row in float4s
    const int64_t rowB = (int64_t)(K / 8) * 3;
    B += t * sB;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int wm = w / WGN, wn = w - (w / WGN) * WGN;

    const float4 *ga[UA];
    int la[UA];
#pragma unroll
    for (int i = 0; i < UA; i++) {
        const int q = tid + i * NT;
        const int row = std::min(q >> 2, BM - 1), g = q & 3;
        ga[i] = static_cast<const float4 *>(Av) + t * sA + std::min<int64_t>(m0 + row, M - 1) * rowA + g * 2;
        la[i] = row * 4 + (g ^ ((row >> 2) & 3));
    }
    int gb[CB];  // chunk offsets from B (the weights: N * K * 3 / 8 chunks, well inside 32 bits)
    int lb[CB];
#pragma unroll
    for (int i = 0; i < CB; i++) {
        const int q = tid + i * NT;
        const int row = q / CPR, rem = q - (q / CPR) * CPR, p = rem >> 2, g = rem & 3;
        gb[i] = (int)((int64_t)(n0 + std::min(row, BN - 1)) * rowB + g * 3 + p);
        lb[i] = 3 * PSA + p * PSB + row * 4 + (g ^ ((row >> 2) & 3));
    }
    float4 ra[UA][2];
    u32x4 rb[CB];
    auto load = [&](int kt) {
#pragma unroll
        for (int i = 0; i < UA; i++) {
            ra[i][0] = ga[i][(int64_t)kt * 8];
            ra[i][1] = ga[i][(int64_t)kt * 8 + 1];
        }
#pragma unroll
        for (int i = 0; i < CB; i++) rb[i] = B[gb[i] + kt * CPR];
    };
    auto store = [&](int buf) {
        u32x4 *st = lds + buf * STAGE;
#pragma unroll
        for (int i = 0; i < UA; i++)
            if ((BM * 4) % NT == 0 || i + 1 < UA || tid + i * NT < BM * 4) {
                u32x4 p0, p1, p2;
                split8(ra[i][0], ra[i][1], p0, p1, p2);
                st[la[i]] = p0;
                st[PSA + la[i]] = p1;
                st[2 * PSA + la[i]] = p2;
            }
#pragma unroll
        for (int i = 0; i < CB; i++)
            if ((BN * CPR) % NT == 0 || i + 1 < CB || tid + i * NT < BN * CPR) st[lb[i]] = rb[i];
    };

    f32x16 hi[TM][TN], lo[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; i++)
#pragma unroll
        for (int j = 0; j < TN; j++) {
            hi[i][j] = f32x16{};
            lo[i][j] = f32x16{};
        }

    // fragment reads: row (tile base + lane & 31), chunk (2 kh + (lane >> 5)) XOR ((lane & 31) >> 2) & 3
    const int fr = lane & 31, fh = lane >> 5, fs = (fr >> 2) & 3;
    const int nk = K / BK;
    load(0);
    store(0);
    if (nk > 1) load(1);
    __syncthreads();
    for (int kt = 0; kt < nk; kt++) {
        const int buf = kt & 1;
        if (kt + 1 < nk) store(buf ^ 1);
        if (kt + 2 < nk) load(kt + 2);
        const u32x4 *sAl = lds + buf * STAGE, *sBl = sAl + 3 * PSA;
#pragma unroll
        for (int i = 0; i < TM; i++) {
            u32x4 af[2][3];
#pragma unroll
            for (int kh = 0; kh < 2; kh++)
#pragma unroll
                for (int p = 0; p < 3; p++)
                    af[kh][p] = sAl[p * PSA + (wm * WTM + i * 32 + fr) * 4 + ((2 * kh + fh) ^ fs)];
#pragma unroll
            for (int j = 0; j < TN; j++) {
                u32x4 bf[2][3];
#pragma unroll
                for (int kh = 0; kh < 2; kh++)
#pragma unroll
                    for (int p = 0; p < 3; p++)
                        bf[kh][p] = sBl[p * PSB + (wn * WTN + j * 32 + fr) * 4 + ((2 * kh + fh) ^ fs)];
                if constexpr (ACC == 1) {
                    f32x16 l = lo[i][j], h = hi[i][j];
#pragma unroll
                    for (int kh = 0; kh < 2; kh++) {
                        l = Mfma32::mma(af[kh][2], bf[kh][0], l);
                        l = Mfma32::mma(af[kh][1], bf[kh][1], l);
                        l = Mfma32::mma(af[kh][0], bf[kh][2], l);
                        l = Mfma32::mma(af[kh][1], bf[kh][0], l);
                        l = Mfma32::mma(af[kh][0], bf[kh][1], l);
                        h = Mfma32::mma(af[kh][0], bf[kh][0], h);
                    }
                    lo[i][j] = l;
                    hi[i][j] = h;
                } else {
                    f32x16 c = f32x16{};
#pragma unroll
                    for (int kh = 0; kh < 2; kh++) {
                        c = Mfma32::mma(af[kh][2], bf[kh][0], c);
                        c = Mfma32::mma(af[kh][1], bf[kh][1], c);
                        c = Mfma32::mma(af[kh][0], bf[kh][2], c);
                        c = Mfma32::mma(af[kh][1], bf[kh][0], c);
                        c = Mfma32::mma(af[kh][0], bf[kh][1], c);
                    }
#pragma unroll
                    for (int kh = 0; kh < 2; kh++) c = Mfma32::mma(af[kh][0], bf[kh][0], c);
                    hi[i][j] += c;
                }
            }
        }
        __syncthreads();
    }

    float *Ct = C + t * sC;
#pragma unroll
    for (int j = 0; j < TN; j++) {
        const int col = n0 + wn * WTN + j * 32 + fr;
        const float bv = EPI == 1 ? bias[(int64_t)t * N + col] : 0.0f;
#pragma unroll
        for (int i = 0; i < TM; i++) {
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int64_t row = m0 + wm * WTM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * fh;
                if (row < M) {
                    const float v = ACC == 1 ? hi[i][j][r] + lo[i][j][r] : hi[i][j][r];
                    Ct[row * N + col] = EPI == 1 ? relu_nan(v + bv) : v;
                }
            }
        }
    }
}

template <int BM, int BN, int WGM, int WGN, int EPI>
__global__ __launch_bounds__(64 * WGM * WGN, 2) void k_x6_nt32b(const float4 *__restrict__ A, const u32x4 *__restrict__ B,
                                                                int64_t M, int N, int K, int64_t sA, int64_t sB,
                                                                const float *__restrict__ bias, float *__restrict__ C,
                                                                int64_t sC, int tiles_n) {
    x6_nt_body<Mfma32, 16, false, X6_WALK_B, int, int, BM, BN, WGM, WGN, EPI>(A, B, M, N, K, sA, sB, bias, C, sC,
                                                                              tiles_n);
}

template <int BM, int BN, int WGM, int WGN>
__global__ __launch_bounds__(64 * WGM * WGN) void k_x6_tn32(const void *__restrict__ Av, const void *__restrict__ Bv,
                                                            int64_t Kd, int M, int N, int64_t sA, int64_t sB,
                                                            int64_t kc, int tiles_n, int tiles, int S,
                                                            float *__restrict__ slab) {
    x6_tn_body<Mfma32, BK, true, X6_WALK_IJ, BM, BN, WGM, WGN>(static_cast<const float4 *>(Av),
                                                               static_cast<const float4 *>(Bv), Kd, M, N, sA, sB, kc,
                                                               tiles_n, tiles, S, slab);
}

template <int BM, int BN, int WGM, int WGN>
__global__ __launch_bounds__(64 * WGM * WGN) void k_x6_tn32k16(const float4 *__restrict__ A,
                                                               const float4 *__restrict__ B, int64_t Kd, int M, int N,
                                                               int64_t sA, int64_t sB, int64_t kc, int tiles_n,
                                                               int tiles, int S, float *__restrict__ slab) {
    x6_tn_body<Mfma32, 16, false, X6_WALK_A, BM, BN, WGM, WGN>(A, B, Kd, M, N, sA, sB, kc, tiles_n, tiles, S, slab);
}

template <int BM, int BN, int WGM, int WGN>
hipError_t nt32b_launch(const float4 *A, const u32x4 *B, int64_t M, int N, int K, int T, int64_t sA, int64_t sB,
                        const float *bias, float *C, int64_t sC, hipStream_t s) {
    if (K % 16) return hipErrorInvalidValue;
    // the kernel keeps offsets into a tower's A and B in 32 bits
    if ((M + BM) * (int64_t)(K / 4) > INT32_MAX || (int64_t)N * (K / 8) * 3 > INT32_MAX) return hipErrorInvalidValue;
    return x6_nt_launch<BM, BN, 64 * WGM * WGN>(k_x6_nt32b<BM, BN, WGM, WGN, 1>, k_x6_nt32b<BM, BN, WGM, WGN, 0>, A, B, M,
                                                N, K, T, sA, sB, bias, C, sC, s);
}

template <int BM, int BN, int WGM, int WGN, int ACC>
hipError_t nt32_launch(const float4 *A, const u32x4 *B, int64_t M, int N, int K, int T, int64_t sA, int64_t sB,
                       const float *bias, float *C, int64_t sC, hipStream_t s) {
    // the kernel keeps B's chunk offsets (N * K * 3 / 8) in 32 bits
    if ((int64_t)N * (K / 8) * 3 > INT32_MAX) return hipErrorInvalidValue;
    return x6_nt_launch<BM, BN, 64 * WGM * WGN>(k_x6_nt32<BM, BN, WGM, WGN, 1, ACC>, k_x6_nt32<BM, BN, WGM, WGN, 0, ACC>,
                                                A, B, M, N, K, T, sA, sB, bias, C, sC, s);
}

template <int BM, int BN, int WGM, int WGN, class... Args>
hipError_t tn32_launch(Args... args) {
    return x6_tn_launch<BK, BM, BN, 64 * WGM * WGN>(k_x6_tn32<BM, BN, WGM, WGN>, args...);
}

template <int BM, int BN, int WGM, int WGN, class... Args>
hipError_t tn32k16_launch(Args... args) {
    return x6_tn_launch<16, BM, BN, 64 * WGM * WGN>(k_x6_tn32k16<BM, BN, WGM, WGN>, args...);
}

}  // namespace

// the 32x32x16 weight-gradient kernels (launch_x6_gemm_tn forwards cfg >= 20 here and folds the slabs); the slab
// count actually used comes back in *S_out
hipError_t launch_x6_gemm_tn32(const float *A, const float *B, int64_t Kd, int M, int N, int T, int64_t a_stride,
                               int64_t b_stride, int splits, float *slab, int cfg, hipStream_t s, int *S_out) {
    const int64_t sA = a_stride / 4, sB = b_stride / 4;
    const float4 *a = reinterpret_cast<const float4 *>(A), *b = reinterpret_cast<const float4 *>(B);
    switch (cfg) {
        // 128 x 192 blocks: 8 waves of 32 x 96, or 4 waves (one per SIMD) of 64 x 96
        case 20: return tn32_launch<128, 192, 4, 2>(a, b, Kd, M, N, T, sA, sB, splits, slab, s, S_out);
        case 21: return tn32_launch<128, 192, 2, 2>(a, b, Kd, M, N, T, sA, sB, splits, slab, s, S_out);
        // 256 x 192 blocks, 16-deep k steps, 8 waves of 64 x 96 (k_x6_tn32k16)
        case 24: return tn32k16_launch<256, 192, 4, 2>(a, b, Kd, M, N, T, sA, sB, splits, slab, s, S_out);
        case 25: return tn32k16_launch<256, 192, 8, 1>(a, b, Kd, M, N, T, sA, sB, splits, slab, s, S_out);
        default: return hipErrorInvalidValue;
    }
}

// cfg numbers continue merlin_gemm.hip's (launch_x6_gemm_nt forwards cfg >= 20 here)
hipError_t launch_x6_gemm_nt32(const float *A, const void *B, int64_t M, int N, int K, int T, int64_t a_stride,
                               int64_t b_stride, const float *bias, float *C, int64_t c_stride, int cfg,
                               hipStream_t s) {
    const float4 *a = reinterpret_cast<const float4 *>(A);
    const u32x4 *b = static_cast<const u32x4 *>(B);
    const int64_t sA = a_stride / 4, sB = b_stride / 8 * 3;
    switch (cfg) {
        // k_x6_nt32b: 16-deep k steps, 4 waves, two blocks per CU (forward 256 x 128, input gradient 128 x 192)
        case 26: return nt32b_launch<256, 128, 2, 2>(a, b, M, N, K, T, sA, sB, bias, C, c_stride, s);
        case 27: return nt32b_launch<128, 192, 2, 2>(a, b, M, N, K, T, sA, sB, bias, C, c_stride, s);
        case 28: return nt32b_launch<128, 128, 2, 2>(a, b, M, N, K, T, sA, sB, bias, C, c_stride, s);
        // forward shape (N = 512): 256 x 128 blocks, 8 waves of 64 x 64
        case 20: return nt32_launch<256, 128, 4, 2, 1>(a, b, M, N, K, T, sA, sB, bias, C, c_stride, s);
        case 21: return nt32_launch<256, 128, 4, 2, 0>(a, b, M, N, K, T, sA, sB, bias, C, c_stride, s);
        // input-gradient shape (N = 576): 128 x 192 blocks, 8 waves of 32 x 96
        case 22: return nt32_launch<128, 192, 4, 2, 1>(a, b, M, N, K, T, sA, sB, bias, C, c_stride, s);
        case 23: return nt32_launch<128, 192, 4, 2, 0>(a, b, M, N, K, T, sA, sB, bias, C, c_stride, s);
        // 256 x 128 over 4 waves (1 per SIMD) of 128 x 64
        case 24: return nt32_launch<256, 128, 2, 2, 1>(a, b, M, N, K, T, sA, sB, bias, C, c_stride, s);
        // 128 x 128, 4 waves of 64 x 64 (2 blocks per CU)
        case 25: return nt32_launch<128, 128, 2, 2, 1>(a, b, M, N, K, T, sA, sB, bias, C, c_stride, s);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace merlin
