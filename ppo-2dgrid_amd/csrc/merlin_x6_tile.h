// merlin_x6_tile.h -- what the six three-plane ("x6") GEMM bodies of merlin_gemm.hip and merlin_gemm2.hip share: the
// vector types, the two bf16 MFMA shapes, the fp32 operand stager that splits while it stages, the stager of ready
// planes, the two-stage pipeline, the six-product step with its walk over a wave's tiles, the epilogue, the two
// bodies (x6_nt_body, x6_tn_body) and their launches.  A kernel of the two files picks an MFMA shape, a k depth, an
// accumulate form, a walk and how its stagers hold addresses.  Users: k_x6_nt, k_x6_nt32b, k_x6_tn32, k_x6_tn32k16.
// k_x6_tn (merlin_gemm.hip) and k_x6_nt32 (merlin_gemm2.hip) hold kernels that fc1 selects, ran 1.6-2 % slower on
// the shared bodies and keep their own text (their comments say more); they take the types, split8, tr_swz and mma.
//
// LDS holds every operand as three plane images (merlin_x6.h), one 16-B chunk per group of 8 values.  An NT image
// is [tile rows][G = k depth / 8 groups], group g of row r at chunk r G + (g ^ x6_nt_swz(r)); a TN image is [k rows]
// [RC = tile columns / 8 groups], group g of k row r at r RC + (g ^ tr_swz(r)), read back transposed.
#pragma once
#include <algorithm>

#include "merlin_internal.h"
#include "merlin_x6.h"

namespace merlin {
namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;
typedef __attribute__((address_space(3))) char lds_char;

constexpr int BK = 32;   // k per step of the 32-deep bodies: 4 groups of 8
constexpr int CPR = 12;  // 16-B plane chunks per row and 32 values of k (4 groups x 3 planes)

// ---------------------------------------------------------------------------------------------------------------
// The MFMA shapes: E x E tiles over K values of k per instruction.  Element r of a tile's accumulator in lane l is
// row (r & 3) + 8 (r >> 2) + 4 (l / E), column l % E (x6_store); an operand fragment is row l % E, values
// 8 (l / E) .. + 7 of the instruction's K (x6_nt_frag, x6_tr_frag).  tr_swz: the TN images' swizzle (x6_tn_body).
struct Mfma16 {  // v_mfma_f32_16x16x32_bf16
    static constexpr int E = 16, K = 32;
    typedef f32x4 Acc;
    static __device__ __forceinline__ Acc mma(const u32x4 a, const u32x4 b, Acc c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b),
                                                       c, 0, 0, 0);
    }
    // a 32-lane half of a transposed read (rows r..r+3 and r+8..r+11, two adjacent chunks each) hits 16 distinct
    // 16-B bank slots (rows of 16k chunks or of 16k + 8 chunks)
    template <int RC>
    static __device__ __forceinline__ int tr_swz(int row) {
        static_assert(RC % 8 == 0, "row chunks");
        if constexpr (RC % 16 == 0)
            return ((row & 3) << 1) | (((row >> 3) & 1) << 3);
        else
            return (((row >> 1) & 1) << 1) | (((row >> 3) & 1) << 2);
    }
};
struct Mfma32 {  // v_mfma_f32_32x32x16_bf16: twice the work per instruction for the same issue hold
    static constexpr int E = 32, K = 16;
    typedef f32x16 Acc;
    static __device__ __forceinline__ Acc mma(const u32x4 a, const u32x4 b, Acc c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b),
                                                       c, 0, 0, 0);
    }
    // a 32-lane half reads 4 rows x 4 adjacent chunks: 16 distinct 16-B bank slots for RC = 16 (XOR by 4 (r & 3))
    // and RC = 24 (row stride 24 = 8 mod 16 separates odd rows; XOR by 4 ((r >> 1) & 1))
    template <int RC>
    static __device__ __forceinline__ int tr_swz(int row) {
        static_assert(RC % 16 == 0 || RC == 24, "row chunks");
        return RC % 16 == 0 ? (row & 3) << 2 : ((row >> 1) & 1) << 2;
    }
};

// NT images: rows of G = 4 chunks (64 B) XOR (row >> 2) & 3, rows of G = 2 chunks XOR (row >> 3) & 1: the
// ds_read_b128 fragment reads of each lane group and the staging writes hit 16 distinct 16-B bank slots
template <int G>
__device__ __forceinline__ int x6_nt_swz(int row) {
    static_assert(G == 4 || G == 2, "k steps of 32 or 16");
    return G == 4 ? (row >> 2) & 3 : (row >> 3) & 1;
}
// the fragment of rows row0 .. + E - 1 (row0 a multiple of E, so the swizzle is the lane's), k half kh of the step,
// from the image `plane` chunks behind img: the constant goes on last, where it folds into the read's offset field
template <class P, int G>
__device__ __forceinline__ u32x4 x6_nt_frag(const u32x4 *img, int row0, int kh, int lane, int plane) {
    const int fr = lane % P::E, g = kh * (P::K / 8) + lane / P::E;
    return (img + ((row0 + fr) * G + (g ^ x6_nt_swz<G>(fr))))[plane];
}
// TN images come out k-contiguous through ds_read_b64_tr_b16 (the hardware transposed read): the fragment of columns
// col0 .. + E - 1, k rows K kh .. + K - 1 is two reads, 16-lane group g taking columns 16 (g % (E / 16)) .. + 15 and
// k rows 8 (g / (E / 16)) + 4 h2 .. + 3
template <class P, int RC>
__device__ __forceinline__ u32x4 x6_tr_frag(const u32x4 *img, int col0, int kh, int lane) {
    constexpr int CH = P::E / 16;
    const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
    const int chunk = ((col0 + 16 * (g % CH)) >> 3) + (p >> 1);
    bf16x4 v[2];
#pragma unroll
    for (int h2 = 0; h2 < 2; h2++) {
        const int row = P::K * kh + 8 * (g / CH) + 4 * h2 + q;
        const int off = (row * RC + (chunk ^ P::template tr_swz<RC>(row))) * 16 + (p & 1) * 8;
        v[h2] = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4 *)((lds_char *)img + off));
    }
    return __builtin_bit_cast(u32x4, bf16x8{v[0][0], v[0][1], v[0][2], v[0][3], v[1][0], v[1][1], v[1][2], v[1][3]});
}

// ---------------------------------------------------------------------------------------------------------------
// Staging.  A stager keeps per unit an address -- AT: a pointer, or a 32-bit offset from the operand's base where
// the launcher has checked that the operand fits (fewer address registers) -- and reads base + a wave-uniform step
// offset: no per-lane 64-bit arithmetic at the loads, whose temporaries made the compiler park the loaded values
// in other registers (a wait right behind every load).
template <class T>
__device__ __forceinline__ void x6_addr(const T *&a, const T *base, int64_t off) { a = base + off; }
template <class T>
__device__ __forceinline__ void x6_addr(int &a, const T *, int64_t off) { a = (int)off; }
template <class T>
__device__ __forceinline__ const T *x6_src(const T *a, const T *, int64_t d) { return a + d; }
template <class T>
__device__ __forceinline__ const T *x6_src(int a, const T *base, int64_t d) { return base + (a + (int)d); }

// 8 fp32 values -> their three planes as 16-B fragment chunks
__device__ __forceinline__ void split8(const float4 a, const float4 b, u32x4 &p0, u32x4 &p1, u32x4 &p2) {
    uint2 x[3], y[3];
    x6_split4(a, x);
    x6_split4(b, y);
    p0 = u32x4{x[0].x, x[0].y, y[0].x, y[0].y};
    p1 = u32x4{x[1].x, x[1].y, y[1].x, y[1].y};
    p2 = u32x4{x[2].x, x[2].y, y[2].x, y[2].y};
}
__device__ __forceinline__ void split8(const f32x4 a, const f32x4 b, u32x4 &p0, u32x4 &p1, u32x4 &p2) {
    split8(make_float4(a[0], a[1], a[2], a[3]), make_float4(b[0], b[1], b[2], b[3]), p0, p1, p2);
}

// An fp32 operand (4 bytes per value from HBM / L2 instead of the planes' 6), split in registers while it is staged:
// images of ROWS rows x G groups, plane p at p Q chunks.  Unit q < Q of a step is group q % G of image row q / G;
// NT's A takes a tile row per image row (src_row clamps it to M - 1), TN's operands a k row.
template <int NT, int ROWS, int G, class AT = const float4 *>
struct X6Split {
    static constexpr int Q = ROWS * G, U = (Q + NT - 1) / NT;
    const float4 *base;
    int64_t rowlen;  // float4s per source row
    int tid;
    AT at[U];
    int kr[U], o[U], l[U];  // image row, float4 within the source row, LDS chunk
    f32x4 r[U][2];  // as native vectors: one 16-B load each, whatever the optimiser makes of the branches around them

    template <class SWZ, class ROW>
    __device__ __forceinline__ void init(int tid_, const float4 *base_, int64_t rowlen_, SWZ swz, ROW src_row) {
        base = base_, rowlen = rowlen_, tid = tid_;
#pragma unroll
        for (int i = 0; i < U; i++) {
            const int q = std::min(tid + i * NT, Q - 1);
            const int row = q / G, g = q - (q / G) * G;
            kr[i] = row;
            o[i] = g * 2;
            l[i] = row * G + (g ^ swz(row));
            x6_addr(at[i], base, (int64_t)src_row(row) * rowlen + g * 2);
        }
    }
    // the step d float4s behind the units' addresses
    __device__ __forceinline__ void load(int64_t d) {
#pragma unroll
        for (int i = 0; i < U; i++) {
            const f32x4 *src = reinterpret_cast<const f32x4 *>(x6_src(at[i], base, d));
            r[i][0] = src[0];
            r[i][1] = src[1];
        }
    }
    // TN, a split's last step, source rows kk + kr: rows past k1 re-read row k1 - 1 and are zeroed when staged -- a
    // select here would make the wave wait for the loads right after issuing them
    __device__ __forceinline__ void load_last(int64_t kk, int64_t k1) {
#pragma unroll
        for (int i = 0; i < U; i++) {
            const f32x4 *src = reinterpret_cast<const f32x4 *>(base + std::min(kk + kr[i], k1 - 1) * rowlen + o[i]);
            r[i][0] = src[0];
            r[i][1] = src[1];
        }
    }
    // the loaded step (source rows kk + kr) into the images at st; rows from k1 on stage as zero
    __device__ __forceinline__ void store(u32x4 *st, int64_t kk = 0, int64_t k1 = INT64_MAX) const {
        const f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int i = 0; i < U; i++)
            if (Q % NT == 0 || i + 1 < U || tid + i * NT < Q) {
                const bool in = kk + kr[i] < k1;
                u32x4 p0, p1, p2;
                split8(in ? r[i][0] : zero, in ? r[i][1] : zero, p0, p1, p2);
                st[l[i]] = p0;
                st[Q + l[i]] = p1;
                st[2 * Q + l[i]] = p2;
            }
    }
};

// NT's B: ready planes [N][K/8][3][8] (the weights, small and re-read by every tile, split once per call), a chunk per
// unit.  G = 4: plane p at p PS chunks with PS = 4 BN + 12 -- the pad and the unit order (planes major within a row)
// keep the staging writes conflict-free as well.  G = 2 (k_x6_nt32b): no pad, groups major.
template <int NT, int BN, int G, class AT>
struct X6Planes {
    static constexpr int RQ = 3 * G;  // chunks per row and step
    static constexpr int Q = BN * RQ, U = (Q + NT - 1) / NT, PS = G == 4 ? BN * 4 + 12 : BN * 2;
    const u32x4 *base;
    int tid;
    AT at[U];
    int l[U];
    u32x4 r[U];

    // rows n0 .. + BN - 1 of B, rowlen chunks per row
    __device__ __forceinline__ void init(int tid_, const u32x4 *base_, int n0, int64_t rowlen) {
        base = base_, tid = tid_;
#pragma unroll
        for (int i = 0; i < U; i++) {
            const int q = std::min(tid + i * NT, Q - 1);
            const int row = q / RQ, rem = q - (q / RQ) * RQ;
            const int p = G == 4 ? rem / G : rem % 3, g = G == 4 ? rem % G : rem / 3;
            x6_addr(at[i], base, (int64_t)(n0 + row) * rowlen + g * 3 + p);
            l[i] = p * PS + row * G + (g ^ x6_nt_swz<G>(row));
        }
    }
    __device__ __forceinline__ void load(int kt) {
#pragma unroll
        for (int i = 0; i < U; i++) r[i] = *x6_src(at[i], base, (int64_t)kt * RQ);
    }
    __device__ __forceinline__ void store(u32x4 *st) const {
#pragma unroll
        for (int i = 0; i < U; i++)
            if (Q % NT == 0 || i + 1 < U || tid + i * NT < Q) st[l[i]] = r[i];
    }
};

// Two LDS stages, one barrier per k step, the step after next in flight in registers: load(kt) reads step kt from
// memory, store(buf, kt) stages the loaded step kt, compute(buf) is the body's MFMAs on a staged step.  Step 0 is
// loaded and staged whatever nk is, so a caller needs nk >= 1 or a load that is safe without it: the NT kernels have
// always read step 0 unguarded (their callers pass K >= 32); in TN x6_tn_launch recomputes the split count so that no
// split is empty, and a ragged load clamps its rows to k1 - 1 >= 0 even if one were.
template <class LOAD, class STORE, class COMPUTE>
__device__ __forceinline__ void x6_pipeline(int nk, LOAD load, STORE store, COMPUTE compute) {
    load(0);
    store(0, 0);
    if (nk > 1) load(1);
    __syncthreads();
    for (int kt = 0; kt < nk; kt++) {
        const int buf = kt & 1;
        if (kt + 1 < nk) store(buf ^ 1, kt + 1);
        if (kt + 2 < nk) load(kt + 2);
        compute(buf);
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------------------
// One tile's k step: the six plane products with i + j <= 2 of each of the step's KH MFMA k halves (the three left
// out are below 2^-24 |a b| together; every bf16 x bf16 product is exact in fp32), smallest first, so that the five
// small ones never round at the running sum's scale -- the error of a blocked fp32 sum, which the weight gradient's
// long, cancelling sums need.  Two forms:
//   chunk (SPLIT false): the step's products in a fresh accumulator (the small ones of every half, then the a0 b0),
//     added to the running sum hi with one rounding;
//   SPLIT: a0 b0 into hi, the small ones into lo, hi + lo once in the epilogue: no per-step adds, twice the registers.
template <class P, int KH, bool SPLIT>
__device__ __forceinline__ void x6_mma6(typename P::Acc &hi, typename P::Acc &lo, const u32x4 (&a)[KH][3],
                                        const u32x4 (&b)[KH][3]) {
    if constexpr (SPLIT) {
        typename P::Acc l = lo, h = hi;
#pragma unroll
        for (int kh = 0; kh < KH; kh++) {
            l = P::mma(a[kh][2], b[kh][0], l);
            l = P::mma(a[kh][1], b[kh][1], l);
            l = P::mma(a[kh][0], b[kh][2], l);
            l = P::mma(a[kh][1], b[kh][0], l);
            l = P::mma(a[kh][0], b[kh][1], l);
            h = P::mma(a[kh][0], b[kh][0], h);
        }
        lo = l;
        hi = h;
    } else {
        typename P::Acc c = {};
#pragma unroll
        for (int kh = 0; kh < KH; kh++) {
            c = P::mma(a[kh][2], b[kh][0], c);
            c = P::mma(a[kh][1], b[kh][1], c);
            c = P::mma(a[kh][0], b[kh][2], c);
            c = P::mma(a[kh][1], b[kh][0], c);
            c = P::mma(a[kh][0], b[kh][1], c);
        }
#pragma unroll
        for (int kh = 0; kh < KH; kh++) c = P::mma(a[kh][0], b[kh][0], c);
        hi += c;
    }
}

template <int KH, class F>
__device__ __forceinline__ void x6_frags(F f, int t, u32x4 (&x)[KH][3]) {
#pragma unroll
    for (int kh = 0; kh < KH; kh++)
#pragma unroll
        for (int p = 0; p < 3; p++) x[kh][p] = f(t, kh, p);
}

// A wave's TM x TN tiles over one staged step; fa(i, kh, p) / fb(j, kh, p) read plane p's fragment of tile row i /
// tile column j.  The walk says which fragments stay in registers: A's (B's read once per tile column), B's (A's once
// per tile row), or neither (tile rows outside, B's fragments read again for every one).
enum { X6_WALK_A, X6_WALK_B, X6_WALK_IJ };

template <class P, int KH, bool SPLIT, int WALK, int TM, int TN, class FA, class FB>
__device__ __forceinline__ void x6_step(typename P::Acc (&hi)[TM][TN], typename P::Acc (&lo)[TM][TN], FA fa, FB fb) {
    if constexpr (WALK == X6_WALK_A) {
        u32x4 af[TM][KH][3];
#pragma unroll
        for (int i = 0; i < TM; i++) x6_frags<KH>(fa, i, af[i]);
#pragma unroll
        for (int j = 0; j < TN; j++) {
            u32x4 bf[KH][3];
            x6_frags<KH>(fb, j, bf);
#pragma unroll
            for (int i = 0; i < TM; i++) x6_mma6<P, KH, SPLIT>(hi[i][j], lo[i][j], af[i], bf);
        }
    } else if constexpr (WALK == X6_WALK_B) {
        u32x4 bf[TN][KH][3];
#pragma unroll
        for (int j = 0; j < TN; j++) x6_frags<KH>(fb, j, bf[j]);
#pragma unroll
        for (int i = 0; i < TM; i++) {
            u32x4 af[KH][3];
            x6_frags<KH>(fa, i, af);
#pragma unroll
            for (int j = 0; j < TN; j++) x6_mma6<P, KH, SPLIT>(hi[i][j], lo[i][j], af, bf[j]);
        }
    } else {
#pragma unroll
        for (int i = 0; i < TM; i++) {
            u32x4 af[KH][3];
            x6_frags<KH>(fa, i, af);
#pragma unroll
            for (int j = 0; j < TN; j++) {
                u32x4 bf[KH][3];
                x6_frags<KH>(fb, j, bf);
                x6_mma6<P, KH, SPLIT>(hi[i][j], lo[i][j], af, bf);
            }
        }
    }
}

// The wave's tiles to C: rows row0 + E i + ..., columns col0 + E j (col0 the lane's column of tile column 0); EPI 1:
// relu(. + bias[column]).  FULL: every row of the tile exists (a TN slab); otherwise rows from M on are not written.
template <class P, bool SPLIT, int EPI, bool FULL, int TM, int TN>
__device__ __forceinline__ void x6_store(const typename P::Acc (&hi)[TM][TN], const typename P::Acc (&lo)[TM][TN],
                                         float *Ct, const float *bias, int N, int64_t M, int64_t row0, int col0,
                                         int lane) {
#pragma unroll
    for (int j = 0; j < TN; j++) {
        const int col = col0 + j * P::E;
        const float bv = EPI == 1 ? bias[col] : 0.0f;
#pragma unroll
        for (int i = 0; i < TM; i++) {
#pragma unroll
            for (int r = 0; r < P::E * P::E / 64; r++) {
                const int64_t row = row0 + i * P::E + (r & 3) + 8 * (r >> 2) + 4 * (lane / P::E);
                if (FULL || row < M) {
                    const float v = SPLIT ? hi[i][j][r] + lo[i][j][r] : hi[i][j][r];
                    Ct[row * N + col] = EPI == 1 ? relu_nan(v + bv) : v;
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// NT: C[t][m][n] = epi(sum_k A[t][m][k] B[t][n][k]); A fp32 [M][K], B x6 planes [N][K/8][3][8] (K % KS == 0,
// N % BN == 0); EPI 1: relu(. + bias[t][n]).  grid (tiles_m * tiles_n, T), each XCD a contiguous run of tiles: the
// BN-column tiles of one BM-row panel run back to back on one L2.  Block tile BM x BN over WGM x WGN waves, k steps
// of KS.
template <class P, int KS, bool SPLIT, int WALK, class ATA, class ATB, int BM, int BN, int WGM, int WGN, int EPI>
__device__ __forceinline__ void x6_nt_body(const float4 *__restrict__ A, const u32x4 *__restrict__ B, int64_t M, int N,
                                           int K, int64_t sA, int64_t sB, const float *__restrict__ bias,
                                           float *__restrict__ C, int64_t sC, int tiles_n) {
    constexpr int NT = 64 * WGM * WGN;
    constexpr int WTM = BM / WGM, WTN = BN / WGN;
    constexpr int TM = WTM / P::E, TN = WTN / P::E, G = KS / 8;
    static_assert(WTM % P::E == 0 && WTN % P::E == 0 && KS % P::K == 0, "wave tile and k step of whole MFMA tiles");
    typedef X6Split<NT, BM, G, ATA> SA;
    typedef X6Planes<NT, BN, G, ATB> SB;
    constexpr int PSA = SA::Q, PSB = SB::PS;
    constexpr int STAGE = 3 * (PSA + PSB);
    __shared__ u32x4 lds[2 * STAGE];

    const int t = blockIdx.y;
    const int L = xcd_tile(blockIdx.x, gridDim.x);
    const int tm = L / tiles_n, tn = L - tm * tiles_n;
    const int64_t m0 = (int64_t)tm * BM;
    const int n0 = tn * BN;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int wm = w / WGN, wn = w - (w / WGN) * WGN;

    SA sa;
    SB sb;
    sa.init(
        tid, A + t * sA, K / 4, [](int row) { return x6_nt_swz<G>(row); },
        [&](int row) { return std::min<int64_t>(m0 + row, M - 1); });
    sb.init(tid, B + t * sB, n0, (int64_t)(K / 8) * 3);

    typename P::Acc hi[TM][TN], lo[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; i++)
#pragma unroll
        for (int j = 0; j < TN; j++) {
            hi[i][j] = typename P::Acc{};
            lo[i][j] = typename P::Acc{};
        }

    x6_pipeline(
        K / KS,
        [&](int kt) {
            sa.load((int64_t)kt * (KS / 4));
            sb.load(kt);
        },
        [&](int buf, int) {
            u32x4 *st = lds + buf * STAGE;
            sa.store(st);
            sb.store(st + 3 * PSA);
        },
        [&](int buf) {
            const u32x4 *sAl = lds + buf * STAGE, *sBl = sAl + 3 * PSA;
            x6_step<P, KS / P::K, SPLIT, WALK>(
                hi, lo, [&](int i, int kh, int p) { return x6_nt_frag<P, G>(sAl, wm * WTM + i * P::E, kh, lane, p * PSA); },
                [&](int j, int kh, int p) { return x6_nt_frag<P, G>(sBl, wn * WTN + j * P::E, kh, lane, p * PSB); });
        });

    x6_store<P, SPLIT, EPI, false>(hi, lo, C + t * sC, EPI == 1 ? bias + (int64_t)t * N : nullptr, N, M, m0 + wm * WTM,
                                   n0 + wn * WTN + lane % P::E, lane);
}

// TN: slab[s][t][m][n] = sum_{k in [s kc, min(Kd, (s + 1) kc))} A[t][k][m] B[t][k][n]; A fp32 [Kd][M], B fp32 [Kd][N],
// both row-major over the long reduction dimension k (the weight gradient dz^T a3 over the minibatch's frames);
// M % BM == 0, N % BN == 0, kc % KS == 0.  1-D grid over (tower, split, tile), tile fastest, XCD-contiguous: the
// tiles of one split read the same k rows of both operands, so they run together on one L2.  Both operands go
// through the same stager; every step of a split but its last is whole.
template <class P, int KS, bool SPLIT, int WALK, int BM, int BN, int WGM, int WGN>
__device__ __forceinline__ void x6_tn_body(const float4 *__restrict__ A, const float4 *__restrict__ B, int64_t Kd,
                                           int M, int N, int64_t sA, int64_t sB, int64_t kc, int tiles_n, int tiles,
                                           int S, float *__restrict__ slab) {
    constexpr int NT = 64 * WGM * WGN;
    constexpr int WTM = BM / WGM, WTN = BN / WGN;
    constexpr int TM = WTM / P::E, TN = WTN / P::E;
    constexpr int RCA = BM / 8, RCB = BN / 8;
    static_assert(WTM % P::E == 0 && WTN % P::E == 0 && KS % P::K == 0, "wave tile and k step of whole MFMA tiles");
    typedef X6Split<NT, KS, RCA> SA;
    typedef X6Split<NT, KS, RCB> SB;
    constexpr int PSA = SA::Q, PSB = SB::Q;
    constexpr int STAGE = 3 * (PSA + PSB);
    __shared__ u32x4 lds[2 * STAGE];

    const int b = xcd_tile(blockIdx.x, gridDim.x);
    const int t = b / (S * tiles), s = (b / tiles) % S, L = b % tiles;
    const int tm = L / tiles_n, tn = L - tm * tiles_n;
    const int m0 = tm * BM, n0 = tn * BN;
    const int64_t k0 = (int64_t)s * kc, k1 = std::min<int64_t>(Kd, k0 + kc);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int wm = w / WGN, wn = w - (w / WGN) * WGN;

    SA sa;
    SB sb;
    const auto src_row = [&](int row) { return k0 + row; };
    sa.init(tid, A + t * sA + m0 / 4, M / 4, [](int row) { return P::template tr_swz<RCA>(row); }, src_row);
    sb.init(tid, B + t * sB + n0 / 4, N / 4, [](int row) { return P::template tr_swz<RCB>(row); }, src_row);

    typename P::Acc hi[TM][TN], lo[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; i++)
#pragma unroll
        for (int j = 0; j < TN; j++) {
            hi[i][j] = typename P::Acc{};
            lo[i][j] = typename P::Acc{};
        }

    x6_pipeline(
        (int)((k1 - k0 + KS - 1) / KS),
        [&](int kt) {
            const int64_t d = (int64_t)kt * KS;
            if (k0 + d + KS <= k1) {
                sa.load(d * sa.rowlen);
                sb.load(d * sb.rowlen);
            } else {
                sa.load_last(k0 + d, k1);
                sb.load_last(k0 + d, k1);
            }
        },
        [&](int buf, int kt) {
            u32x4 *st = lds + buf * STAGE;
            const int64_t kk = k0 + (int64_t)kt * KS;
            sa.store(st, kk, k1);
            sb.store(st + 3 * PSA, kk, k1);
        },
        [&](int buf) {
            const u32x4 *sAl = lds + buf * STAGE, *sBl = sAl + 3 * PSA;
            x6_step<P, KS / P::K, SPLIT, WALK>(
                hi, lo, [&](int i, int kh, int p) { return x6_tr_frag<P, RCA>(sAl + p * PSA, wm * WTM + i * P::E, kh, lane); },
                [&](int j, int kh, int p) { return x6_tr_frag<P, RCB>(sBl + p * PSB, wn * WTN + j * P::E, kh, lane); });
        });

    float *St = slab + ((int64_t)s * (gridDim.x / (S * tiles)) + t) * (int64_t)M * N;
    x6_store<P, SPLIT, 0, true>(hi, lo, St, nullptr, N, 0, m0 + wm * WTM, n0 + wn * WTN + lane % P::E, lane);
}

// ---------------------------------------------------------------------------------------------------------------
// Host side.  An NT launch: with_bias / plain are the kernel's EPI 1 / 0 instantiations.
template <int BM, int BN, int THREADS, class KB, class KP>
hipError_t x6_nt_launch(KB with_bias, KP plain, const float4 *A, const u32x4 *B, int64_t M, int N, int K, int T,
                        int64_t sA, int64_t sB, const float *bias, float *C, int64_t sC, hipStream_t s) {
    if (N % BN) return hipErrorInvalidValue;
    const int64_t tiles_m = (M + BM - 1) / BM;
    const int tiles_n = N / BN;
    if (tiles_m * tiles_n > INT32_MAX) return hipErrorInvalidValue;
    const dim3 grid((unsigned)(tiles_m * tiles_n), T);
    if (bias)
        hipLaunchKernelGGL(with_bias, grid, dim3(THREADS), 0, s, A, B, M, N, K, sA, sB, bias, C, sC, tiles_n);
    else
        hipLaunchKernelGGL(plain, grid, dim3(THREADS), 0, s, A, B, M, N, K, sA, sB, (const float *)nullptr, C, sC,
                           tiles_n);
    return hipGetLastError();
}

// A TN launch into the slabs (launch_x6_gemm_tn folds them): the k range in `splits` slabs of kc rows, kc rounded up
// to the body's k depth KS and the slab count recomputed so that none is empty; it comes back in *S_out
template <int KS, int BM, int BN, int THREADS, class KERN>
hipError_t x6_tn_launch(KERN kern, const float4 *A, const float4 *B, int64_t Kd, int M, int N, int T, int64_t sA,
                        int64_t sB, int splits, float *slab, hipStream_t s, int *S_out) {
    if (M % BM || N % BN) return hipErrorInvalidValue;
    const int tiles_n = N / BN, tiles = (M / BM) * tiles_n;
    int S = std::max(1, splits);
    int64_t kc = (Kd + S - 1) / S;
    kc = (kc + KS - 1) / KS * KS;
    S = (int)std::max<int64_t>(1, (Kd + kc - 1) / kc);
    *S_out = S;
    hipLaunchKernelGGL(kern, dim3(tiles * S * T), dim3(THREADS), 0, s, A, B, Kd, M, N, sA, sB, kc, tiles_n, tiles, S,
                       slab);
    return hipGetLastError();
}

}  // namespace
}  // namespace merlin
