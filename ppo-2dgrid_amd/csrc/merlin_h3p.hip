// merlin_h3p.hip -- fc1's NT GEMM with BOTH operands already in h3 plane form (round 5): no split in the kernel,
// both operands staged by LDS-DMA three k steps deep, the LDS fragment reads interleaved with the MFMAs.
//
// Why hand-placed waits (profiles/r05a_probe_h3_planes.log, the .s of k_h3_ntg): with the fragment reads as plain
// loads, hipcc waited lgkmcnt(0) before the first MFMA of every other half step -- the MFMAs' operands came from
// reads issued after the previous barrier, and the wait also covered the reads issued for the next half -- so the
// matrix pipe drained for an LDS round trip twice per k step.  Ablations of that kernel at the update's shape: 505
// us with everything, 400 us with no DMA in the loop, 384 us for the DMA stream alone.
//
// Here every half step is 3 TM TN MFMAs (TM x TN tiles of 32x32x16 x {hi, lo, lo}) with the 2 (TM + TN) fragment
// reads of the next half interleaved one per MFMA (sched_group_barrier), and the k loop is unrolled (one
// instantiation per K), so the compiler's lgkmcnt waits are exact counts: the reads of a half are waited for once,
// by the first MFMA that needs them (the MFMAs still in the pipe cover it).
//
// Layouts as merlin_h3.hip's k_h3_ntg: operand rows of K/8 groups x (hi, lo) x 8 f16 (h3_split), a k step (32
// values) = 8 16-B chunks per row; LDS image rows of 8 chunks, chunk c of row r at slot c ^ g_swz(r)
// (merlin_h3_tile.h), the permutation applied to the DMA's global source address (a DMA writes lane-linear).
// The accumulator tile with its epilogues (H3Tile) and the TN kernel's transposed fragment read come from
// merlin_h3_tile.h, shared with merlin_h3.hip's TN body.
#include <algorithm>

#include "merlin_h3_tile.h"
#include "merlin_internal.h"

namespace merlin {
namespace {

// the vector types, mfma16, g_swz, IC, the accumulator tile H3Tile and the TN fragment read: merlin_h3_tile.h
// a lo plane fragment (8 f16 at 2^11 x their value) back at scale: v_pk_mul_f16 x 4, exact unless the result is
// subnormal (then rounded to the f16 subnormal grid, 2^-24)
__device__ __forceinline__ u32x4 p_unscale(const u32x4 x) {
    return __builtin_bit_cast(u32x4, __builtin_bit_cast(f16x8, x) * (_Float16)H3_LO_INV);
}

template <int N, int I = 0, class F>
__device__ __forceinline__ void static_for(F &&f) {
    if constexpr (I < N) {
        f(IC<I>{});
        static_for<N, I + 1>(f);
    }
}

typedef __attribute__((address_space(3))) u32x4 lds_u32x4;
// one 16-B LDS fragment read (a plain load: the k loop is unrolled, so the compiler's waits are exact counts)
__device__ __forceinline__ void lds_rd(u32x4 &d, uint32_t addr) { d = *(const lds_u32x4 *)(uintptr_t)addr; }

// ---------------------------------------------------------------------------------------------------------------
// What the four NT bodies below (pq_tile, pqg_tile, pq_walk, pqg_walk) share besides the accumulator tile and its
// epilogues (H3Tile, merlin_h3_tile.h): the fragment reads and MFMAs of a half step over a staged k step.  A body
// keeps what is its own: where its DMAs read, its ring schedule and its waits.
// ONE (round 6): one accumulator per tile -- the lo planes (stored 2^11 up) brought back to scale in registers
// (v_pk_mul_f16 by 2^-11: exact while the result stays normal, f16 subnormals kept) so all three products of a k
// step add into the same fp32 accumulator: half the accumulator registers, hence twice the tile area per byte staged.
// Not the same bits as the two-accumulator kernels (a different summation); its error is held to float64 by
// tests/test_gpu_h3.py like theirs.
// ORD: the order of a half step's MFMAs, see mf.
template <int BM, int BN, int WGM, int WGN, bool ONE = false, int ORD = 0>
struct PCore : H3Tile<BM, BN, WGM, WGN, ONE> {
    using TL = H3Tile<BM, BN, WGM, WGN, ONE>;
    using TL::hi;
    using TL::lo;
    static constexpr int NT = TL::NT, WTM = TL::WTM, WTN = TL::WTN, TM = TL::TM, TN = TL::TN;
    static constexpr int NR = 2 * (TM + TN), NM = 3 * TM * TN;  // fragment reads / MFMAs per half step
    static_assert(NM >= NR, "a read behind every MFMA");
    static constexpr int GA = BM * 8 / NT, GB = BN * 8 / NT, G = GA + GB;  // DMA instructions per thread and k step
    static_assert((BM * 8) % NT == 0 && (BN * 8) % NT == 0, "whole DMA instructions per thread");
    static constexpr int STG = (BM + BN) * 8;  // chunks per stage
    static constexpr uint32_t STG_B = STG * 16;
    static constexpr int CS = TM * TN * 16;  // C stores per wave and tile

    struct Frag {
        u32x4 a[TM][2], b[TN][2];  // [tile][plane]
    };
    // fragment addresses (bytes, stage 0): A tile i / B tile j at half kh, plane p -> row r, chunk 2 (2 kh + fh) + p
    uint32_t adA[2][2], adB[2][2];  // [kh][p], tile 0; tile i is +32 i rows (same swizzle)

    __device__ __forceinline__ void init(uint32_t lds0, int wm, int wn, int fr, int fh) {
        const int ra = wm * WTM + fr, rb = BM + wn * WTN + fr;
#pragma unroll
        for (int kh = 0; kh < 2; kh++)
#pragma unroll
            for (int p = 0; p < 2; p++) {
                const int c = 2 * (2 * kh + fh) + p;
                adA[kh][p] = lds0 + (uint32_t)(ra * 8 + (c ^ g_swz(ra))) * 16u;
                adB[kh][p] = lds0 + (uint32_t)(rb * 8 + (c ^ g_swz(rb))) * 16u;
            }
        this->zero();
    }
    // the k-th of the NR fragment reads of half KH of the stage at byte offset so into g (k, KH compile-time: no
    // runtime-indexed fragment arrays)
    template <class K_, class KH>
    __device__ __forceinline__ void rd(Frag &g, K_, uint32_t so, KH) const {
        constexpr int k = K_::value, kh = KH::value;
        if constexpr (k < 2 * TM)
            lds_rd(g.a[k >> 1][k & 1], adA[kh][k & 1] + so + (k >> 1) * 32 * 128);
        else
            lds_rd(g.b[(k - 2 * TM) >> 1][k & 1], adB[kh][k & 1] + so + ((k - 2 * TM) >> 1) * 32 * 128);
    }
    // MFMA m: tile (i, j), product pr -- ORD 0: a tile's three products back to back (m / 3 = tile, m % 3 = pr);
    // ORD 1: product-major (every tile's pr 0, then every tile's pr 1, ...), so consecutive MFMAs never share an
    // accumulator; each accumulator still sums the same products in the same order (the same bits)
    template <class M_>
    __device__ __forceinline__ void mf(const Frag &f, const Frag &u, M_) {
        constexpr int m = M_::value, tl = ORD ? m % (TM * TN) : m / 3, pr = ORD ? m / (TM * TN) : m % 3;
        constexpr int i = tl / TN, j = tl % TN;
        if constexpr (ONE) {  // u: f's lo planes at scale
            if constexpr (pr == 0)
                hi[i][j] = mfma16(u.a[i][1], f.b[j][0], hi[i][j]);
            else if constexpr (pr == 1)
                hi[i][j] = mfma16(f.a[i][0], u.b[j][1], hi[i][j]);
            else
                hi[i][j] = mfma16(f.a[i][0], f.b[j][0], hi[i][j]);
        } else if constexpr (pr == 0)
            lo[i][j] = mfma16(f.a[i][1], f.b[j][0], lo[i][j]);
        else if constexpr (pr == 1)
            lo[i][j] = mfma16(f.a[i][0], f.b[j][1], lo[i][j]);
        else
            hi[i][j] = mfma16(f.a[i][0], f.b[j][0], hi[i][j]);
    }
    // half step: the NM MFMAs on f, with the NR reads of g (stage offset so, half KH) one behind each of the first NR
    // (sched_group_barrier: MFMA, read, MFMA, read, ...), so the reads of a half are waited for once, by the first
    // MFMA that needs them, with the MFMAs still in the pipe covering the LDS round trip (the file's header)
    template <class KH, class READS>
    __device__ __forceinline__ void half(const Frag &f, Frag &g, uint32_t so, KH kh, READS) {
        Frag u;
        if constexpr (ONE) {
#pragma unroll
            for (int i = 0; i < TM; i++) u.a[i][1] = p_unscale(f.a[i][1]);
#pragma unroll
            for (int j = 0; j < TN; j++) u.b[j][1] = p_unscale(f.b[j][1]);
        }
        static_for<NM>([&](auto M_) __attribute__((always_inline)) {
            mf(f, u, M_);
            if constexpr (READS::value && decltype(M_)::value < NR) rd(g, M_, so, kh);
        });
        if constexpr (READS::value) {
            static_for<NR>([&](auto) __attribute__((always_inline)) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
            });
            if constexpr (NM > NR) __builtin_amdgcn_sched_group_barrier(0x008, NM - NR, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    // makes the compiler's wait for the reads of f fall here: before the barrier that follows, not behind it in front
    // of the first MFMA of the next half
    static __device__ __forceinline__ void touch(const Frag &f) {
#pragma unroll
        for (int i = 0; i < TM; i++) asm volatile("" ::"v"(f.a[i][0]), "v"(f.a[i][1]));
#pragma unroll
        for (int j = 0; j < TN; j++) asm volatile("" ::"v"(f.b[j][0]), "v"(f.b[j][1]));
    }
    // behind a body's own vmcnt wait: every wave's DMAs up to that count are in LDS, and no LDS read moves above
    static __device__ __forceinline__ void publish() {
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
    }
};

// NS: LDS stages of the DMA ring (NS - 1 k steps in flight).  3: 120 KB at 128 x 192; 4 (round 6): 160 KB, the whole
// LDS of a CU -- a step's DMA is latency-bound (~2.5 us under load against ~1.2 us of MFMA work per step), so the
// feed rate per CU is the bytes in flight over that latency
// (pq_tile: the body of k_h3_pq's one-tile form, a block per tile; the kernel and its persistent form are defined
// behind the walks, at the end of this namespace)
template <int BM, int BN, int WGM, int WGN, int EPI, int NK, int NS, bool ONE, int ORD>
__device__ __forceinline__ void pq_tile(const u32x4 *__restrict__ A, const u32x4 *__restrict__ B,
                                        const uint32_t *__restrict__ amaxA, const uint32_t *__restrict__ amaxB,
                                        int64_t M, int N, int K, int64_t sA, int64_t sB,
                                        const float *__restrict__ bias, float *__restrict__ C, int64_t sC,
                                        int tiles_n) {
    using P = PCore<BM, BN, WGM, WGN, ONE, ORD>;
    using Frag = typename P::Frag;
    constexpr int NT = P::NT, WTM = P::WTM, WTN = P::WTN, TN = P::TN, NR = P::NR, G = P::G, STG = P::STG;
    constexpr uint32_t STG_B = P::STG_B;
    static_assert(NS >= 2 && NS <= 4, "ring depth");
    __shared__ u32x4 lds[NS * STG];

    const int t = blockIdx.y;
    const int L = xcd_tile(blockIdx.x, gridDim.x);
    const int tm = L / tiles_n, tn = L - tm * tiles_n;
    const int64_t m0 = (int64_t)tm * BM;
    const int n0 = tn * BN;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int wm = w / WGN, wn = w - (w / WGN) * WGN;
    const int64_t row_ch = K / 4;  // chunks per operand row (4 B per value, planes)

    // the scales first: an ordinary load consumed after a DMA is issued makes the compiler wait for the DMA too
    const int eA = h3_exp(load_amax(amaxA + t)), eB = h3_exp(load_amax(amaxB + t));
    // DMA sources as 32-bit chunk offsets from the uniform row-block bases (6 VGPRs, not 6 64-bit pointers): A's
    // block rows m0.. and B's n0.. (the last A rows clamped to M - 1: read, never stored)
    const u32x4 *baseA = A + t * sA + m0 * row_ch, *baseB = B + t * sB + (int64_t)n0 * row_ch;
    uint32_t off[G];
#pragma unroll
    for (int i = 0; i < G; i++) {
        const int q = i * NT + tid, r = q >> 3, c = (q & 7) ^ g_swz(r);
        off[i] = r < BM ? (uint32_t)(std::min<int64_t>(r, M - 1 - m0) * row_ch + c) : (uint32_t)((r - BM) * row_ch + c);
    }
    typedef __attribute__((address_space(3))) void lds_void;
    typedef __attribute__((address_space(1))) void gbl_void;
    auto issue = [&](int kt, int st) __attribute__((always_inline)) {
        u32x4 *base = lds + st * STG + w * 64;
#pragma unroll
        for (int i = 0; i < G; i++) {
            const int q0 = i * NT;  // instruction-uniform: which operand
            const u32x4 *b = (q0 >> 3) < BM ? baseA : baseB;
            __builtin_amdgcn_global_load_lds((gbl_void *)(b + off[i] + kt * 8), (lds_void *)(base + i * NT), 16, 0, 0);
        }
    };

    const int fr = lane & 31, fh = lane >> 5;
    const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) u32x4 *)lds;
    P c;
    c.init(lds0, wm, wn, fr, fh);

    static_assert(NK >= NS - 1, "the prologue's k steps");
    constexpr int D = NS - 1;  // k steps in flight
    static_for<D>([&](auto KT) __attribute__((always_inline)) { issue(decltype(KT)::value, decltype(KT)::value); });
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(G * (D - 1)) : "memory");  // step 0 landed
    P::publish();
    Frag f0, f1;
    static_for<NR>([&](auto K_) __attribute__((always_inline)) { c.rd(f0, K_, 0, IC<0>{}); });
    static_for<NK>([&](auto KT) __attribute__((always_inline)) {
        constexpr int kt = decltype(KT)::value, st = kt % NS, sn = (kt + 1) % NS;
        if constexpr (kt + D < NK) issue(kt + D, (kt + D) % NS);  // the stage read in step kt - 1
        __builtin_amdgcn_sched_barrier(0);
        c.half(f0, f1, (uint32_t)st * STG_B, IC<1>{}, IC<1>{});  // MFMAs of half 0, reads of half 1
        if constexpr (kt + 1 < NK) {
            P::touch(f1);  // the compiler's wait for f1 here, before the barrier
            // step kt + 1 landed: the steps issued after it (up to kt + D, those that exist) may stay in flight
            constexpr int later = (NK - 1 < kt + D ? NK - 1 : kt + D) - (kt + 1);
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(G * later) : "memory");
            P::publish();  // step kt + 1 published; every wave is past its reads of step kt - 1
            c.half(f1, f0, (uint32_t)sn * STG_B, IC<0>{}, IC<1>{});  // MFMAs of half 1, reads of the next half 0
        } else {
            c.half(f1, f0, 0u, IC<0>{}, IC<0>{});
        }
    });

    // (the epilogue's loads by static_for: behind a loop that does not use the accumulators the optimiser would move
    // the hi MFMAs of every k step, which nothing in the k steps reads, out of the schedule above to this place)
    const int col0 = n0 + wn * WTN + fr;
    float bv[TN];
    static_for<TN>([&](auto J) __attribute__((always_inline)) {
        bv[decltype(J)::value] = EPI == 1 ? bias[(int64_t)t * N + col0 + decltype(J)::value * 32] : 0.0f;
    });
    c.store(IC<0>{}, IC<EPI>{}, C + t * sC, N, M, m0, wm * WTM + 4 * fh, col0, pow2f(-eA), pow2f(-eB), bv);
}

// ---------------------------------------------------------------------------------------------------------------
// TN over plane operands with LDS-DMA staging (round 5; the weight gradient dz^T a3, merlin_h3_gemm_tn_gather_planes
// with cfg 20): slab[s][t][m][n] = sum over the split's rows k of A[t][k][m] B[t][k][n], A planes [Kd][M/8][2][8]
// (k_head_bwd's dz), B planes gathered by 64-column chunks (row k's chunk j is row bmap[k * N / 64 + j] of B seen
// as [*][64]: conv3's representatives).  The LDS images are h3_tn_body's (merlin_h3_tile.h) -- per operand and plane
// [32 k rows][RC chunks of 8 columns], chunk c of row r at c ^ tr_swz(r), fragments k-contiguous through
// ds_read_b64_tr_b16 (tr_off / tr_read / tr_pack) -- but filled by
// DMA three k steps deep: a DMA writes its 64 lanes' 16-B chunks lane-linear, so each lane's source is the chunk
// whose image slot that is (the swizzle and the plane deinterleave are in the source addresses).  B's chunk rows
// come from bmap through a 3-slot LDS ring, itself filled by DMA four steps ahead, so the data DMA's addresses need
// no global load in the loop.  Rows past the split's end read a zero chunk; a split's step count is padded to a
// multiple of three (the ring's period: compile-time stages) with such steps.
// The DMAs are inline asm (s_mov_b32 m0 + global_load_lds_*): issued through the builtin, hipcc treats every LDS read
// that follows as possibly aliasing an in-flight DMA and waits vmcnt(0) before the first fragment read of each step
// (profiles/r05 .s of the first version), which serialises the pipeline; here the waits are all explicit: vmcnt
// counts this wave's DMAs in issue order and the barrier after each wait publishes every wave's.
// Same products in the same order as k_h3_tn / k_h3_tng: the same bits.
__device__ uint4 p_zero16[1] = {{0u, 0u, 0u, 0u}};

// m0 is a reserved register to LLVM (a clobber entry is ignored, with a warning), so the asm saves it in a scratch
// SGPR and puts it back behind the DMA: the compiler's view of m0 is unchanged by these statements whatever it keeps
// there.  (The DMA reads m0 at issue: the compiler's own code rewrites m0 right behind each global_load_lds too.)
__device__ __forceinline__ void p_dma16(const void *src, uint32_t lds) {  // lds: wave-uniform byte address
    uint32_t keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(src), "s"(lds)
                 : "memory");
}
__device__ __forceinline__ void p_dma4(const void *src, uint32_t lds) {
    uint32_t keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\tglobal_load_lds_dword %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(src), "s"(lds)
                 : "memory");
}

typedef __attribute__((address_space(3))) int32_t lds_i32;

template <int BM, int BN, int WGM, int WGN>
__global__ __launch_bounds__(64 * WGM * WGN) void k_h3_tq(const u32x4 *__restrict__ A, const u32x4 *__restrict__ B,
                                                          const uint32_t *__restrict__ amaxA,
                                                          const uint32_t *__restrict__ amaxB, int64_t Kd, int M,
                                                          int N, int64_t sA, int64_t sB, int64_t kc, int tiles_n,
                                                          int tiles, int S, float *__restrict__ slab,
                                                          const int32_t *__restrict__ bmap) {
    using TL = H3Tile<BM, BN, WGM, WGN>;
    constexpr int NT = TL::NT, NW = NT / 64, WTM = TL::WTM, WTN = TL::WTN, TM = TL::TM, TN = TL::TN;
    constexpr int RCA = BM / 8, RCB = BN / 8;
    constexpr int PSA = 32 * RCA, PSB = 32 * RCB;  // chunks per plane image
    constexpr int STG = 2 * (PSA + PSB);
    constexpr uint32_t STG_B = STG * 16;
    static_assert((2 * PSA) % NT == 0 && (2 * PSB) % NT == 0, "whole DMA instructions per operand");
    constexpr int GA = 2 * PSA / NT, GB = 2 * PSB / NT, G = GA + GB + 1;  // + the index DMA
    constexpr int JB = BN / 64;   // 64-column chunks of B per tile (bmap entries per row)
    constexpr int XS = 64 * NW;   // index ring slot (ints; 32 * JB used)
    static_assert(32 * JB <= XS, "index slot");
    constexpr int NF = 2 * (TM + TN);             // fragments per half step (tiles x planes)
    constexpr int NR = 2 * NF, NM = 3 * TM * TN;  // tr reads (two per fragment) / MFMAs per half step
    __shared__ u32x4 lds[3 * STG];
    __shared__ int32_t ixr[3 * XS];

    const int P = xcd_tile(blockIdx.x, gridDim.x);
    const int t = P / (S * tiles), s = (P / tiles) % S, Lt = P % tiles;
    const int tm = Lt / tiles_n, tn = Lt - tm * tiles_n;
    const int m0 = tm * BM, n0 = tn * BN;
    const int64_t k0 = (int64_t)s * kc, k1 = std::min<int64_t>(Kd, k0 + kc);
    const int eA = h3_exp(load_amax(amaxA + t)), eB = h3_exp(load_amax(amaxB + t));
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int wm = w / WGN, wn = w - (w / WGN) * WGN;
    const int nc = N / 64, j0 = n0 / 64;
    const int64_t rowA = M / 4;  // chunks per A row
    const u32x4 *At = A + t * sA, *Bt = B + t * sB;
    const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) u32x4 *)lds;
    const uint32_t ix0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) int32_t *)ixr;
    const uint32_t wbase = (uint32_t)__builtin_amdgcn_readfirstlane(w) * 64u;  // the wave's first slot

    // the thread's DMA slots: A (instructions 0 .. GA-1): row ra, chunk offset oa; B: row rb, ring entry xb, offset gp
    int ra[GA], rb[GB], xb[GB];
    uint32_t oa[GA], gp[GB];
#pragma unroll
    for (int i = 0; i < GA; i++) {
        const int q = i * NT + tid, p = q / PSA, rem = q - p * PSA, r = rem / RCA, cs = rem - r * RCA;
        const int c = cs ^ tr_swz<RCA>(r);
        ra[i] = r;
        oa[i] = (uint32_t)((m0 / 8 + c) * 2 + p);
    }
#pragma unroll
    for (int i = 0; i < GB; i++) {
        const int q = (GA + i) * NT + tid - 2 * PSA, p = q / PSB, rem = q - p * PSB, r = rem / RCB,
                  cs = rem - r * RCB;
        const int c = cs ^ tr_swz<RCB>(r), col = 8 * c;
        rb[i] = r;
        xb[i] = r * JB + (col >> 6);
        gp[i] = (uint32_t)(((col & 63) >> 3) * 2 + p);
    }
    // the index DMA: this thread's ring entry e = tid (< 32 JB used): row e / JB, chunk j0 + e % JB
    const int xr = tid / JB, xj = j0 + tid % JB;
    const int64_t nk = (k1 - k0 + 31) / 32, nk3 = (nk + 2) / 3 * 3;

    auto issue_ix = [&](int64_t kt, int slot) __attribute__((always_inline)) {
        const int64_t row = std::min<int64_t>(k0 + kt * 32 + (tid < 32 * JB ? xr : 0), k1 - 1);
        p_dma4(bmap + row * nc + (tid < 32 * JB ? xj : j0), ix0 + (uint32_t)(slot * XS) * 4u + wbase * 4u);
    };
    // this thread's chunk rows of a step from its index slot (read a step before they are used)
    auto read_ix = [&](int slot, int32_t (&x)[GB]) __attribute__((always_inline)) {
        const lds_i32 *xs = (const lds_i32 *)(uintptr_t)(ix0 + (uint32_t)(slot * XS) * 4u);
#pragma unroll
        for (int i = 0; i < GB; i++) x[i] = xs[xb[i]];
    };
    auto issue = [&](int64_t kt, int st, const int32_t (&x)[GB]) __attribute__((always_inline)) {
        const uint32_t base = lds0 + (uint32_t)(st * STG) * 16u + wbase * 16u;
        const int64_t kk = k0 + kt * 32;
        const bool full = kk + 32 <= k1;  // block-uniform
#pragma unroll
        for (int i = 0; i < GA; i++) {
            const u32x4 *src = full || kk + ra[i] < k1 ? At + (kk + ra[i]) * rowA + oa[i]
                                                          : reinterpret_cast<const u32x4 *>(p_zero16);
            p_dma16(src, base + (uint32_t)(i * NT) * 16u);
        }
#pragma unroll
        for (int i = 0; i < GB; i++) {
            const u32x4 *src = full || kk + rb[i] < k1 ? Bt + (int64_t)x[i] * 16 + gp[i]
                                                          : reinterpret_cast<const u32x4 *>(p_zero16);
            p_dma16(src, base + (uint32_t)((GA + i) * NT) * 16u);
        }
    };

    // fragment reads: fragment f < NF (A tiles x planes, then B tiles x planes), its two transposed halves
    struct Frag {
        bf16x4 v[NF][2];
    };
    auto rd = [&](Frag &g, auto K_, uint32_t so, auto KH) __attribute__((always_inline)) {
        constexpr int k = decltype(K_)::value, kh = decltype(KH)::value, f = k >> 1, h2 = k & 1;
        constexpr bool isA = f < 2 * TM;
        constexpr int tile = isA ? f >> 1 : (f - 2 * TM) >> 1, pl = f & 1;
        constexpr int RC = isA ? RCA : RCB;
        const int col0 = isA ? wm * WTM + tile * 32 : wn * WTN + tile * 32;
        const uint32_t img = lds0 + so + (uint32_t)(isA ? pl * PSA : 2 * PSA + pl * PSB) * 16u;
        g.v[f][h2] = tr_read((const lds_char *)(uintptr_t)(img + (uint32_t)tr_off<RC>(col0, kh, h2, lane)));
    };
    auto frag = [](const Frag &g, int f) __attribute__((always_inline)) { return tr_pack(g.v[f][0], g.v[f][1]); };
    TL c;
    c.zero();
    // MFMA m of a half step: tile (i, j) = (m / (3 TN), (m / 3) % TN), product m % 3 (k_h3_tn's order per tile)
    auto mf = [&](const Frag &f, auto M_) __attribute__((always_inline)) {
        constexpr int m = decltype(M_)::value, i = m / (3 * TN), j = (m / 3) % TN, pr = m % 3;
        constexpr int fa0 = 2 * i, fa1 = 2 * i + 1, fb0 = 2 * TM + 2 * j, fb1 = 2 * TM + 2 * j + 1;
        if constexpr (pr == 0)
            c.lo[i][j] = mfma16(frag(f, fa1), frag(f, fb0), c.lo[i][j]);
        else if constexpr (pr == 1)
            c.lo[i][j] = mfma16(frag(f, fa0), frag(f, fb1), c.lo[i][j]);
        else
            c.hi[i][j] = mfma16(frag(f, fa0), frag(f, fb0), c.hi[i][j]);
    };
    constexpr int RPM = (NR + NM - 1) / NM;  // reads behind each MFMA
    auto half = [&](const Frag &f, Frag &g, uint32_t so, auto KH) __attribute__((always_inline)) {
        static_for<NM>([&](auto M_) __attribute__((always_inline)) {
            mf(f, M_);
            static_for<RPM>([&](auto R_) __attribute__((always_inline)) {
                constexpr int k = decltype(M_)::value * RPM + decltype(R_)::value;
                if constexpr (k < NR) rd(g, IC<k>{}, so, KH);
            });
        });
        static_for<NM>([&](auto M_) __attribute__((always_inline)) {
            constexpr int left = NR - decltype(M_)::value * RPM;
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            if constexpr (left > 0) __builtin_amdgcn_sched_group_barrier(0x100, left < RPM ? left : RPM, 0);
        });
        __builtin_amdgcn_sched_barrier(0);
    };
    auto touch = [&](const Frag &f) __attribute__((always_inline)) {
#pragma unroll
        for (int q = 0; q < NF; q++) asm volatile("" ::"v"(f.v[q][0]), "v"(f.v[q][1]));
    };
    auto publish = [&](auto CNT) __attribute__((always_inline)) {  // this wave's DMAs but the last CNT landed, then
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(decltype(CNT)::value) : "memory");  // every wave's
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
    };

    // prologue: indices of steps 0..2 (slot = step % 3); DMA of steps 0 and 1; once every wave has read slot 0, the
    // indices of step 3 into it
    int32_t x0[GB], x1[GB], x2[GB];  // chunk rows of the steps issued next (step k's in x[k % 3])
    issue_ix(0, 0);
    issue_ix(1, 1);
    issue_ix(2, 2);
    publish(IC<0>{});
    read_ix(0, x0);
    read_ix(1, x1);
    read_ix(2, x2);
    issue(0, 0, x0);
    issue(1, 1, x1);
    publish(IC<G - 1>{});  // DMA 0 landed (DMA 1 may not); every wave has read slots 0 .. 2
    issue_ix(3, 0);
    Frag f0, f1;
    static_for<NR>([&](auto K_) __attribute__((always_inline)) { rd(f0, K_, 0u, IC<0>{}); });
    // step kt (stage st = kt % 3): the indices of kt + 4 (slot (kt + 1) % 3, last read at step kt - 1), the DMA of
    // kt + 2 (stage (kt + 2) % 3, its chunk rows read a step ago), half 0, publish kt + 1 (the two DMA groups just
    // issued may stay in flight; the indices of kt + 3 have landed), read those, half 1
    auto step = [&](int64_t kt, auto ST, int32_t (&xu)[GB], int32_t (&xn)[GB]) __attribute__((always_inline)) {
        constexpr int st = decltype(ST)::value, sn = (st + 1) % 3, s2 = (st + 2) % 3;
        issue_ix(kt + 4, sn);
        issue(kt + 2, s2, xu);
        __builtin_amdgcn_sched_barrier(0);
        half(f0, f1, (uint32_t)st * STG_B, IC<1>{});
        touch(f1);
        publish(IC<G>{});
        read_ix(st, xn);  // slot st = (kt + 3) % 3
        half(f1, f0, (uint32_t)sn * STG_B, IC<0>{});
    };
    for (int64_t kt = 0; kt < nk3; kt += 3) {
        step(kt, IC<0>{}, x2, x0);
        step(kt + 1, IC<1>{}, x0, x1);
        step(kt + 2, IC<2>{}, x1, x2);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the padded steps' DMAs drained before the block ends

    // the slab: the plain epilogue, every row present (M % BM == 0: the launcher checks)
    const float bv[TN] = {};
    c.store(IC<1>{}, IC<0>{}, slab + ((int64_t)s * (gridDim.x / (S * tiles)) + t) * (int64_t)M * N, N, M, m0,
            wm * WTM + 4 * (lane >> 5), n0 + wn * WTN + (lane & 31), pow2f(-eA), pow2f(-eB), bv);
}


// ---------------------------------------------------------------------------------------------------------------
// The update's forward over a3's planes with the rows gathered (round 5; merlin_h3_gemm_nt_heads_planes cfg 60):
// k_h3_pq's schedule (LDS-DMA three steps deep, K = 576 unrolled, fragment reads under the MFMAs) with A's rows read
// through the row map by 64-value chunks -- row m's chunk j is row amap[m * 9 + j] of A seen as [*][64] (conv3's
// patch representatives) -- and k_h3_ntp's epilogues (EPI 1 bias + ReLU; EPI 2 the same plus the policy / value
// heads' partial dot products, merlin_heads_combine's layout).  The block's 9 BM chunk rows are read into LDS once;
// a step's A sources are read from there one step ahead.  DMAs by inline asm as in k_h3_tq (no compiler-inserted
// vmcnt before LDS reads).  The same products in the same order as k_h3_ntpg: the same bits.
// (pqg_tile: the body of k_h3_pqg's one-tile form)
template <int BM, int BN, int WGM, int WGN, int EPI>
__device__ __forceinline__ void pqg_tile(const u32x4 *__restrict__ A, const u32x4 *__restrict__ B,
                                         const uint32_t *__restrict__ amaxA, const uint32_t *__restrict__ amaxB,
                                         int64_t M, int N, int64_t sA, int64_t sB, const float *__restrict__ bias,
                                         float *__restrict__ C, int64_t sC, int tiles_n,
                                         const int32_t *__restrict__ amap, const float *__restrict__ hw0,
                                         const float *__restrict__ hw1, int na, float *__restrict__ hpart) {
    constexpr int K = 576, NK = 18, KC = K / 64;
    using P = PCore<BM, BN, WGM, WGN>;
    using Frag = typename P::Frag;
    constexpr int NT = P::NT, WTM = P::WTM, WTN = P::WTN, TN = P::TN, NR = P::NR, GA = P::GA, GB = P::GB, G = P::G;
    constexpr int STG = P::STG;
    constexpr uint32_t STG_B = P::STG_B;
    __shared__ u32x4 lds[3 * STG];
    __shared__ int32_t gmap[BM * KC];

    const int t = blockIdx.y;
    const int L = xcd_tile(blockIdx.x, gridDim.x);
    const int tm = L / tiles_n, tn = L - tm * tiles_n;
    const int64_t m0 = (int64_t)tm * BM;
    const int n0 = tn * BN;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int wm = w / WGN, wn = w - (w / WGN) * WGN;
    const int eA = h3_exp(load_amax(amaxA + t)), eB = h3_exp(load_amax(amaxB + t));
    for (int e = tid; e < BM * KC; e += NT) {
        const int r = e / KC;
        gmap[e] = amap[std::min<int64_t>(m0 + r, M - 1) * KC + (e - r * KC)];
    }
    __syncthreads();
    const u32x4 *At = A + t * sA, *baseB = B + t * sB + (int64_t)n0 * (K / 4);
    int ga[GA];       // gmap entry base r * KC of the thread's A slots
    uint32_t ca[GA];  // their chunk within a k step
    uint32_t offB[GB];
#pragma unroll
    for (int i = 0; i < GA; i++) {
        const int q = i * NT + tid, r = q >> 3;
        ga[i] = r * KC;
        ca[i] = (uint32_t)((q & 7) ^ g_swz(r));
    }
#pragma unroll
    for (int i = 0; i < GB; i++) {
        const int q = i * NT + tid, r = q >> 3;
        offB[i] = (uint32_t)(r * (K / 4) + ((q & 7) ^ g_swz(r)));
    }
    const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) u32x4 *)lds;
    const uint32_t gm0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) int32_t *)gmap;
    const uint32_t wbase = (uint32_t)__builtin_amdgcn_readfirstlane(w) * 64u;
    // the chunk rows of step kt's A slots (plain LDS loads, read a step ahead of their issue)
    auto read_g = [&](int kt, int32_t (&g)[GA]) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < GA; i++) g[i] = *(const lds_i32 *)(uintptr_t)(gm0 + (uint32_t)(ga[i] + kt / 2) * 4u);
    };
    auto issue = [&](int kt, int st, const int32_t (&g)[GA]) __attribute__((always_inline)) {
        const uint32_t base = lds0 + (uint32_t)(st * STG) * 16u + wbase * 16u;
#pragma unroll
        for (int i = 0; i < GA; i++)
            p_dma16(At + (int64_t)g[i] * 16 + 8 * (kt & 1) + ca[i], base + (uint32_t)(i * NT) * 16u);
#pragma unroll
        for (int i = 0; i < GB; i++) p_dma16(baseB + offB[i] + kt * 8, base + (uint32_t)((GA + i) * NT) * 16u);
    };

    const int fr = lane & 31, fh = lane >> 5;
    P c;
    c.init(lds0, wm, wn, fr, fh);

    int32_t g0[GA], g1[GA];  // chunk rows of the next issue (ping-pong, compile-time choice)
    read_g(0, g0);
    issue(0, 0, g0);
    read_g(1, g1);
    issue(1, 1, g1);
    read_g(2, g0);
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(G) : "memory");
    P::publish();
    Frag f0, f1;
    static_for<NR>([&](auto K_) __attribute__((always_inline)) { c.rd(f0, K_, 0, IC<0>{}); });
    static_for<NK>([&](auto KT) __attribute__((always_inline)) {
        constexpr int kt = decltype(KT)::value, st = kt % 3, sn = (kt + 1) % 3;
        int32_t(&gu)[GA] = (kt % 2 == 0) ? g0 : g1;  // holds step kt + 2's rows
        int32_t(&gn)[GA] = (kt % 2 == 0) ? g1 : g0;
        if constexpr (kt + 2 < NK) issue(kt + 2, (kt + 2) % 3, gu);
        __builtin_amdgcn_sched_barrier(0);
        c.half(f0, f1, (uint32_t)st * STG_B, IC<1>{}, IC<1>{});
        if constexpr (kt + 1 < NK) {
            P::touch(f1);
            if constexpr (kt + 2 < NK)
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"(G) : "memory");
            else
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            P::publish();
            if constexpr (kt + 3 < NK) read_g(kt + 3, gn);
            c.half(f1, f0, (uint32_t)sn * STG_B, IC<0>{}, IC<1>{});
        } else {
            c.half(f1, f0, 0u, IC<0>{}, IC<0>{});
        }
    });

    const float inv = pow2f(-eA), invB = pow2f(-eB);
    float *Ct = C + t * sC;
    const int col0 = n0 + wn * WTN + fr, rw = wm * WTM + 4 * fh;
    float bv[TN];
    static_for<TN>([&](auto J) __attribute__((always_inline)) {
        bv[decltype(J)::value] = EPI >= 1 ? bias[(int64_t)t * N + col0 + decltype(J)::value * 32] : 0.0f;
    });
    if constexpr (EPI == 2) {
        const float *hw = t == 0 ? hw0 : hw1;
        const int nh = t == 0 ? na : 1;
        float wv[4][TN];
        static_for<4 * TN>([&](auto Q) __attribute__((always_inline)) {
            constexpr int j = decltype(Q)::value / 4, o = decltype(Q)::value % 4;
            // loaded unconditionally (row clamped into [0, nh)): no load behind a branch
            const float x = hw[(int64_t)(o < nh ? o : 0) * N + col0 + j * 32];
            wv[o][j] = o < nh ? x : 0.0f;
        });
        float *part = hpart + ((int64_t)(t * tiles_n + tn) * WGN + wn) * M * 4;
        c.store_heads(IC<0>{}, IC<2>{}, Ct, part, N, M, m0, rw, rw, col0, fr, inv, invB, bv, wv);
    } else {
        c.store(IC<0>{}, IC<EPI>{}, Ct, N, M, m0, rw, col0, inv, invB, bv);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Persistent forms of the two NT kernels above (k_h3_pq / k_h3_pqg with PERS): at most one block per CU, each
// walking a static list of (tower, tile) items -- item xcd_tile(b + i gridDim.x, T x tiles) of the tower-major
// list for block b's i-th tile, so the blocks of one XCD still work on neighbouring tiles at the same time.  No
// block talks to another: no counters, nothing to spin on.
// The DMA ring runs on across tile boundaries: the last two k steps of a tile issue the first two of the block's
// next tile (the block's last tile fetches its own first steps again, so that every count below is static; they
// are drained before the block ends), then the tile's C stores go out, then step 2 of the next tile is issued.
// vmcnt retires in issue order, so the wait for step 1 (issued before the stores) lets the stores and step 2 stay
// in flight; the wait for step 2, a k step later, is the first that needs the stores gone.  The stores' count
// must be exact for that, so only a tile whose rows all exist stores unconditionally and carries them into the
// next tile; a ragged tile stores under its row test and drains (one tile in ~900).
// Scales, bias and head weights are plain loads, and hipcc's own wait for a plain load also waits for every DMA
// issued before it: they are loaded before the first DMA and again only when the tower / column tile of the item
// changes (with an explicit drain).  Per output element the same products in the same order and the same epilogue
// arithmetic as the one-tile forms: the same bits.
#define P_VMCNT(n) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(n) : "memory")
// DMA with a uniform 64-bit base and a 32-bit byte offset per lane (no immediate: the instruction's offset field moves
// the LDS address as well as the global one, so a k step's 128 B x kt goes into the base by scalar adds)
__device__ __forceinline__ void p_dma16s(const void *sbase, uint32_t voff, uint32_t lds) {
    uint32_t keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(voff), "s"(sbase), "s"(lds)
                 : "memory");
}
__device__ __forceinline__ void p_dma4s(const void *sbase, uint32_t voff, uint32_t lds) {
    uint32_t keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\tglobal_load_lds_dword %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(voff), "s"(sbase), "s"(lds)
                 : "memory");
}
// every counter but vmcnt left alone (gfx9 encoding: vmcnt 0, expcnt 7, lgkmcnt 15): a wait the compiler sees
__device__ __forceinline__ void p_drain_loads() { __builtin_amdgcn_s_waitcnt(0x0F70); }

struct PItem {
    int t, n0, tn;
    int64_t m0;
};
__device__ __forceinline__ PItem p_item(int v, int W, int tiles, int tiles_n, int BM, int BN) {
    const int it = xcd_tile(v, W), t = it / tiles, L = it - t * tiles, tm = L / tiles_n, tn = L - tm * tiles_n;
    return PItem{t, tn * BN, tn, (int64_t)tm * BM};
}

template <int BM, int BN, int WGM, int WGN, int EPI, int NK, int ORD>
__device__ __forceinline__ void pq_walk(const u32x4 *__restrict__ A, const u32x4 *__restrict__ B,
                                        const uint32_t *__restrict__ amaxA, const uint32_t *__restrict__ amaxB,
                                        int64_t M, int N, int K, int64_t sA, int64_t sB,
                                        const float *__restrict__ bias, float *__restrict__ C, int64_t sC,
                                        int tiles_n, int tiles, int W) {
    using P = PCore<BM, BN, WGM, WGN, false, ORD>;
    using Frag = typename P::Frag;
    constexpr int NT = P::NT, WTM = P::WTM, WTN = P::WTN, TN = P::TN, NR = P::NR, GA = P::GA, GB = P::GB, G = P::G;
    constexpr int STG = P::STG;
    constexpr uint32_t STG_B = P::STG_B;
    constexpr int S = P::CS;                        // C stores per wave and tile
    constexpr int CARRY = S + G < 63 ? S + G : 63;  // the vmcnt field's largest value
    const int N_ = N;
    static_assert(NK >= 4, "the look-ahead's k steps");
    __shared__ u32x4 lds[3 * STG];

    int v = blockIdx.x;
    const int nb = gridDim.x;
    if (v >= W) return;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int wm = w / WGN, wn = w - (w / WGN) * WGN;
    const int64_t row_ch = K / 4;
    const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) u32x4 *)lds;
    const uint32_t wbase = (uint32_t)__builtin_amdgcn_readfirstlane(w) * 64u * 16u;

    PItem cur = p_item(v, W, tiles, tiles_n, BM, BN);
    // the epilogue's constants of the item they were loaded for
    int lt = cur.t, ln = cur.n0;
    int eA = h3_exp(load_amax(amaxA + lt)), eB = h3_exp(load_amax(amaxB + lt));
    float bvv[TN];
    const int fr = lane & 31, fh = lane >> 5;
#pragma unroll
    for (int j = 0; j < TN; j++) bvv[j] = EPI == 1 ? bias[(int64_t)lt * N + ln + wn * WTN + j * 32 + fr] : 0.0f;
    p_drain_loads();

    uint32_t offA[GA], offB[GB];  // byte offsets from the item's uniform row-block bases
    auto set_offA = [&](const PItem &it) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < GA; i++) {
            const int q = i * NT + tid, r = q >> 3, c = (q & 7) ^ g_swz(r);
            offA[i] = (uint32_t)(std::min<int64_t>(r, M - 1 - it.m0) * row_ch + c) * 16u;
        }
    };
#pragma unroll
    for (int i = 0; i < GB; i++) {
        const int q = (GA + i) * NT + tid, r = q >> 3, c = (q & 7) ^ g_swz(r);
        offB[i] = (uint32_t)((r - BM) * row_ch + c) * 16u;
    }
    const u32x4 *bA, *bB;  // the item the DMAs are issued for
    auto set_base = [&](const PItem &it) __attribute__((always_inline)) {
        bA = A + it.t * sA + it.m0 * row_ch;
        bB = B + it.t * sB + (int64_t)it.n0 * row_ch;
        set_offA(it);
    };
    // logical stage s (k step kt's is kt % 3) -> byte offset of the physical stage: NK % 3 stages on per tile
    uint32_t sv[3] = {0u, STG_B, 2u * STG_B};
    auto issue = [&](auto KT, uint32_t so) __attribute__((always_inline)) {
        constexpr int kt = decltype(KT)::value;
        const uint32_t base = lds0 + so + wbase;
#pragma unroll
        for (int i = 0; i < GA; i++) p_dma16s(bA + kt * 8, offA[i], base + (uint32_t)(i * NT) * 16u);
#pragma unroll
        for (int i = 0; i < GB; i++) p_dma16s(bB + kt * 8, offB[i], base + (uint32_t)((GA + i) * NT) * 16u);
    };

    P c;
    c.init(lds0, wm, wn, fr, fh);
    auto store_tile = [&](auto FULL) __attribute__((always_inline)) {
        // opaque per tile: the 48 store addresses are made here, not hoisted out of the walk and kept (or spilled)
        int64_t N = N_;
        int rw = wm * WTM + 4 * fh;
        asm volatile("" : "+s"(N), "+v"(rw));
        c.store(FULL, IC<EPI>{}, C + cur.t * sC, N, M, cur.m0, rw, cur.n0 + wn * WTN + fr, pow2f(-eA), pow2f(-eB),
                bvv);
    };

    set_base(cur);
    issue(IC<0>{}, sv[0]);
    issue(IC<1>{}, sv[1]);
    P_VMCNT(G);  // step 0 landed
    P::publish();
    bool carried = false;  // the previous tile's C stores may still be in flight
    for (;;) {
        const bool more = v + nb < W;
        const PItem nxt = more ? p_item(v + nb, W, tiles, tiles_n, BM, BN) : cur;
        Frag f0, f1;
        static_for<NR>([&](auto K_) __attribute__((always_inline)) { c.rd(f0, K_, sv[0], IC<0>{}); });
        static_for<NK>([&](auto KT) __attribute__((always_inline)) {
            constexpr int kt = decltype(KT)::value, st = kt % 3, sn = (kt + 1) % 3, s2 = (kt + 2) % 3;
            if constexpr (kt == NK - 2) set_base(nxt);  // from here on the DMAs are the next item's
            issue(IC<(kt + 2) % NK>{}, sv[s2]);         // the stage read in step kt - 1
            __builtin_amdgcn_sched_barrier(0);
            c.half(f0, f1, sv[st], IC<1>{}, IC<1>{});
            P::touch(f1);
            // step kt + 1 landed: the step just issued may stay in flight, and behind the first step of a tile the
            // stores of the tile before it, which were issued between the two
            if constexpr (kt == 0) {
                if (carried)
                    P_VMCNT(CARRY);
                else
                    P_VMCNT(G);
            } else {
                P_VMCNT(G);
            }
            P::publish();  // step kt + 1 published; every wave is past its reads of step kt - 1
            if constexpr (kt + 1 < NK)
                c.half(f1, f0, sv[sn], IC<0>{}, IC<1>{});
            else
                c.half(f1, f0, 0u, IC<0>{}, IC<0>{});
        });
        if (cur.t != lt || (EPI == 1 && cur.n0 != ln)) {
            lt = cur.t, ln = cur.n0;
            eA = h3_exp(load_amax(amaxA + lt)), eB = h3_exp(load_amax(amaxB + lt));
#pragma unroll
            for (int j = 0; j < TN; j++)
                bvv[j] = EPI == 1 ? bias[(int64_t)lt * N + ln + wn * WTN + j * 32 + fr] : 0.0f;
            p_drain_loads();
        }
        carried = cur.m0 + BM <= M;
        if (carried) {
            store_tile(IC<1>{});
        } else {
            store_tile(IC<0>{});
            P_VMCNT(0);
        }
        c.zero();
        if (!more) break;
        v += nb;
        cur = nxt;
        if constexpr (NK % 3 == 1) {
            const uint32_t x = sv[0];
            sv[0] = sv[1], sv[1] = sv[2], sv[2] = x;
        } else if constexpr (NK % 3 == 2) {
            const uint32_t x = sv[2];
            sv[2] = sv[1], sv[1] = sv[0], sv[0] = x;
        }
    }
    P_VMCNT(0);  // the last tile's look-ahead DMAs: landed before the block's LDS is given away
}

// k_h3_pqg's walk (K = 576: 18 k steps, the ring's stages line up from tile to tile).  The row map of a tile
// (BM x 9 chunk rows) is itself fetched by DMA, into the other of two LDS buffers, in the middle of the tile before:
// three 4-byte DMAs per thread behind step 10's data, which the waits of steps 8 and 9 let stay in flight.
template <int BM, int BN, int WGM, int WGN, int EPI>
__device__ __forceinline__ void pqg_walk(const u32x4 *__restrict__ A, const u32x4 *__restrict__ B,
                                         const uint32_t *__restrict__ amaxA, const uint32_t *__restrict__ amaxB,
                                         int64_t M, int N, int64_t sA, int64_t sB, const float *__restrict__ bias,
                                         float *__restrict__ C, int64_t sC, int tiles_n, int tiles, int W,
                                         const int32_t *__restrict__ amap, const float *__restrict__ hw0,
                                         const float *__restrict__ hw1, int na, float *__restrict__ hpart) {
    constexpr int K = 576, NK = 18, KC = K / 64;
    using P = PCore<BM, BN, WGM, WGN>;
    using Frag = typename P::Frag;
    constexpr int NT = P::NT, WTM = P::WTM, WTN = P::WTN, TM = P::TM, TN = P::TN, NR = P::NR, GA = P::GA, GB = P::GB;
    constexpr int G = P::G, STG = P::STG;
    constexpr uint32_t STG_B = P::STG_B;
    constexpr int GX = (BM * KC + NT - 1) / NT, XS = GX * NT;  // row map DMAs per thread; ints per buffer
    constexpr int S = P::CS + (EPI == 2 ? 2 * TM : 0);         // stores per wave and tile
    constexpr int CARRY = S + G < 63 ? S + G : 63;
    const int N_ = N;
    static_assert(EPI == 1 || EPI == 2, "bias + ReLU, heads optional");
    __shared__ u32x4 lds[3 * STG];
    __shared__ int32_t gmap[2 * XS];

    int v = blockIdx.x;
    const int nb = gridDim.x;
    if (v >= W) return;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int wm = w / WGN, wn = w - (w / WGN) * WGN;
    const int fr = lane & 31, fh = lane >> 5;
    const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) u32x4 *)lds;
    const uint32_t gm0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) int32_t *)gmap;
    const uint32_t wbase = (uint32_t)__builtin_amdgcn_readfirstlane(w) * 64u;

    PItem cur = p_item(v, W, tiles, tiles_n, BM, BN);
    int lt = -1, ln = -1, eA = 0, eB = 0;
    float bvv[TN], wv[4][TN];
    auto load_consts = [&]() __attribute__((always_inline)) {  // (k_h3_pqg's epilogue loads)
        lt = cur.t, ln = cur.n0;
        eA = h3_exp(load_amax(amaxA + lt)), eB = h3_exp(load_amax(amaxB + lt));
        const float *hw = lt == 0 ? hw0 : hw1;
        const int nh = lt == 0 ? na : 1;
#pragma unroll
        for (int j = 0; j < TN; j++) {
            const int col = ln + wn * WTN + j * 32 + fr;
            bvv[j] = bias[(int64_t)lt * N + col];
#pragma unroll
            for (int o = 0; o < 4; o++) {
                if constexpr (EPI == 2) {
                    const float x = hw[(int64_t)(o < nh ? o : 0) * N + col];
                    wv[o][j] = o < nh ? x : 0.0f;
                } else {
                    wv[o][j] = 0.0f;
                }
            }
        }
        p_drain_loads();
    };
    load_consts();

    int ga[GA];
    uint32_t ca[GA], offB[GB];
#pragma unroll
    for (int i = 0; i < GA; i++) {
        const int q = i * NT + tid, r = q >> 3;
        ga[i] = r * KC;
        ca[i] = (uint32_t)((q & 7) ^ g_swz(r)) * 16u;
    }
#pragma unroll
    for (int i = 0; i < GB; i++) {
        const int q = i * NT + tid, r = q >> 3;
        offB[i] = (uint32_t)(r * (K / 4) + ((q & 7) ^ g_swz(r))) * 16u;
    }
    // (every DMA source is a uniform base + a 32-bit byte offset per lane: the launcher refuses operands past 4 GB)
    // the row map of the tile at m0 into buffer bf (rows past M - 1 clamped: read, never stored; the entries past
    // the tile's BM x KC repeat its last)
    auto issue_map = [&](int64_t m0, int bf) __attribute__((always_inline)) {
        int tl = tid;  // opaque per tile: the entries' rows and chunks are made here, not kept across the walk
        asm volatile("" : "+v"(tl));
        const int mr = (int)(M - 1 - m0);  // (M x KC fits 32 bits: the launcher's test)
#pragma unroll
        for (int i = 0; i < GX; i++) {
            const int e = std::min(i * NT + tl, BM * KC - 1), r = e / KC;
            p_dma4s(amap + m0 * KC, (uint32_t)(std::min(r, mr) * KC + (e - r * KC)) * 4u,
                    gm0 + (uint32_t)(bf * XS + i * NT) * 4u + wbase * 4u);
        }
    };
    // the byte offsets of step kt's A sources (its chunk rows are 256 B each)
    auto read_g = [&](int kt, uint32_t (&g)[GA], int bf) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < GA; i++)
            g[i] = (uint32_t)*(const lds_i32 *)(uintptr_t)(gm0 + (uint32_t)(bf * XS + ga[i] + kt / 2) * 4u) * 256u +
                   ca[i];
    };
    const u32x4 *At, *baseB;  // of the item the DMAs are issued for
    auto set_base = [&](const PItem &it) __attribute__((always_inline)) {
        At = A + it.t * sA;
        baseB = B + it.t * sB + (int64_t)it.n0 * (K / 4);
    };
    auto issue = [&](auto KT, int st, const uint32_t (&g)[GA]) __attribute__((always_inline)) {
        constexpr int kt = decltype(KT)::value;
        const uint32_t base = lds0 + (uint32_t)(st * STG) * 16u + wbase * 16u;
#pragma unroll
        for (int i = 0; i < GA; i++) p_dma16s(At + 8 * (kt & 1), g[i], base + (uint32_t)(i * NT) * 16u);
#pragma unroll
        for (int i = 0; i < GB; i++) p_dma16s(baseB + kt * 8, offB[i], base + (uint32_t)((GA + i) * NT) * 16u);
    };

    P c;
    c.init(lds0, wm, wn, fr, fh);
    // k_h3_pqg's epilogues on the item cur
    auto store_tile = [&](auto FULL) __attribute__((always_inline)) {
        const float inv = pow2f(-eA), invB = pow2f(-eB);
        float *Ct = C + cur.t * sC;
        const int col0 = cur.n0 + wn * WTN + fr;
        // opaque per tile: the store addresses are made here, not hoisted out of the walk and kept (or spilled)
        int64_t N = N_;
        int rw = wm * WTM + 4 * fh, rp = wm * WTM + 4 * fh;
        asm volatile("" : "+s"(N), "+v"(rw), "+v"(rp));
        if constexpr (EPI == 2) {
            float *part = hpart + ((int64_t)(cur.t * tiles_n + cur.tn) * WGN + wn) * M * 4;
            c.store_heads(FULL, IC<2>{}, Ct, part, N, M, cur.m0, rw, rp, col0, fr, inv, invB, bvv, wv);
        } else {
            c.store(FULL, IC<1>{}, Ct, N, M, cur.m0, rw, col0, inv, invB, bvv);
        }
    };

    int cb = 0;  // the row map buffer of the item cur
    issue_map(cur.m0, cb);
    P_VMCNT(0);
    P::publish();
    set_base(cur);
    uint32_t g0[GA], g1[GA];  // A sources of the next issue (ping-pong, compile-time choice: NK is even)
    read_g(0, g0, cb);
    issue(IC<0>{}, 0, g0);
    read_g(1, g1, cb);
    issue(IC<1>{}, 1, g1);
    read_g(2, g0, cb);
    P_VMCNT(G);
    P::publish();
    bool carried = false;
    for (;;) {
        const bool more = v + nb < W;
        const PItem nxt = more ? p_item(v + nb, W, tiles, tiles_n, BM, BN) : cur;
        Frag f0, f1;
        static_for<NR>([&](auto K_) __attribute__((always_inline)) { c.rd(f0, K_, 0, IC<0>{}); });
        static_for<NK>([&](auto KT) __attribute__((always_inline)) {
            constexpr int kt = decltype(KT)::value, st = kt % 3, sn = (kt + 1) % 3;
            uint32_t(&gu)[GA] = (kt % 2 == 0) ? g0 : g1;  // holds step kt + 2's sources
            uint32_t(&gn)[GA] = (kt % 2 == 0) ? g1 : g0;
            if constexpr (kt == NK - 2) set_base(nxt);  // from here on the DMAs are the next item's
            issue(IC<(kt + 2) % NK>{}, (kt + 2) % 3, gu);
            if constexpr (kt == 8) issue_map(nxt.m0, cb ^ 1);
            __builtin_amdgcn_sched_barrier(0);
            c.half(f0, f1, (uint32_t)st * STG_B, IC<1>{}, IC<1>{});
            P::touch(f1);
            // step kt + 1 landed; what was issued behind it may stay in flight: the step just issued, at steps 8
            // and 9 the row map's DMAs too, and behind a tile's first step the stores of the tile before it
            if constexpr (kt == 0) {
                if (carried)
                    P_VMCNT(CARRY);
                else
                    P_VMCNT(G);
            } else if constexpr (kt == 8 || kt == 9) {
                P_VMCNT(G + GX);
            } else {
                P_VMCNT(G);
            }
            P::publish();
            read_g((kt + 3) % NK, gn, kt + 3 < NK ? cb : cb ^ 1);
            if constexpr (kt + 1 < NK)
                c.half(f1, f0, (uint32_t)sn * STG_B, IC<0>{}, IC<1>{});
            else
                c.half(f1, f0, 0u, IC<0>{}, IC<0>{});
        });
        if (cur.t != lt || cur.n0 != ln) load_consts();
        carried = cur.m0 + BM <= M;
        if (carried) {
            store_tile(IC<1>{});
        } else {
            store_tile(IC<0>{});
            P_VMCNT(0);
        }
        c.zero();
        if (!more) break;
        v += nb;
        cur = nxt;
        cb ^= 1;
    }
    P_VMCNT(0);  // the last tile's look-ahead DMAs: landed before the block's LDS is given away
}

// PERS (appended behind the one-tile forms' parameters, so their names stay prefixes): the walk above.  tiles: row
// x column tiles of one tower; the one-tile form's grid is (tiles, T), the walk's at most one block per CU
template <int BM, int BN, int WGM, int WGN, int EPI, int NK, int NS = 3, bool ONE = false, int ORD = 0,
          bool PERS = false>
__global__ __launch_bounds__(64 * WGM * WGN) void k_h3_pq(const u32x4 *__restrict__ A, const u32x4 *__restrict__ B,
                                                          const uint32_t *__restrict__ amaxA,
                                                          const uint32_t *__restrict__ amaxB, int64_t M, int N, int K,
                                                          int64_t sA, int64_t sB, const float *__restrict__ bias,
                                                          float *__restrict__ C, int64_t sC, int tiles_n, int tiles,
                                                          int W) {
    if constexpr (PERS) {
        static_assert(NS == 3 && !ONE, "the walk: a 3-stage ring, two accumulators");
        pq_walk<BM, BN, WGM, WGN, EPI, NK, ORD>(A, B, amaxA, amaxB, M, N, K, sA, sB, bias, C, sC, tiles_n, tiles, W);
    } else {
        pq_tile<BM, BN, WGM, WGN, EPI, NK, NS, ONE, ORD>(A, B, amaxA, amaxB, M, N, K, sA, sB, bias, C, sC, tiles_n);
    }
}

template <int BM, int BN, int WGM, int WGN, int EPI, bool PERS = false>
__global__ __launch_bounds__(64 * WGM * WGN) void k_h3_pqg(const u32x4 *__restrict__ A, const u32x4 *__restrict__ B,
                                                           const uint32_t *__restrict__ amaxA,
                                                           const uint32_t *__restrict__ amaxB, int64_t M, int N,
                                                           int64_t sA, int64_t sB, const float *__restrict__ bias,
                                                           float *__restrict__ C, int64_t sC, int tiles_n, int tiles,
                                                           int W, const int32_t *__restrict__ amap,
                                                           const float *__restrict__ hw0, const float *__restrict__ hw1,
                                                           int na, float *__restrict__ hpart) {
    if constexpr (PERS)
        pqg_walk<BM, BN, WGM, WGN, EPI>(A, B, amaxA, amaxB, M, N, sA, sB, bias, C, sC, tiles_n, tiles, W, amap, hw0,
                                        hw1, na, hpart);
    else
        pqg_tile<BM, BN, WGM, WGN, EPI>(A, B, amaxA, amaxB, M, N, sA, sB, bias, C, sC, tiles_n, amap, hw0, hw1, na,
                                        hpart);
}

// blocks of a walk: one per CU of the current device, or the override (tests: walks that do not depend on the CU
// count), never more than there are items
int g_walk_blocks = 0;  // set_h3p_walk_blocks
int walk_blocks(int64_t items) {
    int n = g_walk_blocks;
    if (n <= 0) {
        static int cus[64];  // per device, 0 = not asked yet
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return -1;
        if (!cus[dev] && hipDeviceGetAttribute(&cus[dev], hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
            return -1;
        n = cus[dev];
    }
    return n <= 0 ? -1 : (int)std::min<int64_t>(n, items);
}

// the tiles of an M x N output over T towers and the grid that covers them: (tiles, T) blocks, one per tile, or a
// walk's blocks
struct PGrid {
    int tiles_n, tiles, W;  // column tiles; row x column tiles of one tower; items (tiles of every tower)
    dim3 grid;
};
hipError_t pq_grid(int64_t M, int N, int T, int BM, int BN, bool walk, PGrid &g) {
    const int64_t tiles_m = (M + BM - 1) / BM;
    g.tiles_n = N / BN;
    if (tiles_m * g.tiles_n * T > INT32_MAX) return hipErrorInvalidValue;
    g.tiles = (int)(tiles_m * g.tiles_n), g.W = g.tiles * T;
    g.grid = dim3((unsigned)g.tiles, T);
    if (walk) {
        const int nb = walk_blocks(g.W);
        if (nb < 1) return hipErrorInvalidValue;
        g.grid = dim3(nb);
    }
    return hipSuccess;
}

template <int BM, int BN, int WGM, int WGN, int NS = 3, bool ONE = false, int ORD = 0, bool PERS = false>
hipError_t pq_launch(const void *A, const void *B, const uint32_t *amaxA, const uint32_t *amaxB, int64_t M, int N,
                     int K, int T, int64_t sA, int64_t sB, const float *bias, float *C, int64_t sC, hipStream_t s) {
    if (N % BN || K % 32 || K < 64) return hipErrorInvalidValue;
    PGrid g;
    if (pq_grid(M, N, T, BM, BN, PERS, g) != hipSuccess) return hipErrorInvalidValue;
    const dim3 block(64 * WGM * WGN);
    const auto *a = static_cast<const u32x4 *>(A);
    const auto *b = static_cast<const u32x4 *>(B);
#define PQ_K(NK)                                                                                                    \
    do {                                                                                                            \
        if (bias)                                                                                                   \
            hipLaunchKernelGGL((k_h3_pq<BM, BN, WGM, WGN, 1, NK, NS, ONE, ORD, PERS>), g.grid, block, 0, s, a, b,   \
                               amaxA, amaxB, M, N, K, sA / 4, sB / 4, bias, C, sC, g.tiles_n, g.tiles, g.W);        \
        else                                                                                                        \
            hipLaunchKernelGGL((k_h3_pq<BM, BN, WGM, WGN, 0, NK, NS, ONE, ORD, PERS>), g.grid, block, 0, s, a, b,   \
                               amaxA, amaxB, M, N, K, sA / 4, sB / 4, nullptr, C, sC, g.tiles_n, g.tiles, g.W);     \
    } while (0)
    switch (K) {  // the k loop is unrolled: one instantiation per depth (fc1's forward K = 576, input gradient 512)
        case 576: PQ_K(18); break;
        case 512: PQ_K(16); break;
        default: return hipErrorInvalidValue;
    }
#undef PQ_K
    return hipGetLastError();
}


}  // namespace

// the walks' block count: 0 = one block per CU (the default), n > 0 = n blocks (tests of the tile walk)
void set_h3p_walk_blocks(int n) { g_walk_blocks = n > 0 ? n : 0; }

// A, B: plane images (4 B per value, strides in values); cfg 60: 128 x 256 tiles (2 x 4 waves),
// 62: 128 x 192 (4 x 2 waves of 32 x 96: N = 576).  The gathered forward's and cfg 62's kernels each have a one-tile
// form (a block per tile: 75 forward, 77 input gradient) and a persistent one (a block per CU walking tiles: 76, 78;
// the same bits); 60 and 62, the update's, are whichever of the two H3P_FWD_WALK / H3P_DGRAD_WALK names
constexpr bool H3P_FWD_WALK = true, H3P_DGRAD_WALK = true;
hipError_t launch_h3p_gemm_nt(const void *A, const uint32_t *amaxA, const void *B, const uint32_t *amaxB, int64_t M,
                              int N, int K, int T, int64_t a_stride, int64_t b_stride, const float *bias, float *C,
                              int64_t c_stride, int cfg, hipStream_t s, const int32_t *a_rows, const float *head_w0,
                              int n_actions, const float *head_w1, float *head_part) {
    if (M <= 0) return hipSuccess;
    if (a_stride % 4 || b_stride % 4) return hipErrorInvalidValue;
    if (a_rows) {  // the forward over a3's gathered planes (cfg 60 tiles, K = 576), bias + ReLU, heads optional
        constexpr int BM = 128, BN = 256;
        if ((cfg != 60 && cfg != 75 && cfg != 76) || K != 576 || N % BN || !bias || !C) return hipErrorInvalidValue;
        if (head_part && (T != 2 || n_actions < 1 || n_actions > 4 || !head_w0 || !head_w1)) return hipErrorInvalidValue;
        const bool walk = cfg == 76 || (cfg == 60 && H3P_FWD_WALK);
        // the walk's DMA sources are 32-bit byte offsets from uniform bases: a tower of A, B's tile rows, the row map
        if (walk && (a_stride > (INT64_C(1) << 30) || M * 9 > (INT64_C(1) << 30))) return hipErrorInvalidValue;
        PGrid g;
        if (pq_grid(M, N, T, BM, BN, walk, g) != hipSuccess) return hipErrorInvalidValue;
        const dim3 block(512);
        const auto *a = static_cast<const u32x4 *>(A);
        const auto *b = static_cast<const u32x4 *>(B);
#define PQG(EPI, PERS, ...)                                                                                          \
    hipLaunchKernelGGL((k_h3_pqg<BM, BN, 2, 4, EPI, PERS>), g.grid, block, 0, s, a, b, amaxA, amaxB, M, N,           \
                       a_stride / 4, b_stride / 4, bias, C, c_stride, g.tiles_n, g.tiles, g.W, a_rows, __VA_ARGS__)
        if (head_part && walk)
            PQG(2, true, head_w0, head_w1, n_actions, head_part);
        else if (head_part)
            PQG(2, false, head_w0, head_w1, n_actions, head_part);
        else if (walk)
            PQG(1, true, nullptr, nullptr, 0, nullptr);
        else
            PQG(1, false, nullptr, nullptr, 0, nullptr);
#undef PQG
        return hipGetLastError();
    }
#define PQ(...) return pq_launch<__VA_ARGS__>(A, B, amaxA, amaxB, M, N, K, T, a_stride, b_stride, bias, C, c_stride, s)
    switch (cfg) {  // PQ returns; its arguments: <BM, BN, WGM, WGN, NS = 3, ONE = false, ORD = 0, PERS = false>
        case 60: PQ(128, 256, 2, 4);
        case 62:
            if (H3P_DGRAD_WALK) PQ(128, 192, 4, 2, 3, false, 0, true);
            PQ(128, 192, 4, 2);
        case 77: PQ(128, 192, 4, 2);
        case 78: PQ(128, 192, 4, 2, 3, false, 0, true);
        // round 6: the same with a 4-stage ring (160 KB of LDS, three k steps in flight)
        case 63: PQ(128, 192, 4, 2, 4);
        // round 6: one accumulator per tile (ONE): 65: 256 x 192 tiles on a 2-stage ring (112 KB), 68: 256 x 256 over
        // 4 waves (one per SIMD: 512 registers each; 8 waves spill), 69: 192 x 192 over 6 waves, 3 stages (144 KB)
        case 65: PQ(256, 192, 4, 2, 2, true);
        // 66: 62's one-tile form with the MFMAs product-major (ORD 1: no two consecutive MFMAs on one accumulator;
        // the same bits)
        case 66: PQ(128, 192, 4, 2, 3, false, 1);
        case 68: PQ(256, 256, 2, 2, 2, true);
        case 69: PQ(192, 192, 3, 2, 3, true);
        default: return hipErrorInvalidValue;
    }
#undef PQ
}


// the weight gradient over plane operands with B's rows gathered (cfg 20: 128 x 192 tiles, 4 x 2 waves); slab as
// merlin_h3_gemm_tn's (S slabs of [T][M][N], summed in order by the caller's fold); strides in values
hipError_t launch_h3p_gemm_tn_gather(const void *A, const uint32_t *amaxA, const void *B, const uint32_t *amaxB,
                                     int64_t Kd, int M, int N, int T, int64_t a_stride, int64_t b_stride, int splits,
                                     float *slab, const int32_t *b_rows, int cfg, int *S_out, hipStream_t s) {
    // cfg 20: 128 x 192 tiles, 8 waves (the whole CU: 256 VGPRs x 2 waves per SIMD, 126 KB of LDS); cfg 21: 64 x 192,
    // 4 waves of the same wave tile (one per SIMD, ~99 KB of LDS), which leaves half of each SIMD's registers to
    // kernels queued beside it (conv3's backward sums)
    const int BM = cfg == 21 ? 64 : 128;
    constexpr int BN = 192, BK = 32;
    if ((cfg != 20 && cfg != 21) || M % BM || N % BN || N % 64 || a_stride % 4 || b_stride % 4 || !b_rows)
        return hipErrorInvalidValue;
    const int tiles_n = N / BN, tiles = (M / BM) * tiles_n;
    int S = std::max(1, splits);
    int64_t kc = (Kd + S - 1) / S;
    kc = (kc + BK - 1) / BK * BK;
    S = (int)std::max<int64_t>(1, (Kd + kc - 1) / kc);
    *S_out = S;
    if (cfg == 21)
        hipLaunchKernelGGL((k_h3_tq<64, BN, 2, 2>), dim3(tiles * S * T), dim3(256), 0, s,
                           static_cast<const u32x4 *>(A), static_cast<const u32x4 *>(B), amaxA, amaxB, Kd, M, N,
                           a_stride / 4, b_stride / 4, kc, tiles_n, tiles, S, slab, b_rows);
    else
        hipLaunchKernelGGL((k_h3_tq<128, BN, 4, 2>), dim3(tiles * S * T), dim3(512), 0, s,
                           static_cast<const u32x4 *>(A), static_cast<const u32x4 *>(B), amaxA, amaxB, Kd, M, N,
                           a_stride / 4, b_stride / 4, kc, tiles_n, tiles, S, slab, b_rows);
    return hipGetLastError();
}

}  // namespace merlin
