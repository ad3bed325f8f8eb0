// merlin_h3_tile.h -- what the two-plane ("h3") GEMM bodies of merlin_h3.hip and merlin_h3p.hip share: the vector
// types and the f16 MFMA, a wave's accumulator tile with its per-tile product and its epilogues, and the transposed
// fragment read of the TN bodies.  A body keeps what is its own: how its operands reach LDS, the order in which it
// walks (i, j, kh), its schedule and its waits.  Users: merlin_h3.hip's h3_tn_body (k_h3_tn / tng / tnp / tnq) and
// merlin_h3p.hip's PCore and k_h3_tq.  merlin_h3.hip's three NT bodies take the types, mfma16 and g_swz from here but
// keep their own accumulators and epilogues (the file's header says why).
#pragma once
#include <type_traits>

#include "merlin_internal.h"

namespace merlin {
namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;
typedef __attribute__((address_space(3))) char lds_char;

template <int V>
using IC = std::integral_constant<int, V>;  // a compile-time switch passed as an argument

__device__ __forceinline__ f32x16 mfma16(const u32x4 a, const u32x4 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0,
                                                   0);
}

// the LDS-DMA staged NT bodies' images: rows of 8 16-B chunks (a k step), chunk c of row r at slot c ^ g_swz(r)
__device__ __forceinline__ int g_swz(int r) { return (r >> 1) & 7; }

// ---------------------------------------------------------------------------------------------------------------
// The accumulators of one wave of a BM x BN block tile over WGM x WGN waves: TM x TN MFMA tiles of 32 x 32, each a
// hi (sum h_a h_b) and a lo (sum h_a l_b + l_a h_b, 2^11 up) accumulator, combined once in the epilogue.  Element r
// of a tile's accumulator in lane l is row (r & 3) + 8 (r >> 2) + 4 (l >> 5), column l & 31 of the tile.
// ONE (merlin_h3p.hip, round 6): every product into hi (the caller brings the lo planes back to scale); lo is unused.
template <int BM, int BN, int WGM, int WGN, bool ONE = false>
struct H3Tile {
    static constexpr int NT = 64 * WGM * WGN;
    static constexpr int WTM = BM / WGM, WTN = BN / WGN;
    static constexpr int TM = WTM / 32, TN = WTN / 32;
    static_assert(WTM % 32 == 0 && WTN % 32 == 0, "wave tile of 32 x 32 MFMA tiles");

    f32x16 hi[TM][TN], lo[TM][TN];

    __device__ __forceinline__ void zero() {
#pragma unroll
        for (int i = 0; i < TM; i++)
#pragma unroll
            for (int j = 0; j < TN; j++) {
                hi[i][j] = f32x16{};
                lo[i][j] = f32x16{};
            }
    }
    // tile (i, j) += a b over 16 values of k, a and b as (hi, lo) plane fragments: the three products of the file
    // header's sum, lo's two first
    __device__ __forceinline__ void mma3(int i, int j, const u32x4 a_hi, const u32x4 a_lo, const u32x4 b_hi,
                                         const u32x4 b_lo) {
        static_assert(!ONE, "two accumulators");
        lo[i][j] = mfma16(a_lo, b_hi, lo[i][j]);
        lo[i][j] = mfma16(a_hi, b_lo, lo[i][j]);
        hi[i][j] = mfma16(a_hi, b_hi, hi[i][j]);
    }
    __device__ __forceinline__ float acc(int i, int j, int r) const {
        return ONE ? hi[i][j][r] : hi[i][j][r] + lo[i][j][r] * H3_LO_INV;
    }
    // The plain epilogue: C[row][col] = acc x inv x invB (EPI 1: + bias, ReLU) over the wave's part of the tile at
    // row m0: rows m0 + rw + ..., rw = wm WTM + 4 fh; columns col0 + 32 j, col0 = n0 + wn WTN + fr; bv[j] their bias.
    // FULL: every row of the tile exists, so the stores are unconditional (a walk counts them in its vmcnt waits;
    // a TN slab, whose M is a multiple of BM)
    template <class FULL, class EPI_>
    __device__ __forceinline__ void store(FULL, EPI_, float *Ct, int64_t N, int64_t M, int64_t m0, int rw, int col0,
                                          float inv, float invB, const float (&bv)[TN]) const {
#pragma unroll
        for (int j = 0; j < TN; j++) {
            const int col = col0 + j * 32;
#pragma unroll
            for (int i = 0; i < TM; i++) {
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int64_t row = m0 + rw + i * 32 + (r & 3) + 8 * (r >> 2);
                    if (FULL::value || row < M) {
                        const float v = acc(i, j, r) * inv * invB;
                        Ct[row * N + col] = EPI_::value == 1 ? relu_nan(v + bv[j]) : v;
                    }
                }
            }
        }
    }
    // The heads epilogue (EPI 2, the update's fc1 forward): bias + ReLU as above, and of the stored values the
    // policy / value heads' partial dot products over the wave's 64 columns (wv[o][j]: head row o's weights of the
    // lane's columns), two per lane into part[row][4] (rp: rw again, for the partials' rows): CS + 2 TM stores per
    // wave.  Per i: the 16 rows x 4 head outputs of this lane's two columns, then a reduce-scatter over the 32 column
    // lanes of the half-wave (xor 16 .. 1, each step keeping the half of the values its lane bit selects): lane fr
    // ends with output o = fr >> 3 of rows r = 2 (fr & 7) + k, k < 2.  EPI 3: the partials only, h itself is not
    // written.  (merlin_h3.hip's h3_ntp_body still writes this epilogue itself: on this tile struct its heads-only
    // kernel k_h3_ntp<128, 128, 2, 2, 3> goes from 284 to 300 VGPRs, profiles/r10_isa_compare.md.)
    template <class FULL, class EPI_>
    __device__ __forceinline__ void store_heads(FULL, EPI_, float *Ct, float *part, int64_t N, int64_t M, int64_t m0,
                                                int rw, int rp, int col0, int fr, float inv, float invB,
                                                const float (&bv)[TN], const float (&wv)[4][TN]) const {
        static_assert(TN == 2 && WTN == 64, "heads epilogue: a wave tile 64 columns wide");
#pragma unroll
        for (int i = 0; i < TM; i++) {
            float pv[64];  // [o][r]
#pragma unroll
            for (int q = 0; q < 64; q++) pv[q] = 0.0f;
#pragma unroll
            for (int j = 0; j < TN; j++) {
                const int col = col0 + j * 32;
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int64_t row = m0 + rw + i * 32 + (r & 3) + 8 * (r >> 2);
                    const float v = relu_nan(acc(i, j, r) * inv * invB + bv[j]);
                    if (EPI_::value == 2 && (FULL::value || row < M)) Ct[row * N + col] = v;
#pragma unroll
                    for (int o = 0; o < 4; o++) pv[o * 16 + r] += v * wv[o][j];
                }
            }
#pragma unroll
            for (int c = 64, off = 16; off >= 1; c >>= 1, off >>= 1) {
                const bool up = (fr & off) != 0;
#pragma unroll
                for (int k = 0; k < c / 2; k++) {
                    const float send = up ? pv[k] : pv[k + c / 2], keep = up ? pv[k + c / 2] : pv[k];
                    pv[k] = keep + __shfl_xor(send, off);
                }
            }
            const int o = fr >> 3;
#pragma unroll
            for (int k = 0; k < 2; k++) {
                const int r = 2 * (fr & 7) + k;
                const int64_t row = m0 + rp + i * 32 + (r & 3) + 8 * (r >> 2);
                if (FULL::value || row < M) part[row * 4 + o] = pv[k];
            }
        }
    }
};

// ---------------------------------------------------------------------------------------------------------------
// The TN bodies' plane images: per operand and plane [32 k rows][RC chunks of 8 columns], chunk c of row r at
// r RC + (c ^ tr_swz(r)); fragments k-contiguous through ds_read_b64_tr_b16 (a 32x32x16 fragment, lane l: column
// l & 31, k = 8 (l >> 5) + j, is two transposed reads: 16-lane group g takes columns 16 (g & 1) .. + 15 and k rows
// 8 (g >> 1) + 4 h2 .. + 3).  The 16 chunks a 32-lane half reads (4 rows x 4 adjacent chunks) land on 16 distinct
// 16-B bank slots for RC = 16 (XOR 4 (r & 3)) and RC = 24 (XOR 4 ((r >> 1) & 1)).
template <int RC>
__device__ __forceinline__ int tr_swz(int row) {
    // RC = 8 (128-B rows) as RC = 24: two rows per 256-B bank row, rows r and r + 2 on the same slots
    static_assert(RC % 16 == 0 || RC == 24 || RC == 8, "row chunks");
    return RC % 16 == 0 ? (row & 3) << 2 : ((row >> 1) & 1) << 2;
}
// byte offset in its image of transposed read h2 of the fragment at columns col0 .. + 31, k rows 16 kh .. + 15
template <int RC>
__device__ __forceinline__ int tr_off(int col0, int kh, int h2, int lane) {
    const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
    const int chunk = ((col0 + 16 * (g & 1)) >> 3) + (p >> 1);
    const int row = 16 * kh + 8 * (g >> 1) + 4 * h2 + q;
    return (row * RC + (chunk ^ tr_swz<RC>(row))) * 16 + (p & 1) * 8;
}
__device__ __forceinline__ bf16x4 tr_read(const lds_char *at) {  // 16-bit lanes moved as bits (the planes are f16)
    return __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4 *)at);
}
__device__ __forceinline__ u32x4 tr_pack(const bf16x4 v0, const bf16x4 v1) {  // reads h2 = 0, 1 -> the fragment
    return __builtin_bit_cast(u32x4, bf16x8{v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]});
}
template <int RC>
__device__ __forceinline__ u32x4 tr_frag(const u32x4 *img, int col0, int kh, int lane) {
    return tr_pack(tr_read((lds_char *)img + tr_off<RC>(col0, kh, 0, lane)),
                   tr_read((lds_char *)img + tr_off<RC>(col0, kh, 1, lane)));
}

}  // namespace
}  // namespace merlin
