// merlin_plan.hip -- the per-update plan as native launches.  Phase 2 (first below): every minibatch's grouping arrays
// (merlin/windows.py WindowPlan.update_minibatches(bulk=True)) from one stable radix sort of (minibatch * F + frame,
// position) over every epoch's permutation, one scan of the run heads and one pass that writes every array the
// optimizer steps read.  Phase 1 (after it): the frame groups, the window / patch / band numbering and the four
// segmented-sum lists (merlin/dedup.py FrameGroups, WindowPlan.__init__, SegmentPlan), one sort per list.  The torch
// builders stay the oracle: every output here equals their arrays element for element
// (tests/test_gpu_native_plan.py).  Sorts and scans are rocprim's (header-only, ships with ROCm); their scratch is
// carved from the caller's workspace.
#include <cstring>  // before rocprim: its headers use std::memcpy without including it

#include <rocprim/rocprim.hpp>

#include "merlin_internal.h"

namespace merlin {
namespace {

constexpr int64_t ALIGN = 256;
inline int64_t aligned(int64_t bytes) { return (bytes + ALIGN - 1) / ALIGN * ALIGN; }

struct MbGeom {
    int64_t N, P, mbs, per, F, B0;  // samples of the update, of an epoch, of a minibatch; minibatches per epoch
    int nmb;
};

__device__ __forceinline__ int64_t mb_lo(const MbGeom &g, int m) { return (m / g.per) * g.P + (m % g.per) * g.mbs; }
__device__ __forceinline__ int64_t mb_hi(const MbGeom &g, int m) {
    const int64_t e = m / g.per, k = m % g.per;
    return e * g.P + (g.P < (k + 1) * g.mbs ? g.P : (k + 1) * g.mbs);
}

// key[pos] = minibatch(pos) * F + uid[idxs[pos]], val[pos] = pos.  An index or a frame id out of range sets *err and
// takes frame 0, so that no later pass can index out of bounds.
__global__ __launch_bounds__(256) void k_plan_keys(MbGeom g, const int64_t *__restrict__ idxs,
                                                   const int64_t *__restrict__ uid, uint32_t *__restrict__ key,
                                                   uint32_t *__restrict__ val, int64_t *__restrict__ err) {
    const int64_t pos = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (pos >= g.N) return;
    const int64_t e = pos / g.P, r = pos - e * g.P;
    const int64_t m = e * g.per + r / g.mbs;
    const int64_t i = idxs[pos];
    int64_t u = 0;
    if (i < 0 || i >= g.B0) {
        *err = 1;
    } else {
        u = uid[i];
        if (u < 0 || u >= g.F) {
            *err = 1;
            u = 0;
        }
    }
    key[pos] = (uint32_t)(m * g.F + u);
    val[pos] = (uint32_t)pos;
}

__global__ __launch_bounds__(256) void k_plan_heads(int64_t N, const uint32_t *__restrict__ sk,
                                                    int32_t *__restrict__ head) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    head[i] = (i == 0 || sk[i] != sk[i - 1]) ? 1 : 0;
}

// Sorted position i holds sample pos = sv[i] of group rank[i] - 1 (rank: inclusive scan of the heads).  Minibatch m's
// samples are exactly the sorted positions lo(m) .. hi(m) (m is the major key and its sample count is fixed), so its
// first group is rank[lo(m)] - 1 and every per-minibatch offset is known without a second pass.
__global__ __launch_bounds__(256) void k_plan_derive(MbGeom g, const uint32_t *__restrict__ sk,
                                                     const uint32_t *__restrict__ sv, const int32_t *__restrict__ rank,
                                                     int64_t *__restrict__ gkey, int64_t *__restrict__ gall,
                                                     int64_t *__restrict__ inv, int32_t *__restrict__ slot,
                                                     int32_t *__restrict__ order, int32_t *__restrict__ offs,
                                                     int64_t *__restrict__ goff) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= g.N) return;
    const int64_t key = sk[i], pos = sv[i];
    const int m = (int)(key / g.F);
    const int64_t frame = key - (int64_t)m * g.F;
    const int64_t lo = mb_lo(g, m), hi = mb_hi(g, m);
    const int64_t grp = rank[i] - 1, g0 = rank[lo] - 1;
    inv[pos] = grp - g0;
    order[i] = (int32_t)((pos % g.P) % g.mbs);
    if (i == 0 || sk[i - 1] != (uint32_t)key) {
        gkey[grp] = key;
        gall[grp] = frame;
        slot[(int64_t)m * g.F + frame] = (int32_t)(grp - g0);
        offs[grp + m] = (int32_t)(i - lo);
    }
    if (i == lo) goff[m] = grp;
    if (i == hi - 1) {
        offs[grp + 1 + m] = (int32_t)(hi - lo);
        if (m == g.nmb - 1) goff[g.nmb] = grp + 1;
    }
}

int key_bits(int64_t span) {  // bits of the largest key, span - 1
    int b = 1;
    while (b < 32 && ((int64_t)1 << b) < span) ++b;
    return b;
}

struct PlanScratch {
    int64_t key_in, val_in, key_out, val_out, rank, temp, temp_bytes, total;
};

hipError_t plan_scratch(int64_t N, int bits, PlanScratch &s) {
    size_t sort_bytes = 0, scan_bytes = 0;
    hipError_t e = rocprim::radix_sort_pairs(nullptr, sort_bytes, (uint32_t *)nullptr, (uint32_t *)nullptr,
                                             (uint32_t *)nullptr, (uint32_t *)nullptr, (size_t)N, 0u, (unsigned)bits);
    if (e != hipSuccess) return e;
    e = rocprim::inclusive_scan(nullptr, scan_bytes, (int32_t *)nullptr, (int32_t *)nullptr, (size_t)N,
                                rocprim::plus<int32_t>());
    if (e != hipSuccess) return e;
    const int64_t a = aligned(N * 4);
    s.key_in = 0;
    s.val_in = a;
    s.key_out = 2 * a;
    s.val_out = 3 * a;
    s.rank = 4 * a;
    s.temp = 5 * a;
    s.temp_bytes = aligned((int64_t)std::max(sort_bytes, scan_bytes));
    s.total = s.temp + s.temp_bytes;
    return hipSuccess;
}

// ---- phase 1: frames, windows, patches, bands and the four segmented-sum lists ---------------------------------
// (merlin/dedup.py FrameGroups, merlin/windows.py WindowPlan.__init__ and SegmentPlan as native launches.)  Every
// list is one stable sort of (key, entry index): the run ids are the numbering (torch.unique's inverse) and the
// sorted order is the destination-sorted entry list, where torch sorts once to number and once more to order.

constexpr int64_t W9 = 1953125;         // 5^9 window keys
constexpr int64_t B15 = 30517578125LL;  // 5^15 band keys per row

// Scratch of one sort of n (key, uint32) pairs with run ranks: carved from the caller's workspace.
template <class K>
struct SortBufs {
    K *kin, *kout;
    uint32_t *vin, *vout;
    int32_t *rank;  // inclusive scan of the run heads of kout (rank - 1 = run id); head() holds the flags
    void *temp;
    size_t temp_bytes;
    int64_t n;

    static hipError_t bytes(int64_t n, int64_t &total, size_t &temp_bytes) {
        size_t sort_bytes = 0, scan_bytes = 0;
        hipError_t e = rocprim::radix_sort_pairs(nullptr, sort_bytes, (K *)nullptr, (K *)nullptr, (uint32_t *)nullptr,
                                                 (uint32_t *)nullptr, (size_t)n, 0u, (unsigned)(8 * sizeof(K)));
        if (e != hipSuccess) return e;
        e = rocprim::inclusive_scan(nullptr, scan_bytes, (int32_t *)nullptr, (int32_t *)nullptr, (size_t)n,
                                    rocprim::plus<int32_t>());
        if (e != hipSuccess) return e;
        size_t table_bytes = 0;  // the frames stage also scans the 5^9 window marks with this scratch
        e = rocprim::exclusive_scan(nullptr, table_bytes, (int32_t *)nullptr, (int32_t *)nullptr, (int32_t)0,
                                    (size_t)W9, rocprim::plus<int32_t>());
        if (e != hipSuccess) return e;
        // (queried for all key bits: a sort over fewer bits runs fewer digit passes over the same buffers, and
        // rocprim returns hipErrorInvalidValue, not a fault, should a call ever want more than it is given)
        temp_bytes = (size_t)aligned((int64_t)std::max(std::max(sort_bytes, scan_bytes), table_bytes));
        total = 2 * aligned(n * (int64_t)sizeof(K)) + 4 * aligned(n * 4) + (int64_t)temp_bytes;
        return hipSuccess;
    }

    hipError_t carve(void *ws, int64_t ws_bytes, int64_t n_) {
        n = n_;
        int64_t total;
        hipError_t e = bytes(n, total, temp_bytes);
        if (e != hipSuccess) return e;
        if (ws_bytes < total) return hipErrorInvalidValue;
        char *w = (char *)ws;
        const int64_t ak = aligned(n * (int64_t)sizeof(K)), av = aligned(n * 4);
        kin = (K *)w, kout = (K *)(w + ak);
        vin = (uint32_t *)(w + 2 * ak), vout = (uint32_t *)(w + 2 * ak + av);
        rank = (int32_t *)(w + 2 * ak + 2 * av);
        // (one more av-sized slot holds the head flags)
        temp = w + 2 * ak + 4 * av;
        return hipSuccess;
    }
    int32_t *head() const { return (int32_t *)((char *)rank + aligned(n * 4)); }
};

template <class K>
__global__ __launch_bounds__(256) void k_plan_run_heads(int64_t n, const K *__restrict__ sk,
                                                        int32_t *__restrict__ head) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    head[i] = (i == 0 || sk[i] != sk[i - 1]) ? 1 : 0;
}

template <class K>
hipError_t sort_and_rank(SortBufs<K> &b, int bits, bool want_rank, hipStream_t st) {
    size_t tb = b.temp_bytes;
    hipError_t e = rocprim::radix_sort_pairs(b.temp, tb, b.kin, b.kout, b.vin, b.vout, (size_t)b.n, 0u,
                                             (unsigned)bits, st);
    if (e != hipSuccess || !want_rank) return e;
    const dim3 grid((unsigned)((b.n + 255) / 256));
    hipLaunchKernelGGL(k_plan_run_heads<K>, grid, dim3(256), 0, st, b.n, b.kout, b.head());
    if ((e = hipGetLastError()) != hipSuccess) return e;
    tb = b.temp_bytes;
    return rocprim::inclusive_scan(b.temp, tb, b.head(), b.rank, (size_t)b.n, rocprim::plus<int32_t>(), st);
}

struct Mult8 {
    uint64_t m[8];
};

// merlin/dedup.py hash_codes: wrapping 64-bit arithmetic, logical shift
__global__ __launch_bounds__(256) void k_plan_hash(const uint32_t *__restrict__ codes, int64_t B, Mult8 mu,
                                                   int64_t *__restrict__ key, uint32_t *__restrict__ val) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= B) return;
    uint64_t h = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        h = (h ^ (uint64_t)codes[i * 8 + k]) * mu.m[k];
        h ^= h >> 29;
    }
    key[i] = (int64_t)h;
    val[i] = (uint32_t)i;
}

__device__ __forceinline__ int tile_class(const uint32_t (&w)[8], int r, int c) {
    const int cell = r * 7 + c;
    const int v = (int)((w[cell >> 3] >> ((cell & 7) * 4)) & 0xF);
    return v > 4 ? 4 : v;
}

enum { CNT_F = 0, CNT_BAD = 1, CNT_NW = 2, CNT_ROWS = 3, CNT_K = 4, CNT_NB = 5, CNT_NOWIN = 6, CNT_N = 8 };

// Sorted position i holds frame sidx[i] of group rank[i] - 1.  Every frame gets its group id; each group's first
// sorted frame is its representative, whose 25 window keys (marked in the 5^9 table) and 9 patch keys are written at
// the group's rows.
__global__ __launch_bounds__(256) void k_plan_frames(int64_t B, const int64_t *__restrict__ sh,
                                                     const uint32_t *__restrict__ sidx,
                                                     const int32_t *__restrict__ rank,
                                                     const uint32_t *__restrict__ codes, int64_t *__restrict__ uid,
                                                     int64_t *__restrict__ rep, int32_t *__restrict__ wkey,
                                                     uint64_t *__restrict__ pkey, int32_t *__restrict__ mark,
                                                     int64_t *__restrict__ counts) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= B) return;
    const int64_t u = rank[i] - 1, frame = sidx[i];
    uid[frame] = u;
    if (i == B - 1) counts[CNT_F] = u + 1;
    if (i > 0 && sh[i] == sh[i - 1]) return;
    rep[u] = frame;
    uint32_t w[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) w[k] = codes[frame * 8 + k];
    int r3[7][5], r5[7][3];
#pragma unroll
    for (int r = 0; r < 7; ++r) {
        int c[7];
#pragma unroll
        for (int x = 0; x < 7; ++x) c[x] = tile_class(w, r, x);
#pragma unroll
        for (int x = 0; x < 5; ++x) r3[r][x] = c[x] * 25 + c[x + 1] * 5 + c[x + 2];
#pragma unroll
        for (int x = 0; x < 3; ++x) r5[r][x] = (((c[x] * 5 + c[x + 1]) * 5 + c[x + 2]) * 5 + c[x + 3]) * 5 + c[x + 4];
    }
#pragma unroll
    for (int py = 0; py < 5; ++py)
#pragma unroll
        for (int px = 0; px < 5; ++px) {
            const int k = r3[py][px] * 15625 + r3[py + 1][px] * 125 + r3[py + 2][px];
            wkey[u * 25 + py * 5 + px] = k;
            mark[k] = 1;
        }
#pragma unroll
    for (int oy = 0; oy < 3; ++oy)
#pragma unroll
        for (int ox = 0; ox < 3; ++ox) {
            uint64_t k = 0;
#pragma unroll
            for (int a = 0; a < 5; ++a) k = k * 3125 + (uint64_t)r5[oy + a][ox];
            pkey[u * 9 + oy * 3 + ox] = k;
        }
}

// every frame word for word against its group's representative
__global__ __launch_bounds__(256) void k_plan_verify(int64_t B, const uint32_t *__restrict__ codes,
                                                     const int64_t *__restrict__ uid, const int64_t *__restrict__ rep,
                                                     int64_t *__restrict__ counts) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= B) return;
    const int64_t r = rep[uid[i]];
    bool same = true;
#pragma unroll
    for (int k = 0; k < 8; ++k) same = same && codes[i * 8 + k] == codes[r * 8 + k];
    if (!same) counts[CNT_BAD] = 1;
}

__global__ __launch_bounds__(256) void k_plan_count_windows(const int32_t *__restrict__ mark,
                                                            const int32_t *__restrict__ wrank,
                                                            int64_t *__restrict__ counts) {
    if (blockIdx.x == 0 && threadIdx.x == 0) counts[CNT_NW] = (int64_t)wrank[W9 - 1] + mark[W9 - 1];
}

// merlin/windows.py window_rows: the conv2 table row each tap 4 ky + kx of window `key` reads
__device__ __forceinline__ int window_row(int key, int ky, int kx) {
    int d[9], q = key;
#pragma unroll
    for (int i = 8; i >= 0; --i) {
        d[i] = q % 5;
        q /= 5;
    }
    const int i = 3 * (ky >> 1) + (kx >> 1), j = 2 * (ky >> 1) + (kx >> 1);
    if (!(ky & 1) && !(kx & 1)) return 4 * d[i] + j;
    if (!(ky & 1)) return 20 + 4 * (5 * d[i] + d[i + 1]) + j;
    if (!(kx & 1)) return 120 + 4 * (5 * d[i] + d[i + 3]) + j;
    return 220 + 4 * (125 * d[i] + 25 * d[i + 1] + 5 * d[i + 3] + d[i + 4]) + j;
}

// one thread per (window key, tap): the marked keys' table rows at their rank, as the dT2 list's sort input too
__global__ __launch_bounds__(256) void k_plan_window_rows(const int32_t *__restrict__ mark,
                                                          const int32_t *__restrict__ wrank, int lut_rows,
                                                          int32_t *__restrict__ rows, uint32_t *__restrict__ hkey,
                                                          uint32_t *__restrict__ hval, int64_t *__restrict__ counts) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= W9 * 16) return;
    const int key = (int)(t >> 4), tap = (int)(t & 15);
    if (!mark[key]) return;
    const int w = wrank[key], r = window_row(key, tap >> 2, tap & 3);
    if (r >= lut_rows) counts[CNT_ROWS] = 1;
    rows[w * 16 + tap] = r;
    hkey[w * 16 + tap] = (uint32_t)r;
    hval[w * 16 + tap] = (uint32_t)(w * 16 + tap);
}

__global__ __launch_bounds__(256) void k_plan_wid(int64_t n, const int32_t *__restrict__ wkey,
                                                  const int32_t *__restrict__ wrank, int32_t *__restrict__ wid) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < n) wid[e] = wrank[wkey[e]];
}

// list outputs after a sort: MODE 0 dT2 (key = the sorted table rows, idx = entry / 16), 1 patches (key = run id, idx
// = entry, kid[entry] = run id, pk[run] = patch key), 2 bands (key = run id, idx = entry % div, ub[run] = band key), 3
// dQ (key = the sorted destinations, idx = entry % div)
template <int MODE, class K>
__global__ __launch_bounds__(256) void k_plan_list(int64_t n, const K *__restrict__ sk,
                                                   const uint32_t *__restrict__ sv, const int32_t *__restrict__ rank,
                                                   int64_t div, int32_t *__restrict__ key, int32_t *__restrict__ idx,
                                                   int32_t *__restrict__ inverse, uint64_t *__restrict__ uniq,
                                                   int64_t *__restrict__ count) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t e = sv[i];
    if (MODE == 0 || MODE == 3) {
        key[i] = (int32_t)sk[i];
        idx[i] = MODE == 0 ? (int32_t)(e >> 4) : (int32_t)(e % (uint32_t)div);
    } else {
        const int32_t run = rank[i] - 1;
        key[i] = run;
        idx[i] = MODE == 1 ? (int32_t)e : (int32_t)(e % (uint32_t)div);
        if (MODE == 1) inverse[e] = run;
        if (i == 0 || sk[i] != sk[i - 1]) uniq[run] = (uint64_t)sk[i];
        if (i == n - 1) *count = run + 1;
    }
}

// entry ky * K + k: band ky of patch k = its tile rows ky .. ky + 2 = digits 5 ky .. 5 ky + 14 of the patch key
__global__ __launch_bounds__(256) void k_plan_band_keys(int64_t K, const uint64_t *__restrict__ pk,
                                                        uint64_t *__restrict__ key, uint32_t *__restrict__ val) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= 3 * K) return;
    const int ky = (int)(e / K);
    const int64_t k = e - ky * K;
    const uint64_t div = ky == 0 ? 9765625ULL : ky == 1 ? 3125ULL : 1ULL;  // 5^(10 - 5 ky)
    key[e] = (uint64_t)ky * (uint64_t)B15 + (pk[k] / div) % (uint64_t)B15;
    val[e] = (uint32_t)e;
}

// entry kx * nb + j: band j's window at column kx -> Q row w * 9 + ky * 3 + kx
__global__ __launch_bounds__(256) void k_plan_dq_keys(int64_t nb, const uint64_t *__restrict__ ub,
                                                      const int32_t *__restrict__ mark,
                                                      const int32_t *__restrict__ wrank, uint32_t *__restrict__ key,
                                                      uint32_t *__restrict__ val, int64_t *__restrict__ counts) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= 3 * nb) return;
    const int kx = (int)(e / nb);
    const int64_t j = e - kx * nb;
    const uint64_t b = ub[j], bky = b / (uint64_t)B15, bkey = b % (uint64_t)B15;
    const int p5 = kx == 0 ? 25 : kx == 1 ? 5 : 1;  // 5^(2 - kx)
    const int c0 = (int)((bkey / 9765625ULL) % 3125) / p5 % 125, c1 = (int)((bkey / 3125ULL) % 3125) / p5 % 125,
              c2 = (int)(bkey % 3125) / p5 % 125;
    const int wk = (c0 * 125 + c1) * 125 + c2;
    if (!mark[wk]) counts[CNT_NOWIN] = 1;  // cannot happen: a band's windows are windows of a frame
    key[e] = (uint32_t)(wrank[wk] * 9 + (int)bky * 3 + kx);
    val[e] = (uint32_t)e;
}

__device__ __forceinline__ int64_t plan_bound(const int32_t *key, int64_t n, int32_t x, bool upper) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (upper ? key[mid] <= x : key[mid] < x)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// merlin/windows.py SegmentPlan: per item j of L entries, the fix row and the head fix
__global__ __launch_bounds__(256) void k_plan_segfix(const int32_t *__restrict__ key, int64_t n, int64_t L,
                                                     int64_t nitems, int4 *__restrict__ fix,
                                                     int32_t *__restrict__ head_fix) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= nitems) return;
    const int64_t p = ((j + 1) * L < n ? (j + 1) * L : n) - 1;
    const int32_t kp = key[p];
    const int64_t s = plan_bound(key, n, kp, false), e = plan_bound(key, n, kp, true);
    const bool live = e > (j + 1) * L && s >= j * L;
    fix[j] = make_int4(live ? kp : -1, (int)j, (int)((e - 1) / L), s != j * L ? 1 : 0);
    const int64_t sf = plan_bound(key, n, key[j * L], false);
    head_fix[j] = sf < j * L ? (int32_t)(sf / L) : -1;
}

__global__ __launch_bounds__(256) void k_plan_copy_keys(int64_t n, const uint64_t *__restrict__ src,
                                                        uint64_t *__restrict__ key, uint32_t *__restrict__ val) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    key[e] = src[e];
    val[e] = (uint32_t)e;
}

hipError_t launch_segfix(const int32_t *key, int64_t n, int64_t L, int32_t *fix, int32_t *head_fix, hipStream_t st) {
    const int64_t nitems = (n + L - 1) / L;
    hipLaunchKernelGGL(k_plan_segfix, dim3((unsigned)((nitems + 255) / 256)), dim3(256), 0, st, key, n, L, nitems,
                       (int4 *)fix, head_fix);
    return hipGetLastError();
}

inline dim3 grid_of(int64_t n) { return dim3((unsigned)((n + 255) / 256)); }

}  // namespace

int64_t plan_sort_workspace(int64_t n, int key_bytes) {
    int64_t total = -1;
    size_t tb;
    if (n <= 0) return -1;
    const hipError_t e = key_bytes == 8 ? SortBufs<uint64_t>::bytes(n, total, tb) : SortBufs<uint32_t>::bytes(n, total, tb);
    return e == hipSuccess ? total : -1;
}

hipError_t launch_plan_frames(const uint32_t *codes, int64_t B, const uint64_t *mult, void *ws, int64_t ws_bytes,
                              int64_t *uid, int64_t *rep, int32_t *wkey, uint64_t *pkey, int32_t *mark,
                              int32_t *wrank, int64_t *counts, hipStream_t st) {
    SortBufs<int64_t> b;
    hipError_t e = b.carve(ws, ws_bytes, B);
    if (e != hipSuccess) return e;
    Mult8 mu;
    for (int k = 0; k < 8; ++k) mu.m[k] = mult[k];
    if ((e = hipMemsetAsync(counts, 0, CNT_N * 8, st)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(mark, 0, W9 * 4, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_plan_hash, grid_of(B), dim3(256), 0, st, codes, B, mu, b.kin, b.vin);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = sort_and_rank(b, 64, true, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_plan_frames, grid_of(B), dim3(256), 0, st, B, b.kout, b.vout, b.rank, codes, uid, rep, wkey,
                       pkey, mark, counts);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_plan_verify, grid_of(B), dim3(256), 0, st, B, codes, uid, rep, counts);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    // the window numbering: ranks of the marked keys in key order (no sort: the keys are below 5^9)
    size_t tb = b.temp_bytes, need = 0;
    e = rocprim::exclusive_scan(nullptr, need, mark, wrank, (int32_t)0, (size_t)W9, rocprim::plus<int32_t>());
    if (e != hipSuccess) return e;
    if (need > tb) return hipErrorInvalidValue;
    e = rocprim::exclusive_scan(b.temp, tb, mark, wrank, (int32_t)0, (size_t)W9, rocprim::plus<int32_t>(), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_plan_count_windows, dim3(1), dim3(256), 0, st, mark, wrank, counts);
    return hipGetLastError();
}

hipError_t launch_plan_windows(int64_t F, int64_t nw, const int32_t *wkey, const int32_t *mark, const int32_t *wrank,
                               int lut_rows, int64_t L, void *ws, int64_t ws_bytes, int32_t *wid, int32_t *rows,
                               int32_t *key, int32_t *idx, int32_t *fix, int32_t *head_fix, int64_t *counts,
                               hipStream_t st) {
    SortBufs<uint32_t> b;
    hipError_t e = b.carve(ws, ws_bytes, nw * 16);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_plan_wid, grid_of(F * 25), dim3(256), 0, st, F * 25, wkey, wrank, wid);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_plan_window_rows, grid_of(W9 * 16), dim3(256), 0, st, mark, wrank, lut_rows, rows, b.kin,
                       b.vin, counts);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = sort_and_rank(b, key_bits(lut_rows > 1 ? 2 * (int64_t)lut_rows : 2), false, st)) != hipSuccess) return e;
    hipLaunchKernelGGL((k_plan_list<0, uint32_t>), grid_of(b.n), dim3(256), 0, st, b.n, b.kout, b.vout, nullptr,
                       (int64_t)16, key, idx, nullptr, nullptr, nullptr);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return launch_segfix(key, b.n, L, fix, head_fix, st);
}

hipError_t launch_plan_patches(int64_t F, const uint64_t *pkey, int64_t L, void *ws, int64_t ws_bytes, int32_t *kid,
                               uint64_t *pk, int32_t *key, int32_t *idx, int32_t *fix, int32_t *head_fix,
                               int64_t *counts, hipStream_t st) {
    SortBufs<uint64_t> b;
    hipError_t e = b.carve(ws, ws_bytes, F * 9);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_plan_copy_keys, grid_of(b.n), dim3(256), 0, st, b.n, pkey, b.kin, b.vin);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = sort_and_rank(b, 59, true, st)) != hipSuccess) return e;  // 5^25 < 2^59
    hipLaunchKernelGGL((k_plan_list<1, uint64_t>), grid_of(b.n), dim3(256), 0, st, b.n, b.kout, b.vout, b.rank,
                       (int64_t)1, key, idx, kid, pk, counts + CNT_K);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return launch_segfix(key, b.n, L, fix, head_fix, st);
}

hipError_t launch_plan_bands(int64_t K, const uint64_t *pk, int64_t L, void *ws, int64_t ws_bytes, uint64_t *ub,
                             int32_t *key, int32_t *idx, int32_t *fix, int32_t *head_fix, int64_t *counts,
                             hipStream_t st) {
    SortBufs<uint64_t> b;
    hipError_t e = b.carve(ws, ws_bytes, K * 3);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_plan_band_keys, grid_of(b.n), dim3(256), 0, st, K, pk, b.kin, b.vin);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = sort_and_rank(b, 37, true, st)) != hipSuccess) return e;  // 3 * 5^15 < 2^37
    hipLaunchKernelGGL((k_plan_list<2, uint64_t>), grid_of(b.n), dim3(256), 0, st, b.n, b.kout, b.vout, b.rank, K, key,
                       idx, nullptr, ub, counts + CNT_NB);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return launch_segfix(key, b.n, L, fix, head_fix, st);
}

hipError_t launch_plan_dq(int64_t nb, int64_t nw, const uint64_t *ub, const int32_t *mark, const int32_t *wrank,
                          int64_t L, void *ws, int64_t ws_bytes, int32_t *key, int32_t *idx, int32_t *fix,
                          int32_t *head_fix, int64_t *counts, hipStream_t st) {
    SortBufs<uint32_t> b;
    hipError_t e = b.carve(ws, ws_bytes, nb * 3);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_plan_dq_keys, grid_of(b.n), dim3(256), 0, st, nb, ub, mark, wrank, b.kin, b.vin, counts);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = sort_and_rank(b, key_bits(nw * 9), false, st)) != hipSuccess) return e;
    hipLaunchKernelGGL((k_plan_list<3, uint32_t>), grid_of(b.n), dim3(256), 0, st, b.n, b.kout, b.vout, nullptr, nb,
                       key, idx, nullptr, nullptr, nullptr);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return launch_segfix(key, b.n, L, fix, head_fix, st);
}

int64_t plan_minibatches_workspace(int64_t N, int64_t key_span) {
    PlanScratch s;
    if (N <= 0 || plan_scratch(N, key_bits(key_span), s) != hipSuccess) return -1;
    return s.total;
}

hipError_t launch_plan_minibatches(const int64_t *idxs, int64_t N, int64_t P, int64_t mbs, const int64_t *uid,
                                   int64_t B0, int64_t F, void *ws, int64_t ws_bytes, int64_t *gkey, int64_t *gall,
                                   int64_t *inv, int32_t *slot, int32_t *order, int32_t *offs, int64_t *goff,
                                   hipStream_t st) {
    MbGeom g;
    g.N = N, g.P = P, g.mbs = mbs, g.F = F, g.B0 = B0;
    g.per = (P + mbs - 1) / mbs;
    g.nmb = (int)((N / P) * g.per);
    const int bits = key_bits((int64_t)g.nmb * F);
    PlanScratch s;
    hipError_t e = plan_scratch(N, bits, s);
    if (e != hipSuccess) return e;
    if (ws_bytes < s.total) return hipErrorInvalidValue;
    char *w = (char *)ws;
    uint32_t *key_in = (uint32_t *)(w + s.key_in), *val_in = (uint32_t *)(w + s.val_in);
    uint32_t *key_out = (uint32_t *)(w + s.key_out), *val_out = (uint32_t *)(w + s.val_out);
    int32_t *rank = (int32_t *)(w + s.rank);
    const dim3 grid((unsigned)((N + 255) / 256));
    e = hipMemsetAsync(slot, 0xFF, (size_t)g.nmb * F * 4, st);  // -1: the frame is not in the minibatch
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(goff, 0, (size_t)(g.nmb + 2) * 8, st);  // goff[nmb + 1]: the error flag
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_plan_keys, grid, dim3(256), 0, st, g, idxs, uid, key_in, val_in, goff + g.nmb + 1);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    size_t tb = (size_t)s.temp_bytes;
    e = rocprim::radix_sort_pairs(w + s.temp, tb, key_in, key_out, val_in, val_out, (size_t)N, 0u, (unsigned)bits, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_plan_heads, grid, dim3(256), 0, st, N, key_out, (int32_t *)key_in);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    tb = (size_t)s.temp_bytes;
    e = rocprim::inclusive_scan(w + s.temp, tb, (int32_t *)key_in, rank, (size_t)N, rocprim::plus<int32_t>(), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_plan_derive, grid, dim3(256), 0, st, g, key_out, val_out, rank, gkey, gall, inv, slot, order,
                       offs, goff);
    return hipGetLastError();
}

}  // namespace merlin
