// merlin_render.hip -- full-grid RGB frames: minigrid's render() in rgb_array mode, get_frame(highlight, tile_size)
// = Grid.render of the whole grid, tile (i, j) blitted to img[ts j : ts j + ts, ts i : ts i + ts], the agent's
// triangle in its world direction, every cell the agent's 7x7 view shows brightened.
//
// Write-bound: ~80 B of state in, (size ts)^2 3 B out per frame (786,432 B at 16x16 cells of 32 px).  A frame is a
// flat byte range; its 16-B aligned body is emitted as one uint4 store per thread, consecutive threads consecutive
// chunks, assembled from the frame atlas (include/merlin_hip.h MERLIN_FRAME_TILES): the 6 agent-less tiles from an LDS
// copy (18 KB at 32 px), the one agent tile of a frame through L2.  A work item is one slab of one frame's chunks
// (the slabs of a frame interleave in 4-KB stripes, so the blocks that share a frame write one contiguous front: 13 %
// faster than contiguous slabs at 32 px); per item one lane computes the view's visibility mask (view_mask, the
// observation's own code) into LDS, the block then fills the frame's cell -> tile table in LDS, and only then are
// pixels produced: a table lookup each.
//
// Three assembly paths per chunk, chosen per frame (uniform in the block):
//   * tile rows that are multiples of 4 B (ts % 4 == 0) and a frame whose body starts on a 4-B boundary of the
//     frame: four aligned 32-bit atlas reads, each inside one tile row -- or one 128-bit read when the chunk lies in
//     one tile row on a 16-B boundary of the atlas (every chunk at 32 px, a third of them at 8 px, where a 24-B tile
//     row makes two of three chunks straddle two tiles);
//   * anything else (odd tile sizes, frame bases that are not 4-B aligned): sixteen byte reads.
// The frame's unaligned head and tail (< 16 B each) are byte stores by the first lanes of its first / last slab.
#include <algorithm>

#include "merlin_internal.h"

namespace merlin {
namespace {

constexpr int RB = 256;           // threads per block
constexpr int PLAIN = 6;          // atlas tiles without the agent: (empty, wall, goal) x (plain, highlighted)
constexpr int MAX_TS = 32, MAX_S = 32;
// 256 CUs x 6 blocks.  Measured at 256 frames of 16x16 cells, 32 px: 2 blocks per CU leave the stores
// latency-bound, beyond 6 the per-item set-up of the extra slabs costs more than the occupancy gains
constexpr int MAX_BLOCKS = 1536;

struct RenderArgs {
    const uint32_t *walls;     // [maps][wall_stride] bit rows
    int64_t wall_stride;
    const int32_t *goal;       // stateless: [maps][2] (nullable: no goal)
    const int32_t *agent;      // stateless: [F][4] = x, y, dir, 0
    const uint4 *env_agent;    // env context: the packed agent state (merlin_internal.h EnvDev::agent)
    const int64_t *env_index;  // env context: env id of frame f (nullable: f)
    int64_t n_envs;
    const int32_t *map_index;  // stateless: map of frame f (nullable: f)
    int64_t n_frames;
    int S, ts, highlight, slabs;
    float inv_row, inv_ts, inv_ts3;  // reciprocals of the three divisors of the pixel decode
    const uint8_t *atlas;            // [MERLIN_FRAME_TILES][ts][ts][3]
    uint8_t *out;
    uint32_t *err;
};

// a / d for 0 <= a < 2^23 by a float reciprocal (the estimate is off by at most one), remainder in r
__device__ __forceinline__ int divmod(int a, int d, float inv, int &r) {
    int q = (int)((float)a * inv);
    r = a - q * d;
    if (r < 0) {
        q--;
        r += d;
    } else if (r >= d) {
        q++;
        r -= d;
    }
    return q;
}

__global__ __launch_bounds__(RB) void k_render_frames(const RenderArgs A) {
    __shared__ uint4 s_atlas4[PLAIN * MAX_TS * MAX_TS * 3 / 16];
    __shared__ uint8_t s_tid[MAX_S * MAX_S];
    __shared__ uint32_t s_m[8];  // the 7 mask rows, [7] = 1 when the agent is drawable
    const uint32_t *s_atlas32 = reinterpret_cast<const uint32_t *>(s_atlas4);
    const uint8_t *s_atlas8 = reinterpret_cast<const uint8_t *>(s_atlas4);
    const uint32_t *g_atlas32 = reinterpret_cast<const uint32_t *>(A.atlas);
    const int S = A.S, ts = A.ts, ts3 = 3 * ts, rowb = S * ts3;
    const int FB = rowb * S * ts;  // bytes per frame, <= 3,145,728
    {
        // the agent-less tiles, whole words (the last word may reach into tile 6: still inside the atlas)
        const int words = (PLAIN * ts * ts3 + 3) >> 2;
        uint32_t *dst = reinterpret_cast<uint32_t *>(s_atlas4);
        for (int k = threadIdx.x; k < words; k += RB) dst[k] = g_atlas32[k];
    }
    const int64_t items = A.n_frames * A.slabs;
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int64_t f = item / A.slabs;
        const int slab = (int)(item - f * A.slabs);
        // -- the frame's state (uniform in the block) -------------------------------------------------------------
        int ax, ay, dir, gx = -1, gy = -1;
        int64_t map;
        bool bad = false;
        if (A.env_agent) {
            map = A.env_index ? A.env_index[f] : f;
            if (map < 0 || map >= A.n_envs) {
                bad = true;
                map = 0;
            }
            const uint4 a = A.env_agent[map];
            ax = a.x & 0xff;
            ay = (a.x >> 8) & 0xff;
            dir = (a.x >> 16) & 3;
            gx = a.z & 0xff;
            gy = (a.z >> 8) & 0xff;
        } else {
            map = A.map_index ? (int64_t)A.map_index[f] : f;
            ax = A.agent[4 * f];
            ay = A.agent[4 * f + 1];
            dir = A.agent[4 * f + 2];
            if (A.goal) {
                gx = A.goal[2 * map];
                gy = A.goal[2 * map + 1];
            }
        }
        const uint32_t *wrow = A.walls + map * A.wall_stride;
        bool ok = !bad && ax >= 0 && ax < S && ay >= 0 && ay < S && dir >= 0 && dir <= 3;
        if (ok && ((wrow[ay] >> ax) & 1u)) ok = false;  // the agent never stands on a wall
        if (!ok) {  // drawn without the agent and its highlight, MERLIN_DEVERR_BAD_FRAME raised
            ax = ay = -64;
            dir = 0;
        }
        __syncthreads();  // the previous item's pixels are out (s_tid, s_m), the atlas copy is in
        if (threadIdx.x == 0) {
            uint32_t V[7], m[7];
            if (ok) {
                view_mask([&](int y) { return wrow[y]; }, S, ax, ay, dir, V, m);
            } else {
#pragma unroll
                for (int j = 0; j < 7; j++) m[j] = 0u;
                if (slab == 0) atomicOr(A.err, MERLIN_DEVERR_BAD_FRAME);
            }
#pragma unroll
            for (int j = 0; j < 7; j++) s_m[j] = m[j];
            s_m[7] = ok ? 1u : 0u;
        }
        __syncthreads();
        // -- cell -> atlas tile -----------------------------------------------------------------------------------
        {
            const int Fx = (dir == 0) - (dir == 2), Fy = (dir == 1) - (dir == 3);
            const int Rx = -Fy, Ry = Fx;
            for (int c = threadIdx.x; c < S * S; c += RB) {
                const int j = c / S, i = c - j * S;
                const bool wall = (wrow[j] >> i) & 1u;
                const bool goal = !wall && i == gx && j == gy;
                const int dx = i - ax, dy = j - ay;
                const int vj = 6 - (dx * Fx + dy * Fy), vi = 3 + (dx * Rx + dy * Ry);
                const bool vis = ok && vi >= 0 && vi < 7 && vj >= 0 && vj < 7 && ((s_m[vj < 0 || vj > 6 ? 0 : vj] >> (vi & 7)) & 1u);
                const int hl = (A.highlight && vis) ? 1 : 0;
                const int obj = wall ? 1 : (goal ? 2 : 0);
                const bool here = ok && dx == 0 && dy == 0;
                s_tid[c] = (uint8_t)(here ? PLAIN + (((goal ? 4 : 0) + dir) * 2 + hl) : obj + 3 * hl);
            }
        }
        __syncthreads();
        // -- pixels -----------------------------------------------------------------------------------------------
        uint8_t *base = A.out + f * (int64_t)FB;
        int head = (int)((16u - (uint32_t)(reinterpret_cast<uintptr_t>(base) & 15u)) & 15u);
        if (head > FB) head = FB;
        const int nchunks = (FB - head) >> 4;
        const int tail = FB - head - (nchunks << 4);
        auto byte_at = [&](int o) -> uint8_t {  // frame byte o, 0 <= o < FB
            int r, py, q;
            const int y = divmod(o, rowb, A.inv_row, r);
            const int j = divmod(y, ts, A.inv_ts, py);
            const int i = divmod(r, ts3, A.inv_ts3, q);
            const int t = s_tid[j * S + i];
            const int off = (t * ts + py) * ts3 + q;
            return t < PLAIN ? s_atlas8[off] : A.atlas[off];
        };
        if (slab == 0 && (int)threadIdx.x < head) base[threadIdx.x] = byte_at(threadIdx.x);
        if (slab == A.slabs - 1 && (int)threadIdx.x < tail)
            base[head + (nchunks << 4) + threadIdx.x] = byte_at(head + (nchunks << 4) + threadIdx.x);
        uint4 *body = reinterpret_cast<uint4 *>(base + head);
        const bool words = ((ts & 3) == 0) && ((head & 3) == 0);
        // the frame's slabs interleave in stripes of RB chunks (4 KB)
        for (int c = slab * RB + threadIdx.x; c < nchunks; c += A.slabs * RB) {
            int r, py, q;
            const int y = divmod(head + (c << 4), rowb, A.inv_row, r);
            int j = divmod(y, ts, A.inv_ts, py);
            int i = divmod(r, ts3, A.inv_ts3, q);
            uint32_t w[4];
            if (words) {
                int t = s_tid[j * S + i];
                int off = (t * ts + py) * ts3 + q;
                if (q + 16 <= ts3 && (off & 15) == 0) {  // one tile row, on a 16-B boundary of the atlas
                    body[c] = t < PLAIN ? s_atlas4[off >> 4] : reinterpret_cast<const uint4 *>(A.atlas)[off >> 4];
                    continue;
                }
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    w[k] = t < PLAIN ? s_atlas32[off >> 2] : g_atlas32[off >> 2];
                    q += 4;
                    off += 4;
                    if (q == ts3) {  // next tile of the pixel row, or the next pixel row's first
                        q = 0;
                        if (++i == S) {
                            i = 0;
                            if (++py == ts) {
                                py = 0;
                                j++;
                            }
                        }
                        if (k < 3) {  // (the chunk's last word may end the frame: no tile follows)
                            t = s_tid[j * S + i];
                            off = (t * ts + py) * ts3;
                        }
                    }
                }
            } else {
                int t = s_tid[j * S + i];
                int off = (t * ts + py) * ts3 + q;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    uint32_t v = 0u;
#pragma unroll
                    for (int b = 0; b < 4; b++) {
                        v |= (uint32_t)(t < PLAIN ? s_atlas8[off] : A.atlas[off]) << (8 * b);
                        q++;
                        off++;
                        if (q == ts3) {
                            q = 0;
                            if (++i == S) {
                                i = 0;
                                if (++py == ts) {
                                    py = 0;
                                    j++;
                                }
                            }
                            if (k * 4 + b < 15) {
                                t = s_tid[j * S + i];
                                off = (t * ts + py) * ts3;
                            }
                        }
                    }
                    w[k] = v;
                }
            }
            body[c] = make_uint4(w[0], w[1], w[2], w[3]);
        }
    }
}

// merlin_env_snapshot: env i's state in merlin_render_frames' layouts
__global__ __launch_bounds__(256) void k_env_snapshot(const uint32_t *__restrict__ walls, const uint4 *__restrict__ agent,
                                                      int n, int S, int sp, uint32_t *__restrict__ walls_out,
                                                      int32_t *__restrict__ goal_out, int32_t *__restrict__ agent_out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (walls_out)
        for (int y = 0; y < S; y++) walls_out[(int64_t)i * S + y] = walls[(int64_t)i * sp + y];
    const uint4 a = agent[i];
    if (goal_out) {
        goal_out[2 * (int64_t)i] = a.z & 0xff;
        goal_out[2 * (int64_t)i + 1] = (a.z >> 8) & 0xff;
    }
    if (agent_out)
        reinterpret_cast<int4 *>(agent_out)[i] = make_int4(a.x & 0xff, (a.x >> 8) & 0xff, (a.x >> 16) & 3, 0);
}

hipError_t launch(RenderArgs &A, hipStream_t s) {
    if (A.n_frames <= 0) return hipSuccess;
    const int ts3 = 3 * A.ts, rowb = A.S * ts3;
    const int64_t chunks = (int64_t)rowb * A.S * A.ts / 16;
    // enough items to fill the device, each at least ~1024 chunks (4 stores per thread): the per-item set-up (state
    // loads, one lane's mask, the tile table: a few microseconds) is paid once per slab
    int64_t slabs = (MAX_BLOCKS + A.n_frames - 1) / A.n_frames;
    slabs = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(slabs, chunks / 1024), 64));
    A.slabs = (int)slabs;
    A.inv_row = 1.0f / (float)rowb;
    A.inv_ts = 1.0f / (float)A.ts;
    A.inv_ts3 = 1.0f / (float)ts3;
    const int grid = (int)std::min<int64_t>(A.n_frames * slabs, MAX_BLOCKS);
    hipLaunchKernelGGL(k_render_frames, dim3(grid), dim3(RB), 0, s, A);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_render_frames(const uint32_t *walls, const int32_t *goal, const int32_t *agent,
                                const int32_t *map_index, int64_t n_frames, int size, int ts, int highlight,
                                const uint8_t *atlas, uint8_t *out, uint32_t *err, hipStream_t s) {
    RenderArgs A{};
    A.walls = walls;
    A.wall_stride = size;
    A.goal = goal;
    A.agent = agent;
    A.map_index = map_index;
    A.n_frames = n_frames;
    A.S = size;
    A.ts = ts;
    A.highlight = highlight ? 1 : 0;
    A.atlas = atlas;
    A.out = out;
    A.err = err;
    return launch(A, s);
}

hipError_t launch_env_render(const EnvDev &E, const int64_t *index, int64_t n_frames, int ts, int highlight,
                             const uint8_t *atlas, uint8_t *out, hipStream_t s) {
    RenderArgs A{};
    A.walls = E.walls;
    A.wall_stride = E.sp;
    A.env_agent = E.agent;
    A.env_index = index;
    A.n_envs = E.n;
    A.n_frames = n_frames;
    A.S = E.size;
    A.ts = ts;
    A.highlight = highlight ? 1 : 0;
    A.atlas = atlas;
    A.out = out;
    A.err = E.err;
    return launch(A, s);
}

hipError_t launch_env_snapshot(const EnvDev &E, uint32_t *walls, int32_t *goal, int32_t *agent, hipStream_t s) {
    hipLaunchKernelGGL(k_env_snapshot, dim3((E.n + 255) / 256), dim3(256), 0, s, E.walls, E.agent, E.n, E.size, E.sp,
                       walls, goal, agent);
    return hipGetLastError();
}

}  // namespace merlin
