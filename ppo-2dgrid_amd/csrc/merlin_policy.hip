// merlin_policy.hip -- the policy field's two kernels: the observation of any pose of any map, and
// the number of actions after which a deterministic policy's episode terminates, from every pose of a map at once.
//
// k_view_codes: the 8 nibble words merlin_env_reset / merlin_env_step write for an env in that state, without an env.
// One thread per query.  The intended use lists every free pose of M maps in (map, dir, y, x) order, so the 64 queries
// of a wave stand on two or three neighbouring grid rows of one map: the 7 row words a lane's window needs are the
// same 9 or so words for the whole wave, one or two cache lines that the lanes read as broadcasts.  A block per map
// with its rows in LDS would save those (cached) loads and cost a pass to find each map's queries, which map_index
// does not have to keep together; a query is a few hundred integer instructions and 32 B out either way.
//
// k_policy_paths: every pose takes its own action, so a map is a functional graph over its 4 S^2 poses, and steps(p)
// is the depth of p in the tree that hangs from the terminating poses (the free poses in front of the goal whose
// action is forward); a pose on or leading to a cycle, a forward move into a wall or an action outside {0, 1, 2} has
// none: -1.  It is k_shortest_paths' backward search (merlin_paths.hip: 32 lanes per map, lane y holds row y, the
// frontier and visited masks per direction in registers, the vertical moves by shuffles; the pieces around the
// layer step are merlin_grid.h's) with an edge kept only where the predecessor's action takes it: per direction three
// masks L / R / W of the poses that turn left / turn right / move forward, built by the lane from its row of action
// bytes,
//   layer 1            F[d] = bit(goal - vec(d)) & free & W[d]
//   layer k -> k + 1   N[d] = ((F[(d + 3) & 3] & L[d]) | (F[(d + 1) & 3] & R[d]) | (back_d(F[d]) & W[d])) & free & ~V[d]
// A pose has one successor, so it enters at most one layer -- but for the forward-acting pose in front of the goal,
// whose front cell also holds a pose (the goal cell is an ordinary cell to stand on): ~V[d] keeps it in layer 1.
#include "merlin_internal.h"
#include "merlin_grid.h"

#include <vector>

namespace merlin {
namespace {

using namespace grid;

constexpr int VBLK = 256;

__global__ __launch_bounds__(VBLK) void k_view_codes(const uint32_t *__restrict__ walls,
                                                      const int32_t *__restrict__ goal,
                                                      const int32_t *__restrict__ agent,
                                                      const int32_t *__restrict__ map_index, int64_t n, int S,
                                                      uint32_t *__restrict__ codes, int wide, uint32_t *err) {
    const int64_t q = (int64_t)blockIdx.x * VBLK + threadIdx.x;
    if (q >= n) return;
    const int64_t m = map_index ? (int64_t)map_index[q] : q;
    const int ax = agent[4 * q], ay = agent[4 * q + 1], dir = agent[4 * q + 2];
    const uint32_t *wrow = walls + m * S;
    bool ok = in_grid(S, ax, ay) && dir >= 0 && dir <= 3;
    if (ok && ((wrow[ay] >> ax) & 1u)) ok = false;  // no env stands on a wall
    uint32_t out[MERLIN_OBS_WORDS];
#pragma unroll
    for (int w = 0; w < MERLIN_OBS_WORDS; w++) out[w] = 0u;
    if (ok) {
        int gx = -1, gy = -1;
        if (goal) {
            gx = goal[2 * m];
            gy = goal[2 * m + 1];
        }
        const Goal g = goal_at(gx, gy, S);
        uint32_t V[7], vis[7];
        view_mask([&](int y) { return wrow[y]; }, S, ax, ay, dir, V, vis);
        // the goal's view cell: view (vi, vj) shows world agent + (6 - vj) F + (vi - 3) R
        const int Fx = dir_x(dir), Fy = dir_y(dir);
        const int Rx = -Fy, Ry = Fx;
        const int dx = g.gx - ax, dy = g.gy - ay;
        const int gvj = 6 - (dx * Fx + dy * Fy), gvi = 3 + (dx * Rx + dy * Ry);
        const bool ginv = g.in && gvi >= 0 && gvi < 7 && gvj >= 0 && gvj < 7;
        // tile classes: 0 not visible, 1 empty, 2 wall, 3 goal, 4 the agent's own cell (3, 6); nibble vj * 7 + vi
#pragma unroll
        for (int j = 0; j < 7; j++) {
            const uint32_t seen = vis[j], wl = V[j] & seen;
            const uint32_t gl = (ginv && gvj == j) ? (1u << gvi) & seen & ~wl : 0u;
#pragma unroll
            for (int i = 0; i < 7; i++) {
                const int k = j * 7 + i;
                const uint32_t c = (i == 3 && j == 6) ? 4u
                                                      : ((seen >> i) & 1u) + ((wl >> i) & 1u) + 2u * ((gl >> i) & 1u);
                out[k >> 3] |= c << ((k & 7) * 4);
            }
        }
    } else {
        atomicOr(err, MERLIN_DEVERR_BAD_FRAME);
    }
    uint32_t *dst = codes + q * MERLIN_OBS_WORDS;
    if (wide) {  // a 16-B aligned output (uniform): two 128-bit stores
        reinterpret_cast<uint4 *>(dst)[0] = make_uint4(out[0], out[1], out[2], out[3]);
        reinterpret_cast<uint4 *>(dst)[1] = make_uint4(out[4], out[5], out[6], out[7]);
    } else {
#pragma unroll
        for (int w = 0; w < MERLIN_OBS_WORDS; w++) dst[w] = out[w];
    }
}

constexpr int PBLK = 256;  // 8 maps per block, as k_shortest_paths
constexpr int PMAPS = PBLK / 32;

__global__ __launch_bounds__(PBLK) void k_policy_paths(const uint32_t *__restrict__ walls,
                                                        const int32_t *__restrict__ goal,
                                                        const int8_t *__restrict__ action, int64_t n, int S,
                                                        int16_t *__restrict__ steps) {
    const int y = threadIdx.x & 31;
    const int64_t m0 = (int64_t)blockIdx.x * PMAPS + (threadIdx.x >> 5);
    const bool live = m0 < n;
    const int64_t m = live ? m0 : n - 1;  // a map-less half wave computes a copy of the last map, stores nothing
    const bool row = y < S;
    const uint32_t full = row_mask(S);
    const uint32_t free_ = row ? ~walls[m * S + y] & full : 0u;
    const Goal g = goal_of(goal, m, S);

    // this lane's rows: the action masks read, the field set to -1 (overwritten below by the same lane)
    uint32_t L[4], R[4], W[4];
    int16_t *srow[4] = {nullptr, nullptr, nullptr, nullptr};
    const bool st = live && row;
#pragma unroll
    for (int d = 0; d < 4; d++) {
        L[d] = R[d] = W[d] = 0u;
        if (row) {
            const int64_t o = ((m * 4 + d) * S + y) * (int64_t)S;
            const int8_t *arow = action + o;
            for (int x = 0; x < S; x++) {
                const int a = arow[x];
                L[d] |= (uint32_t)(a == 0) << x;
                R[d] |= (uint32_t)(a == 1) << x;
                W[d] |= (uint32_t)(a == 2) << x;
            }
            if (st) {
                srow[d] = steps + o;
                for (int x = 0; x < S; x++) srow[d][x] = (int16_t)-1;
            }
        }
    }

    // layer 1: the cell goal - vec(d) where the action is forward
    uint32_t F[4], V[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int d = 0; d < 4; d++) F[d] = layer_seed(g, S, d, y, free_ & W[d]);

    const int kmax = 4 * S * S;
    for (int k = 1; k <= kmax; k++) {
        if (st) {
#pragma unroll
            for (int d = 0; d < 4; d++) store_layer(srow[d], F[d], k);
        }
#pragma unroll
        for (int d = 0; d < 4; d++) V[d] |= F[d];
        const uint32_t dn = (uint32_t)__shfl_down((int)F[1], 1, 32);  // row y + 1's frontier
        const uint32_t up = (uint32_t)__shfl_up((int)F[3], 1, 32);    // row y - 1's
        uint32_t N[4];
        N[0] = ((F[3] & L[0]) | (F[1] & R[0]) | ((F[0] >> 1) & W[0])) & free_ & ~V[0];
        N[1] = ((F[0] & L[1]) | (F[2] & R[1]) | ((y < 31 ? dn : 0u) & W[1])) & free_ & ~V[1];
        N[2] = ((F[1] & L[2]) | (F[3] & R[2]) | ((F[2] << 1) & W[2])) & free_ & ~V[2];
        N[3] = ((F[2] & L[3]) | (F[0] & R[3]) | ((y > 0 ? up : 0u) & W[3])) & free_ & ~V[3];
#pragma unroll
        for (int d = 0; d < 4; d++) F[d] = N[d];
        // every lane of the wave stays until both of its maps' frontiers are empty (the shuffles read neighbours)
        if (!__any((F[0] | F[1] | F[2] | F[3]) != 0u)) break;
    }
}

}  // namespace

hipError_t launch_view_codes(const uint32_t *walls, const int32_t *goal, const int32_t *agent,
                             const int32_t *map_index, int64_t n, int size, uint32_t *codes, uint32_t *err,
                             hipStream_t s) {
    if (n <= 0) return hipSuccess;
    const int64_t blocks = (n + VBLK - 1) / VBLK;
    const int wide = (reinterpret_cast<uintptr_t>(codes) & 15u) == 0;
    hipLaunchKernelGGL(k_view_codes, dim3((unsigned)blocks), dim3(VBLK), 0, s, walls, goal, agent, map_index, n, size,
                       codes, wide, err);
    return hipGetLastError();
}

hipError_t launch_policy_paths(const uint32_t *walls, const int32_t *goal, const int8_t *action, int64_t n_maps,
                               int size, int16_t *steps, hipStream_t s) {
    if (n_maps <= 0) return hipSuccess;
    const int64_t blocks = (n_maps + PMAPS - 1) / PMAPS;
    hipLaunchKernelGGL(k_policy_paths, dim3((unsigned)blocks), dim3(PBLK), 0, s, walls, goal, action, n_maps, size,
                       steps);
    return hipGetLastError();
}

// The same field on host arrays by the opposite route: a forward walk from every pose along its own actions, with
// memoisation.  state[p]: UNSEEN, ON_PATH (on the walk in progress: meeting it again closes a cycle) or the pose's
// answer.  A walk stops at a terminating action (1), a dead end (-1: a wall pose, an action outside {0, 1, 2}, a
// forward move into a wall or off the grid), an answered pose or its own path (-1), and unwinds: answer + 1, or -1.
void policy_paths_host(const uint32_t *walls, const int32_t *goal, const int8_t *action, int64_t n_maps, int S,
                       int16_t *steps) {
    using namespace grid_host;
    constexpr int UNSEEN = -2, ON_PATH = -3;
    const int P = 4 * S * S;
    std::vector<int> state(P), path;
    path.reserve(P);
    for (int64_t m = 0; m < n_maps; m++) {
        const MapView mv{walls + m * S, S};
        const int8_t *act = action + m * P;
        const int gx = goal[2 * m], gy = goal[2 * m + 1];
        std::fill(state.begin(), state.end(), UNSEEN);
        for (int p0 = 0; p0 < P; p0++) {
            if (state[p0] != UNSEEN) continue;
            path.clear();
            int p = p0, tail;  // tail: the answer of the pose after the path's last
            for (;;) {
                if (state[p] == ON_PATH) {
                    tail = -1;
                    break;
                }
                if (state[p] != UNSEEN) {
                    tail = state[p];
                    break;
                }
                int d, y, x;
                mv.decode(p, d, y, x);
                const int a = act[p];
                state[p] = ON_PATH;
                path.push_back(p);
                if (!mv.is_free(x, y) || a < 0 || a > 2) {
                    tail = -2;  // the pose itself is the dead end: -1 after the unwind's + 1
                    break;
                }
                if (a == 2) {
                    const int fx = x + DX[d], fy = y + DY[d];
                    if (!mv.is_free(fx, fy)) {
                        tail = -2;
                        break;
                    }
                    if (fx == gx && fy == gy) {
                        tail = 0;
                        break;
                    }
                    p = mv.pose(d, fy, fx);
                } else {
                    p = mv.pose((a == 0 ? d + 3 : d + 1) & 3, y, x);
                }
            }
            for (size_t i = path.size(); i-- > 0;) {
                tail = tail < 0 ? -1 : tail + 1;
                state[path[i]] = tail;
            }
        }
        for (int p = 0; p < P; p++) steps[m * P + p] = (int16_t)state[p];
    }
}

}  // namespace merlin
