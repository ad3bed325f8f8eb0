// merlin_paths.hip -- the length of the shortest action sequence to the goal, for every env at once.
//
// The step rule (merlin_env.hip k_env_step): action 0 turns left (dir + 3) & 3, 1 turns right (dir + 1) & 3, 2 moves
// to the front cell unless it is a wall, and the episode terminates on a forward action whose front cell is the goal.
// dist(x, y, d) is the least number of actions after which an episode started in pose (x, y, d) terminates, -1 if
// none does.  It is a breadth-first search over the 4 S^2 poses, run backwards from the goal so that one search
// answers every pose of a map (the field) and the agent's pose is a lookup:
//   layer 1            the free poses whose front cell is the goal: for each d the cell goal - vec(d)
//   layer k -> k + 1   a pose is new in layer k + 1 if one of its three successors is in layer k:
//                      N[d] = (F[(d + 1) & 3] | F[(d + 3) & 3] | back_d(F[d])) & free & ~V[d]
// with back_d the frontier moved one cell against vec(d).  A forward move into a wall is a self loop and adds nothing.
//
// Layout: one env per 32 lanes (two per wave), lane y holds row y: its free mask and, per direction, the visited and
// frontier masks -- 9 words.  back_0 / back_2 are shifts inside the lane, back_1 / back_3 read the lane below / above
// (__shfl_down / __shfl_up with width 32; the edge lanes take 0).  No LDS, no barrier, no atomic.  Every lane of a wave
// stays in the loop until both of its envs are done (the shuffles read neighbouring lanes), and the half of the last
// wave that has no env computes on a clamped index and stores nothing.
// row_mask, layer_seed and store_layer are merlin_grid.h's, shared with k_policy_paths; the layer step is written out.
#include "merlin_internal.h"
#include "merlin_grid.h"

#include <vector>

namespace merlin {
namespace {

using namespace grid;

constexpr int PBLK = 256;            // 8 envs per block
constexpr int PENVS = PBLK / 32;

struct PathArgs {
    const uint32_t *walls;   // row y of map m at walls[m * wstride + y]
    int wstride;
    const uint4 *packed;     // the env context's agent words (EnvDev::agent); null: goal / agent below
    const int32_t *goal;     // int32[M][2]
    const int32_t *agent;    // int32[n][4] = x, y, dir, 0
    const int32_t *map_index;
    int64_t n;
    int S;
    int32_t *dist;
    int16_t *field;          // nullable: int16[n][4][S][S]
};

__global__ __launch_bounds__(PBLK) void k_shortest_paths(PathArgs A) {
    const int y = threadIdx.x & 31;
    const int64_t q0 = (int64_t)blockIdx.x * PENVS + (threadIdx.x >> 5);
    const bool live = q0 < A.n;
    const int64_t q = live ? q0 : A.n - 1;  // an env-less half wave computes a copy of the last env, stores nothing
    const int S = A.S;

    int ax, ay, dir, gx, gy;
    int64_t m = q;
    if (A.packed) {
        const uint4 st = A.packed[q];
        ax = st.x & 0xff;
        ay = (st.x >> 8) & 0xff;
        dir = (st.x >> 16) & 3;
        gx = st.z & 0xff;
        gy = (st.z >> 8) & 0xff;
    } else {
        if (A.map_index) m = A.map_index[q];
        ax = A.agent[4 * q];
        ay = A.agent[4 * q + 1];
        dir = A.agent[4 * q + 2];
        gx = A.goal[2 * m];
        gy = A.goal[2 * m + 1];
    }
    const uint32_t full = row_mask(S);
    const uint32_t free_ = y < S ? ~A.walls[m * A.wstride + y] & full : 0u;
    const Goal g = goal_at(gx, gy, S);
    const bool agent_ok = ax >= 0 && ax < S && ay >= 0 && ay < S && dir >= 0 && dir < 4;
    const bool mine = agent_ok && y == ay;  // the lane that holds the agent's row
    const uint32_t abit = mine ? 1u << ax : 0u;

    // this lane's rows of the field: -1 first, overwritten below by the same lane (program order, no fill pass)
    int16_t *frow[4] = {nullptr, nullptr, nullptr, nullptr};
    const bool fld = A.field && live && y < S;
    if (fld) {
#pragma unroll
        for (int d = 0; d < 4; d++) {
            frow[d] = A.field + (((q * 4 + d) * S + y) * (int64_t)S);
            for (int x = 0; x < S; x++) frow[d][x] = (int16_t)-1;
        }
    }

    uint32_t F[4], V[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int d = 0; d < 4; d++) F[d] = layer_seed(g, S, d, y, free_);

    int res = -1;
    const int half = threadIdx.x & 32;  // bit offset of this env's lanes in a wave-wide ballot
    const int kmax = 4 * S * S;
    for (int k = 1; k <= kmax; k++) {
        const uint32_t fa = dir == 0 ? F[0] : dir == 1 ? F[1] : dir == 2 ? F[2] : F[3];
        if (fa & abit) res = k;
        if (fld) {
#pragma unroll
            for (int d = 0; d < 4; d++) store_layer(frow[d], F[d], k);
        }
#pragma unroll
        for (int d = 0; d < 4; d++) V[d] |= F[d];
        const uint32_t dn = (uint32_t)__shfl_down((int)F[1], 1, 32);  // row y + 1's frontier
        const uint32_t up = (uint32_t)__shfl_up((int)F[3], 1, 32);    // row y - 1's
        uint32_t N[4];
        N[0] = (F[1] | F[3] | (F[0] >> 1)) & free_ & ~V[0];
        N[1] = (F[2] | F[0] | (y < 31 ? dn : 0u)) & free_ & ~V[1];
        N[2] = (F[3] | F[1] | (F[2] << 1)) & free_ & ~V[2];
        N[3] = (F[0] | F[2] | (y > 0 ? up : 0u)) & free_ & ~V[3];
#pragma unroll
        for (int d = 0; d < 4; d++) F[d] = N[d];
        // an env is done when its frontier is empty, or, with no field asked for, when its agent has its answer
        bool more = (F[0] | F[1] | F[2] | F[3]) != 0u;
        if (!A.field) {
            const uint32_t found = (uint32_t)(__ballot(res >= 0) >> half);
            more = more && agent_ok && found == 0u;
        }
        if (!__any(more)) break;
    }
    if (live && A.dist) {
        const int r = __shfl(res, agent_ok ? ay : 0, 32);
        if (y == 0) A.dist[q] = r;
    }
}

hipError_t launch(const PathArgs &A, hipStream_t s) {
    if (A.n <= 0) return hipSuccess;
    const int64_t blocks = (A.n + PENVS - 1) / PENVS;
    hipLaunchKernelGGL(k_shortest_paths, dim3((unsigned)blocks), dim3(PBLK), 0, s, A);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_shortest_paths(const uint32_t *walls, const int32_t *goal, const int32_t *agent,
                                 const int32_t *map_index, int64_t n, int size, int32_t *dist, int16_t *field,
                                 hipStream_t s) {
    PathArgs A{walls, size, nullptr, goal, agent, map_index, n, size, dist, field};
    return launch(A, s);
}

hipError_t launch_env_optimal_steps(const EnvDev &E, int32_t *dist, int16_t *field, hipStream_t s) {
    PathArgs A{E.walls, E.sp, E.agent, nullptr, nullptr, nullptr, (int64_t)E.n, E.size, dist, field};
    return launch(A, s);
}

// The same problem on host arrays, as a queue search: poses are numbered (d * S + y) * S + x, the queue starts with
// the poses in front of the goal and a popped pose relaxes its predecessors -- the two turns into it and, if its own
// cell is where a forward move from behind lands, the pose one cell back.
void shortest_paths_host(const uint32_t *walls, const int32_t *goal, const int32_t *agent, int64_t n, int S,
                         int32_t *dist, int16_t *field) {
    using namespace grid_host;
    const int P = 4 * S * S;
    std::vector<int> dd(P), queue(P);
    for (int64_t q = 0; q < n; q++) {
        const MapView mv{walls + q * S, S};
        std::fill(dd.begin(), dd.end(), -1);
        int head = 0, tail = 0;
        const int gx = goal[2 * q], gy = goal[2 * q + 1];
        if (mv.inside(gx, gy))
            for (int d = 0; d < 4; d++) {
                const int x = gx - DX[d], y = gy - DY[d];
                if (mv.is_free(x, y)) {
                    const int p = mv.pose(d, y, x);
                    dd[p] = 1;
                    queue[tail++] = p;
                }
            }
        while (head < tail) {
            const int p = queue[head++];
            int d, y, x;
            mv.decode(p, d, y, x);
            const int pred[3] = {mv.pose((d + 1) & 3, y, x), mv.pose((d + 3) & 3, y, x),
                                 mv.is_free(x - DX[d], y - DY[d]) ? mv.pose(d, y - DY[d], x - DX[d]) : -1};
            for (int j = 0; j < 3; j++)
                if (pred[j] >= 0 && dd[pred[j]] < 0) {
                    dd[pred[j]] = dd[p] + 1;
                    queue[tail++] = pred[j];
                }
        }
        if (dist) {
            const int ax = agent[4 * q], ay = agent[4 * q + 1], ad = agent[4 * q + 2];
            dist[q] = (ad >= 0 && ad < 4 && mv.is_free(ax, ay)) ? dd[mv.pose(ad, ay, ax)] : -1;
        }
        if (field)
            for (int p = 0; p < P; p++) field[q * P + p] = (int16_t)dd[p];
    }
}

}  // namespace merlin
