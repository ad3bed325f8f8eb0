// merlin_level_edit.hip -- level editing (merlin_levels_mutate): child c of generation g is its parent
// after `edits` random edits, with the length of its shortest action sequence and whether anything changed.
//
// The edit rule (include/merlin_hip.h has the contract): edit e of child c draws u_j = uniform01(seed, g, e, c, j),
// j = 0..2; kind = min(floor(4 u_0), 3); the cell is interior cell n = min(floor(u_1 (S-2)^2), (S-2)^2 - 1), (x, y) =
// (1 + n % (S-2), 1 + n / (S-2)).  Kind 0, 1: toggle the wall bit unless the cell is the agent's or the goal's.  Kind
// 2: the goal moves there unless it is a wall, the agent's cell or the goal's own.  Kind 3: the agent moves there with
// dir = min(floor(4 u_2), 3) unless it is a wall or the goal's cell.
//
// Layout, as k_shortest_paths (merlin_paths.hip): one child per 32 lanes (two per wave), lane y holds row y.  Every
// lane of a half wave computes the same three uniforms -- the draw is a pure function of its key -- so the only value
// that crosses lanes in the edit loop is the edited cell's wall bit, read by __shfl from lane y.  A toggle is applied by
// the lane that holds the row; the goal and the pose live in every lane's registers.  The backward layer search then
// runs on the edited rows: no LDS, no barrier, no atomic.  row_mask and layer_seed are merlin_grid.h's; the layer step
// is written out.  The half of the last wave that has no child computes on a clamped index and stores
// nothing.  A parent index outside [0, P) loads nothing: the child is zeros, dist -1, changed 0.
#include "merlin_internal.h"
#include "merlin_grid.h"

#include <vector>

namespace merlin {
namespace {

using namespace grid;

constexpr int MBLK = 256;  // 8 children per block
constexpr int MCH = MBLK / 32;

struct MutateArgs {
    const uint32_t *walls;  // parents: uint32[P][S]
    const int32_t *goal;    // int32[P][2]
    const int32_t *agent;   // int32[P][4]
    int64_t P;
    const int32_t *parent;  // int32[C], null: child c edits parent c
    int64_t C;
    int S, edits;
    uint64_t seed, generation;
    uint32_t *out_walls;
    int32_t *out_goal, *out_agent, *dist;
    uint8_t *changed;
};

// one edit's draws, shared by the kernel and the host restatement (as level_draw is)
struct EditDraw {
    int kind, x, y, dir;
};
__host__ __device__ __forceinline__ EditDraw edit_draw(uint64_t seed, uint64_t gen, int e, uint64_t c, int S) {
    const double u0 = uniform01(seed, gen, (uint64_t)e, c, 0);
    const double u1 = uniform01(seed, gen, (uint64_t)e, c, 1);
    const double u2 = uniform01(seed, gen, (uint64_t)e, c, 2);
    const int in = S - 2;
    const int64_t cells = (int64_t)in * in;
    int64_t n = (int64_t)floor(u1 * (double)cells);
    if (n > cells - 1) n = cells - 1;
    int kind = (int)floor(u0 * 4.0), dir = (int)floor(u2 * 4.0);
    if (kind > 3) kind = 3;
    if (dir > 3) dir = 3;
    return EditDraw{kind, 1 + (int)(n % in), 1 + (int)(n / in), dir};
}

__global__ __launch_bounds__(MBLK) void k_levels_mutate(MutateArgs A) {
    const int y = threadIdx.x & 31;
    const int64_t c0 = (int64_t)blockIdx.x * MCH + (threadIdx.x >> 5);
    const bool live = c0 < A.C;
    const int64_t c = live ? c0 : A.C - 1;  // a child-less half wave computes a copy of the last child, stores nothing
    const int S = A.S;
    const int half = threadIdx.x & 32;  // bit offset of this child's lanes in a wave-wide ballot

    const int64_t p = A.parent ? (int64_t)A.parent[c] : c;
    const bool valid = p >= 0 && p < A.P;
    uint32_t row = 0u;
    int gx = 0, gy = 0, ax = 0, ay = 0, dir = 0, a3 = 0;
    if (valid) {
        if (y < S) row = A.walls[p * S + y];
        gx = A.goal[2 * p];
        gy = A.goal[2 * p + 1];
        ax = A.agent[4 * p];
        ay = A.agent[4 * p + 1];
        dir = A.agent[4 * p + 2];
        a3 = A.agent[4 * p + 3];
    }
    const uint32_t row0 = row;
    const int gx0 = gx, gy0 = gy, ax0 = ax, ay0 = ay, dir0 = dir;

    for (int e = 0; e < A.edits; e++) {
        const EditDraw d = edit_draw(A.seed, A.generation, e, (uint64_t)c, S);
        const bool wall = ((uint32_t)__shfl((int)row, d.y, 32) >> d.x) & 1u;  // d.y in [1, S - 2]: a lane of this half
        const bool at_agent = d.x == ax && d.y == ay, at_goal = d.x == gx && d.y == gy;
        if (d.kind <= 1) {
            if (valid && !at_agent && !at_goal && y == d.y) row ^= 1u << d.x;
        } else if (d.kind == 2) {
            if (valid && !wall && !at_agent && !at_goal) {
                gx = d.x;
                gy = d.y;
            }
        } else if (valid && !wall && !at_goal) {
            ax = d.x;
            ay = d.y;
            dir = d.dir;
        }
    }
    const uint32_t rows_differ = (uint32_t)(__ballot(row != row0) >> half);
    const bool changed = rows_differ != 0u || gx != gx0 || gy != gy0 || ax != ax0 || ay != ay0 || dir != dir0;

    // the backward layer search of k_shortest_paths on the edited rows, without a field
    const uint32_t full = row_mask(S);
    const uint32_t free_ = y < S ? ~row & full : 0u;
    const Goal g = goal_at(gx, gy, S);
    const bool agent_ok = valid && ax >= 0 && ax < S && ay >= 0 && ay < S && dir >= 0 && dir < 4;
    const uint32_t abit = (agent_ok && y == ay) ? 1u << ax : 0u;
    uint32_t F[4], V[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int d = 0; d < 4; d++) F[d] = layer_seed(g, S, d, y, free_);
    int res = -1;
    const int kmax = 4 * S * S;
    for (int k = 1; k <= kmax; k++) {
        const uint32_t fa = dir == 0 ? F[0] : dir == 1 ? F[1] : dir == 2 ? F[2] : F[3];
        if (fa & abit) res = k;
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
        const uint32_t found = (uint32_t)(__ballot(res >= 0) >> half);
        const bool more = (F[0] | F[1] | F[2] | F[3]) != 0u && agent_ok && found == 0u;
        if (!__any(more)) break;
    }
    const int r = __shfl(res, agent_ok ? ay : 0, 32);

    if (!live) return;
    if (y < S) A.out_walls[c0 * S + y] = row;
    if (y == 0) {
        A.out_goal[2 * c0] = gx;
        A.out_goal[2 * c0 + 1] = gy;
        A.out_agent[4 * c0] = ax;
        A.out_agent[4 * c0 + 1] = ay;
        A.out_agent[4 * c0 + 2] = dir;
        A.out_agent[4 * c0 + 3] = a3;
        A.dist[c0] = r;
        A.changed[c0] = changed ? 1 : 0;
    }
}

}  // namespace

hipError_t launch_levels_mutate(const uint32_t *walls, const int32_t *goal, const int32_t *agent, int64_t P,
                                const int32_t *parent, int64_t C, int size, int edits, uint64_t seed,
                                uint64_t generation, uint32_t *out_walls, int32_t *out_goal, int32_t *out_agent,
                                int32_t *dist, uint8_t *changed, hipStream_t s) {
    if (C <= 0) return hipSuccess;
    const MutateArgs A{walls, goal, agent, P, parent, C, size, edits, seed, generation,
                       out_walls, out_goal, out_agent, dist, changed};
    hipLaunchKernelGGL(k_levels_mutate, dim3((unsigned)((C + MCH - 1) / MCH)), dim3(MBLK), 0, s, A);
    return hipGetLastError();
}

// The same on host arrays, one child after another: the edits on a copy of the parent, then the library's queue
// search (shortest_paths_host) on the children.  No device code.
void levels_mutate_host(const uint32_t *walls, const int32_t *goal, const int32_t *agent, int64_t P,
                        const int32_t *parent, int64_t C, int S, int edits, uint64_t seed, uint64_t generation,
                        uint32_t *out_walls, int32_t *out_goal, int32_t *out_agent, int32_t *dist, uint8_t *changed) {
    std::vector<uint8_t> valid((size_t)C);
    for (int64_t c = 0; c < C; c++) {
        const int64_t p = parent ? (int64_t)parent[c] : c;
        uint32_t *w = out_walls + c * S;
        int32_t *g = out_goal + 2 * c, *a = out_agent + 4 * c;
        valid[c] = p >= 0 && p < P;
        if (!valid[c]) {
            for (int y = 0; y < S; y++) w[y] = 0u;
            g[0] = g[1] = 0;
            a[0] = a[1] = a[2] = a[3] = 0;
            changed[c] = 0;
            continue;
        }
        for (int y = 0; y < S; y++) w[y] = walls[p * S + y];
        for (int j = 0; j < 2; j++) g[j] = goal[2 * p + j];
        for (int j = 0; j < 4; j++) a[j] = agent[4 * p + j];
        for (int e = 0; e < edits; e++) {
            const EditDraw d = edit_draw(seed, generation, e, (uint64_t)c, S);
            const bool wall = (w[d.y] >> d.x) & 1u;
            const bool at_agent = d.x == a[0] && d.y == a[1], at_goal = d.x == g[0] && d.y == g[1];
            if (d.kind <= 1) {
                if (!at_agent && !at_goal) w[d.y] ^= 1u << d.x;
            } else if (d.kind == 2) {
                if (!wall && !at_agent && !at_goal) g[0] = d.x, g[1] = d.y;
            } else if (!wall && !at_goal) {
                a[0] = d.x, a[1] = d.y, a[2] = d.dir;
            }
        }
        bool ch = g[0] != goal[2 * p] || g[1] != goal[2 * p + 1];
        for (int j = 0; j < 3; j++) ch = ch || a[j] != agent[4 * p + j];
        for (int y = 0; y < S; y++) ch = ch || w[y] != walls[p * S + y];
        changed[c] = ch ? 1 : 0;
    }
    shortest_paths_host(out_walls, out_goal, out_agent, C, S, dist, nullptr);
    for (int64_t c = 0; c < C; c++)
        if (!valid[c]) dist[c] = -1;
}

}  // namespace merlin
