// merlin_grid.h -- the grid geometry of the map-analysis kernels (merlin_paths.hip, merlin_policy.hip,
// merlin_chain.hip) and of their host restatements.  Two halves that share nothing: the device half is
// __device__ only, the host half plain C++, so no host restatement checks a kernel with the kernel's own code.
// A map is S rows of wall bits (bit x of row y = wall); directions 0 = +x, 1 = +y, 2 = -x, 3 = -y; action 0 turns
// left (d + 3) & 3, 1 turns right (d + 1) & 3, 2 moves to the front cell; poses are numbered (d * S + y) * S + x.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace merlin {
namespace grid {  // device

__device__ __forceinline__ int dir_x(int d) { return (d == 0) - (d == 2); }
__device__ __forceinline__ int dir_y(int d) { return (d == 1) - (d == 3); }
__device__ __forceinline__ bool in_grid(int S, int x, int y) { return x >= 0 && x < S && y >= 0 && y < S; }

// (x, y) is a cell of the grid and no wall; wrow: the map's rows  (bounds spelled out, as in goal_at: DESIGN.md §6g)
__device__ __forceinline__ bool free_at(const uint32_t *__restrict__ wrow, int S, int x, int y) {
    return x >= 0 && x < S && y >= 0 && y < S && !((wrow[y] >> x) & 1u);
}

struct Goal {
    int gx, gy;
    bool in;  // on the grid: a goal outside it terminates nothing
};
__device__ __forceinline__ Goal goal_at(int gx, int gy, int S) {
    return Goal{gx, gy, gx >= 0 && gx < S && gy >= 0 && gy < S};
}
__device__ __forceinline__ Goal goal_of(const int32_t *__restrict__ goal, int64_t m, int S) {
    return goal_at(goal[2 * m], goal[2 * m + 1], S);
}

// ---- pieces of the backward layer search of k_shortest_paths / k_policy_paths (merlin_paths.hip has the derivation).
// The layer step itself stays written out in each kernel: as a shared function, templated on the action masks, it
// compiled to the same operations in another issue order and cost k_shortest_paths 1 to 2 us.
// the S columns of the grid as a mask: a row's free mask is ~walls & row_mask(S), 0 in a lane with y >= S
__device__ __forceinline__ uint32_t row_mask(int S) { return S >= 32 ? 0xffffffffu : ((1u << S) - 1u); }

// layer 1 of direction d in lane y: the cell goal - vec(d), if free
__device__ __forceinline__ uint32_t layer_seed(const Goal &g, int S, int d, int y, uint32_t free_) {
    const int sx = g.gx - dir_x(d), sy = g.gy - dir_y(d);
    return (g.in && y == sy && sx >= 0 && sx < S) ? (1u << sx) & free_ : 0u;
}

// the set bits of row y of direction d's frontier take the value k
__device__ __forceinline__ void store_layer(int16_t *__restrict__ row, uint32_t f, int k) {
    while (f) {
        const int x = __ffs((int)f) - 1;
        f &= f - 1u;
        row[x] = (int16_t)k;
    }
}

}  // namespace grid

namespace grid_host {  // host: what the restatements (the kernels' oracles) share -- never called from a kernel

inline constexpr int DX[4] = {1, 0, -1, 0}, DY[4] = {0, 1, 0, -1};

struct MapView {
    const uint32_t *w;  // the map's S rows
    int S;
    bool inside(int x, int y) const { return x >= 0 && x < S && y >= 0 && y < S; }
    bool is_free(int x, int y) const { return inside(x, y) && !((w[y] >> x) & 1u); }
    int pose(int d, int y, int x) const { return (d * S + y) * S + x; }
    void decode(int p, int &d, int &y, int &x) const { d = p / (S * S), y = (p / S) % S, x = p % S; }
};

}  // namespace grid_host
}  // namespace merlin
