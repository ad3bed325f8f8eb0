// merlin_chain.hip -- the sampled-policy field's two kernels: a policy that samples from probabilities
// which depend on the view alone turns a map into a time-homogeneous Markov chain over its 4 S^2 poses, and one dynamic
// programme over that chain and the horizon gives what an episode's result is made of, without sampling noise.
//
// k_policy_chain      backwards from the goal, every pose at once: h_t(p) = P(the episode started in p terminates at
//                     exactly action t), accumulated for t = 1..T into success, return, expected length and the
//                     discounted return from step 0.
// k_policy_occupancy  forwards from one start pose per map: mu_t = the distribution over poses after t actions of
//                     the episodes still running, accumulated into the expected visits, and the probability hit[t - 1]
//                     that the episode terminates at action t.
//
// Both: one block per map, one thread per cell; a thread holds its cell's four directions -- the three normalised
// probabilities of each, the state (h or mu) and the accumulators -- in registers, so both turn terms are
// thread-local.  Only the forward term crosses cells, through an LDS image of one double per pose, [dir][cell]:
// lane l reads cell l +- 1 or l +- S of a plane, consecutive doubles for consecutive lanes, so every ds_read_b64 /
// ds_write_b64 of a wave is conflict-free (the bank of a b64 access is (addr / 4) % 64 over a half wave: 32
// consecutive doubles cover the 64 banks once).  The image is double-buffered, [t & 1], which leaves one block
// barrier per step: a thread writes buffer b again two steps later, after the barrier of the step between, which
// every thread reaches only once its reads of b are done.  T steps, no early exit.  The block is the smallest of 256,
// 512 and 1,024 threads that holds S^2 cells (S <= 16, S <= 22, S <= 32): 16, 32 or 64 KiB of LDS.
// Float64 throughout; the file is compiled with -ffp-contract=off like the rest, so the host restatements below, which
// keep the kernels' order of operations inside a term, differ from them by the order of a pose's incoming terms only.
// Grid geometry (direction vectors, free_at, the goal; the host's map view and pose numbering) is merlin_grid.h's.
#include "merlin_internal.h"
#include "merlin_grid.h"

#include <algorithm>
#include <limits>
#include <type_traits>
#include <vector>

namespace merlin {
namespace {

using namespace grid;

// What a thread knows of its cell: (x, y) and whether it is a free cell of the grid.
struct Cell {
    int x, y;
    bool live;
};

__device__ __forceinline__ Cell cell_of(const uint32_t *__restrict__ wrow, int S, int c) {
    Cell k;
    k.y = c / S;
    k.x = c - k.y * S;
    k.live = c < S * S && !((wrow[k.y < S ? k.y : 0] >> k.x) & 1u);
    return k;
}

// a pose's three probabilities, widened and normalised (float32 softmax rows do not sum to 1)
__device__ __forceinline__ void load_probs(const float *__restrict__ p, double &qL, double &qR, double &qF) {
    const double p0 = (double)p[0], p1 = (double)p[1], p2 = (double)p[2];
    const double s = (p0 + p1) + p2;
    qL = p0 / s;
    qR = p1 / s;
    qF = p2 / s;
}

template <int BLK>
__global__ __launch_bounds__(BLK) void k_policy_chain(const uint32_t *__restrict__ walls,
                                                       const int32_t *__restrict__ goal,
                                                       const float *__restrict__ probs, int S, int T, double gamma,
                                                       double *__restrict__ success, double *__restrict__ ret,
                                                       double *__restrict__ steps, double *__restrict__ disc) {
    __shared__ double hb[2][4 * BLK];
    const int64_t m = blockIdx.x;
    const int c = threadIdx.x, cells = S * S;
    const uint32_t *wrow = walls + m * S;
    const Cell k = cell_of(wrow, S, c);
    const Goal gl = goal_of(goal, m, S);

    // qF is the forward probability as the recursion uses it: 0 where the front cell is the goal (that forward move
    // terminates: it is h_1, and g_t = 0 after it); src is the LDS slot the forward term reads, the front pose or,
    // where the front cell is a wall or off the grid, the pose itself (a self loop)
    double qL[4], qR[4], qF[4], h[4];
    int src[4];
#pragma unroll
    for (int d = 0; d < 4; d++) {
        qL[d] = qR[d] = qF[d] = h[d] = 0.0;
        src[d] = d * BLK + c;
        if (k.live) {
            load_probs(probs + (((m * 4 + d) * S + k.y) * (int64_t)S + k.x) * 3, qL[d], qR[d], qF[d]);
            const int fx = k.x + dir_x(d), fy = k.y + dir_y(d);
            if (gl.in && fx == gl.gx && fy == gl.gy) {
                h[d] = qF[d];
                qF[d] = 0.0;
            } else if (free_at(wrow, S, fx, fy)) {
                src[d] = d * BLK + fy * S + fx;
            }
        }
    }

    double a_s[4], a_r[4], a_n[4], a_d[4];
#pragma unroll
    for (int d = 0; d < 4; d++) a_s[d] = a_r[d] = a_n[d] = a_d[d] = 0.0;
    const double Td = (double)T;
    double g = 1.0;
    for (int t = 1; t <= T; t++) {
        const double td = (double)t;
        const double r = 1.0 - 0.9 * (td / Td);  // k_env_step's reward at action t
        const double gr = g * r;
        double *buf = hb[t & 1];
        if (k.live) {
#pragma unroll
            for (int d = 0; d < 4; d++) {
                a_s[d] += h[d];
                a_r[d] += h[d] * r;
                a_n[d] += td * h[d];
                a_d[d] += h[d] * gr;
                buf[d * BLK + c] = h[d];
            }
        }
        __syncthreads();
        if (k.live) {
            double f[4], n[4];
#pragma unroll
            for (int d = 0; d < 4; d++) f[d] = buf[src[d]];
#pragma unroll
            for (int d = 0; d < 4; d++) n[d] = (qL[d] * h[(d + 3) & 3] + qR[d] * h[(d + 1) & 3]) + qF[d] * f[d];
#pragma unroll
            for (int d = 0; d < 4; d++) h[d] = n[d];
        }
        g *= gamma;
    }

    if (c < cells) {
        const double nan = __longlong_as_double(0x7ff8000000000000LL);
#pragma unroll
        for (int d = 0; d < 4; d++) {
            const int64_t o = (m * 4 + d) * (int64_t)cells + c;
            if (success) success[o] = k.live ? a_s[d] : nan;
            if (ret) ret[o] = k.live ? a_r[d] : nan;
            if (steps) steps[o] = k.live ? a_n[d] + Td * (1.0 - a_s[d]) : nan;
            if (disc) disc[o] = k.live ? a_d[d] : nan;
        }
    }
}

template <int BLK>
__global__ __launch_bounds__(BLK) void k_policy_occupancy(const uint32_t *__restrict__ walls,
                                                           const int32_t *__restrict__ goal,
                                                           const float *__restrict__ probs,
                                                           const int32_t *__restrict__ agent, int S, int T,
                                                           double *__restrict__ visits, double *__restrict__ hit,
                                                           uint32_t *err) {
    __shared__ double fb[2][4 * BLK];
    const int64_t m = blockIdx.x;
    const int c = threadIdx.x, cells = S * S;
    const uint32_t *wrow = walls + m * S;
    const int ax = agent[4 * m], ay = agent[4 * m + 1], ad = agent[4 * m + 2];
    if (!(free_at(wrow, S, ax, ay) && ad >= 0 && ad <= 3)) {  // uniform over the block: no episode starts here
        const double nan = __longlong_as_double(0x7ff8000000000000LL);
        if (visits && c < cells) {
#pragma unroll
            for (int d = 0; d < 4; d++) visits[(m * 4 + d) * (int64_t)cells + c] = nan;
        }
        if (hit) {
            for (int t = c; t < T; t += BLK) hit[m * (int64_t)T + t] = nan;
        }
        if (c == 0) atomicOr(err, MERLIN_DEVERR_BAD_FRAME);
        return;
    }
    const Cell k = cell_of(wrow, S, c);
    const Goal gl = goal_of(goal, m, S);
    const bool on_goal = gl.in && k.x == gl.gx && k.y == gl.gy && c < cells;

    // back: the LDS slot of the pose whose forward move arrives here (-1: none -- the cell behind is a wall or off
    // the grid, or this cell is the goal, where a forward move ends the episode instead); qS: the forward
    // probability where the front is blocked, the self loop
    double qL[4], qR[4], qF[4], qS[4], mu[4], vis[4];
    int back[4];
#pragma unroll
    for (int d = 0; d < 4; d++) {
        qL[d] = qR[d] = qF[d] = qS[d] = mu[d] = vis[d] = 0.0;
        back[d] = -1;
        if (k.live) {
            load_probs(probs + (((m * 4 + d) * S + k.y) * (int64_t)S + k.x) * 3, qL[d], qR[d], qF[d]);
            const int vx = dir_x(d), vy = dir_y(d);
            const int fx = k.x + vx, fy = k.y + vy;
            if (!(gl.in && fx == gl.gx && fy == gl.gy) && !free_at(wrow, S, fx, fy)) qS[d] = qF[d];
            if (!on_goal && free_at(wrow, S, k.x - vx, k.y - vy)) back[d] = d * BLK + (k.y - vy) * S + (k.x - vx);
            if (k.x == ax && k.y == ay && d == ad) mu[d] = 1.0;
        }
    }
    // hit[t] is written by one thread, the goal cell's (thread 0 for a goal outside the grid: nothing terminates): the
    // sum over the at most four free poses facing the goal, d = 0..3
    const bool hitter = hit && (gl.in ? on_goal : c == 0);
    int face[4];
#pragma unroll
    for (int d = 0; d < 4; d++) {
        const int sx = gl.gx - dir_x(d), sy = gl.gy - dir_y(d);
        face[d] = (gl.in && free_at(wrow, S, sx, sy)) ? d * BLK + sy * S + sx : -1;
    }

    for (int t = 0; t < T; t++) {
        double *buf = fb[t & 1];
        double f[4];
        if (k.live) {
#pragma unroll
            for (int d = 0; d < 4; d++) {
                vis[d] += mu[d];
                f[d] = qF[d] * mu[d];
                buf[d * BLK + c] = f[d];
            }
        }
        __syncthreads();
        if (hitter) {
            double s = 0.0;
#pragma unroll
            for (int d = 0; d < 4; d++)
                if (face[d] >= 0) s += buf[face[d]];
            hit[m * (int64_t)T + t] = s;
        }
        if (k.live) {
            double n[4];
#pragma unroll
            for (int d = 0; d < 4; d++) {
                const double in = back[d] >= 0 ? buf[back[d]] : 0.0;
                const double self = qS[d] * mu[d];
                n[d] = ((qL[(d + 1) & 3] * mu[(d + 1) & 3] + qR[(d + 3) & 3] * mu[(d + 3) & 3]) + in) + self;
            }
#pragma unroll
            for (int d = 0; d < 4; d++) mu[d] = n[d];
        }
    }

    if (visits && c < cells) {
#pragma unroll
        for (int d = 0; d < 4; d++) visits[(m * 4 + d) * (int64_t)cells + c] = vis[d];
    }
}

// launch(integral_constant BLK) with the smallest block of 256, 512 and 1,024 threads that holds size^2 cells
template <class Launch>
hipError_t with_block(int size, Launch launch) {
    if (size * size <= 256)
        launch(std::integral_constant<int, 256>{});
    else if (size * size <= 512)
        launch(std::integral_constant<int, 512>{});
    else
        launch(std::integral_constant<int, 1024>{});
    return hipGetLastError();
}

}  // namespace

hipError_t launch_policy_chain(const uint32_t *walls, const int32_t *goal, const float *probs, int64_t n_maps, int size,
                               int horizon, double gamma, double *success, double *ret, double *steps, double *disc,
                               hipStream_t s) {
    if (n_maps <= 0) return hipSuccess;
    return with_block(size, [&](auto blk) {
        constexpr int BLK = decltype(blk)::value;
        hipLaunchKernelGGL(k_policy_chain<BLK>, dim3((unsigned)n_maps), dim3(BLK), 0, s, walls, goal, probs, size,
                           horizon, gamma, success, ret, steps, disc);
    });
}

hipError_t launch_policy_occupancy(const uint32_t *walls, const int32_t *goal, const float *probs,
                                   const int32_t *agent, int64_t n_maps, int size, int horizon, double *visits,
                                   double *hit, uint32_t *err, hipStream_t s) {
    if (n_maps <= 0) return hipSuccess;
    return with_block(size, [&](auto blk) {
        constexpr int BLK = decltype(blk)::value;
        hipLaunchKernelGGL(k_policy_occupancy<BLK>, dim3((unsigned)n_maps), dim3(BLK), 0, s, walls, goal, probs, agent,
                           size, horizon, visits, hit, err);
    });
}

// The host restatements go by another route: no cells and no neighbours, but one explicit successor table per map,
// three entries per pose (left, right, forward), over P = 4 S^2 poses and one absorbing state G = P, "the episode has
// terminated".  A forward move into the goal leads to G, one into a wall or off the grid to the pose itself.
namespace {

struct ChainTable {
    int P;
    std::vector<int> succ;     // [P][3]
    std::vector<double> q;     // [P][3], normalised
    std::vector<uint8_t> live; // [P]
};

void build_table(const grid_host::MapView &mv, int gx, int gy, const float *probs, ChainTable &tb) {
    const int S = mv.S;
    const int P = 4 * S * S;
    tb.P = P;
    tb.succ.assign((size_t)P * 3, 0);
    tb.q.assign((size_t)P * 3, 0.0);
    tb.live.assign(P, 0);
    const bool goal_in = mv.inside(gx, gy);
    for (int p = 0; p < P; p++) {
        int d, y, x;
        mv.decode(p, d, y, x);
        if (!mv.is_free(x, y)) continue;
        tb.live[p] = 1;
        const double p0 = (double)probs[3 * p], p1 = (double)probs[3 * p + 1], p2 = (double)probs[3 * p + 2];
        const double s = (p0 + p1) + p2;
        tb.q[3 * p] = p0 / s;
        tb.q[3 * p + 1] = p1 / s;
        tb.q[3 * p + 2] = p2 / s;
        tb.succ[3 * p] = mv.pose((d + 3) & 3, y, x);
        tb.succ[3 * p + 1] = mv.pose((d + 1) & 3, y, x);
        const int fx = x + grid_host::DX[d], fy = y + grid_host::DY[d];
        if (goal_in && fx == gx && fy == gy)
            tb.succ[3 * p + 2] = P;
        else if (mv.is_free(fx, fy))
            tb.succ[3 * p + 2] = mv.pose(d, fy, fx);
        else
            tb.succ[3 * p + 2] = p;
    }
}

}  // namespace

// u_0 = the indicator of G, u_{t+1}(p) = sum over the pose's three actions of q_a(p) u_t(succ_a(p)), u_{t+1}(G) = 0:
// u_t(p) is h_t(p), the probability of arriving in G at exactly action t.
void policy_chain_host(const uint32_t *walls, const int32_t *goal, const float *probs, int64_t n_maps, int S, int T,
                       double gamma, double *success, double *ret, double *steps, double *disc) {
    const int P = 4 * S * S;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    ChainTable tb;
    std::vector<double> u(P + 1), v(P + 1), a_s(P), a_r(P), a_n(P), a_d(P);
    for (int64_t m = 0; m < n_maps; m++) {
        build_table({walls + m * S, S}, goal[2 * m], goal[2 * m + 1], probs + m * (int64_t)P * 3, tb);
        std::fill(u.begin(), u.end(), 0.0);
        u[P] = 1.0;
        std::fill(a_s.begin(), a_s.end(), 0.0);
        std::fill(a_r.begin(), a_r.end(), 0.0);
        std::fill(a_n.begin(), a_n.end(), 0.0);
        std::fill(a_d.begin(), a_d.end(), 0.0);
        double g = 1.0;
        for (int t = 1; t <= T; t++) {
            for (int p = 0; p < P; p++) {
                const int *sc = &tb.succ[3 * p];
                const double *q = &tb.q[3 * p];
                v[p] = (q[0] * u[sc[0]] + q[1] * u[sc[1]]) + q[2] * u[sc[2]];
            }
            v[P] = 0.0;
            u.swap(v);
            const double r = 1.0 - 0.9 * ((double)t / (double)T);
            const double gr = g * r;
            for (int p = 0; p < P; p++) {
                a_s[p] += u[p];
                a_r[p] += u[p] * r;
                a_n[p] += (double)t * u[p];
                a_d[p] += u[p] * gr;
            }
            g *= gamma;
        }
        for (int p = 0; p < P; p++) {
            const int64_t o = m * (int64_t)P + p;
            const bool lv = tb.live[p] != 0;
            if (success) success[o] = lv ? a_s[p] : nan;
            if (ret) ret[o] = lv ? a_r[p] : nan;
            if (steps) steps[o] = lv ? a_n[p] + (double)T * (1.0 - a_s[p]) : nan;
            if (disc) disc[o] = lv ? a_d[p] : nan;
        }
    }
}

// mu_0 = the indicator of the start pose; every pose scatters its mass to its three successors, and what arrives in G
// at action t is hit[t - 1] (poses are visited in (dir, y, x) order, so the at most four poses facing the goal add
// up in the order d = 0..3).
void policy_occupancy_host(const uint32_t *walls, const int32_t *goal, const float *probs, const int32_t *agent,
                           int64_t n_maps, int S, int T, double *visits, double *hit) {
    const int P = 4 * S * S;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    ChainTable tb;
    std::vector<double> mu(P + 1), nx(P + 1), vis(P);
    for (int64_t m = 0; m < n_maps; m++) {
        const grid_host::MapView mv{walls + m * S, S};
        const int ax = agent[4 * m], ay = agent[4 * m + 1], ad = agent[4 * m + 2];
        if (!(mv.is_free(ax, ay) && ad >= 0 && ad <= 3)) {
            if (visits) std::fill(visits + m * (int64_t)P, visits + (m + 1) * (int64_t)P, nan);
            if (hit) std::fill(hit + m * (int64_t)T, hit + (m + 1) * (int64_t)T, nan);
            continue;
        }
        build_table(mv, goal[2 * m], goal[2 * m + 1], probs + m * (int64_t)P * 3, tb);
        std::fill(mu.begin(), mu.end(), 0.0);
        std::fill(vis.begin(), vis.end(), 0.0);
        mu[mv.pose(ad, ay, ax)] = 1.0;
        for (int t = 0; t < T; t++) {
            std::fill(nx.begin(), nx.end(), 0.0);
            for (int p = 0; p < P; p++) {
                const double mp = mu[p];
                vis[p] += mp;
                if (mp == 0.0) continue;
                for (int a = 0; a < 3; a++) nx[tb.succ[3 * p + a]] += tb.q[3 * p + a] * mp;
            }
            if (hit) hit[m * (int64_t)T + t] = nx[P];
            nx[P] = 0.0;
            mu.swap(nx);
        }
        if (visits)
            for (int p = 0; p < P; p++) visits[m * (int64_t)P + p] = vis[p];
    }
}

}  // namespace merlin
