// merlin_capi.hip -- host side of libmerlin_hip.so: the extern "C" ABI declared
// in include/merlin_hip.h, env-context lifetime, numpy SeedSequence seeding and
// the library's own restatement of minigrid's tile renderer (the atlas).
#include <math.h>
#include <string.h>

#include <mutex>
#include <string>
#include <vector>

#include <algorithm>

#include "merlin_internal.h"

struct merlin_env {
    merlin::EnvDev dev;
    int device;
    bool has_state;
    int steps_since_refill;  // merlin_env_step launches since the last look-ahead refill
    int refill_every;        // 0: the caller launches refills (merlin_env_refill)
    bool no_fallback = false;  // merlin_env_set_step_fallback(0): with refill_every 0, no k_env_fallback pass
    // reseed mode (every reset is reset(seed=task_seed)) after a full reset: every look-ahead slot holds its env's
    // seed map and no reset consumes it, so the periodic refills and the fallback pass would find nothing to do and
    // are left out (an empty slot would still raise MERLIN_DEVERR_SLOT_EMPTY); cleared when merlin_env_seed makes
    // the slots stale (round 6: FOMAML's 32-env task rollouts, two graph nodes fewer per step)
    bool seed_slots_full = false;
    // the per-env generator classes uint8[n], allocated with the context so that its address never changes: dev.diff
    // is this buffer once merlin_env_set_difficulties has assigned classes, null (the uniform dev.difficulty) before
    // that and after a NULL assignment
    uint8_t *diff_buf = nullptr;
    int32_t *level_log = nullptr;  // merlin_env_set_level_log: where the next step launches log the envs' levels
    uint8_t *lv_flags = nullptr;   // merlin_env_replace_levels' scratch, uint8[lv_n]: the slots a call replaces
    // (level mode, merlin_env_set_levels: dev.lv_* are buffers the context owns from one binding to the next or to the
    // unbinding; a graph captured under a binding reads that binding's buffers)
};

namespace {

thread_local std::string g_err;

int fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}

int hip_fail(hipError_t e, const char *what) {
    return fail(MERLIN_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

#define HIP_TRY(expr)                                  \
    do {                                               \
        hipError_t _e = (expr);                        \
        if (_e != hipSuccess) return hip_fail(_e, #expr); \
    } while (0)

// The map entries' shared argument rules, in order: the grid size, the entry's own range check (`range_err`: its
// message, or null), the count's sign, the needed pointers.  0: go on, -1: a zero count, nothing to do, else the code.
int map_args(int32_t size, const char *range_err, int64_t n, const char *negative, bool required) {
    if (size < 5 || size > 32) return fail(MERLIN_E_INVALID, "grid size must be in [5, 32]");
    if (range_err) return fail(MERLIN_E_INVALID, range_err);
    if (n < 0) return fail(MERLIN_E_INVALID, negative);
    if (n == 0) return -1;
    if (!required) return fail(MERLIN_E_INVALID, "null argument");
    return 0;
}

#define ARGS_TRY(expr)                                      \
    do {                                                    \
        const int _rc = (expr);                             \
        if (_rc) return _rc < 0 ? MERLIN_OK : _rc;          \
    } while (0)

// ---------------------------------------------------------------------------
// numpy SeedSequence(seed).generate_state(4, uint64) -> PCG64 seeding
// (numpy/random/bit_generator.pyx mix_entropy / generate_state,
//  numpy/random/_pcg64.pyx -> pcg64_set_seed -> pcg_setseq_128_srandom_r).
struct U128 {
    uint64_t hi, lo;
};

U128 mul128(U128 a, U128 b) {
    const unsigned __int128 x = ((unsigned __int128)a.hi << 64) | a.lo;
    const unsigned __int128 y = ((unsigned __int128)b.hi << 64) | b.lo;
    const unsigned __int128 z = x * y;
    return {(uint64_t)(z >> 64), (uint64_t)z};
}

U128 add128(U128 a, U128 b) {
    const unsigned __int128 x = ((unsigned __int128)a.hi << 64) | a.lo;
    const unsigned __int128 y = ((unsigned __int128)b.hi << 64) | b.lo;
    const unsigned __int128 z = x + y;
    return {(uint64_t)(z >> 64), (uint64_t)z};
}

void seed_pcg64(uint64_t seed, U128 &state, U128 &inc) {
    uint32_t ent[2];
    int n = 0;
    if (seed == 0) ent[n++] = 0;
    for (uint64_t s = seed; s; s >>= 32) ent[n++] = (uint32_t)s;
    uint32_t pool[4];
    uint32_t hc = 0x43b0d7e5u;
    auto hashmix = [&hc](uint32_t v) {
        v ^= hc;
        hc *= 0x931e8875u;
        v *= hc;
        v ^= v >> 16;
        return v;
    };
    auto mix = [](uint32_t x, uint32_t y) {
        uint32_t r = 0xca01f9ddu * x - 0x4973f715u * y;
        return r ^ (r >> 16);
    };
    for (int i = 0; i < 4; i++) pool[i] = hashmix(i < n ? ent[i] : 0u);
    for (int s = 0; s < 4; s++)
        for (int d = 0; d < 4; d++)
            if (s != d) pool[d] = mix(pool[d], hashmix(pool[s]));
    uint32_t w[8];
    uint32_t hb = 0x8b51f9ddu;
    for (int i = 0; i < 8; i++) {
        uint32_t v = pool[i & 3] ^ hb;
        hb *= 0x58f38dedu;
        v *= hb;
        w[i] = v ^ (v >> 16);
    }
    const uint64_t v0 = (uint64_t)w[0] | ((uint64_t)w[1] << 32), v1 = (uint64_t)w[2] | ((uint64_t)w[3] << 32);
    const uint64_t v2 = (uint64_t)w[4] | ((uint64_t)w[5] << 32), v3 = (uint64_t)w[6] | ((uint64_t)w[7] << 32);
    const U128 initstate{v0, v1}, initseq{v2, v3};
    inc = {(initseq.hi << 1) | (initseq.lo >> 63), (initseq.lo << 1) | 1u};
    const U128 mult{0x2360ed051fc65da4ULL, 0x4385df649fccf645ULL};
    state = inc;  // step from state 0: 0 * mult + inc
    state = add128(state, initstate);
    state = add128(mul128(state, mult), inc);
}

// ---------------------------------------------------------------------------
// minigrid 3.0.0 Grid.render_tile(obj, agent_dir, highlight, tile_size=8, subdivs=3)
// with minigrid.utils.rendering fill_coords / point_in_rect / point_in_triangle /
// rotate_fn / highlight_img / downsample, keeping numpy's dtypes: float32
// triangle vertices and their dot products, float64 sample points, uint8
// canvas, float64 means, truncating cast into the uint8 frame.
struct Tri {
    float ax, ay, v0x, v0y, v1x, v1y, dot00, dot01, dot11, inv;
    Tri() {
        const float a[2] = {0.12f, 0.19f}, b[2] = {0.87f, 0.50f}, c[2] = {0.12f, 0.81f};
        ax = a[0];
        ay = a[1];
        v0x = c[0] - a[0];
        v0y = c[1] - a[1];
        v1x = b[0] - a[0];
        v1y = b[1] - a[1];
        dot00 = v0x * v0x + v0y * v0y;
        dot01 = v0x * v1x + v0y * v1y;
        dot11 = v1x * v1x + v1y * v1y;
        const float den = dot00 * dot11 - dot01 * dot01;
        inv = 1.0f / den;
    }
    bool in(double x, double y) const {
        const double v2x = x - (double)ax, v2y = y - (double)ay;
        const double dot02 = (double)v0x * v2x + (double)v0y * v2y;
        const double dot12 = (double)v1x * v2x + (double)v1y * v2y;
        const double u = ((double)dot11 * dot02 - (double)dot01 * dot12) * (double)inv;
        const double v = ((double)dot00 * dot12 - (double)dot01 * dot02) * (double)inv;
        return (u >= 0) && (v >= 0) && (u + v) < 1;
    }
};

// agent_dir < 0: no agent; out uint8[ts][ts][3]
void render_tile(int obj /*0 none 1 wall 2 goal*/, int agent_dir, bool highlight, int ts, uint8_t *out) {
    const int N = 3 * ts;  // subdivs = 3
    std::vector<uint8_t> canvas((size_t)N * N * 3, 0);
    auto img = [&](int y, int x) { return canvas.data() + ((size_t)y * N + x) * 3; };
    auto fill_rect = [&](double xmin, double xmax, double ymin, double ymax, const uint8_t col[3]) {
        for (int y = 0; y < N; y++)
            for (int x = 0; x < N; x++) {
                const double yf = (y + 0.5) / N, xf = (x + 0.5) / N;
                if (xf >= xmin && xf <= xmax && yf >= ymin && yf <= ymax) memcpy(img(y, x), col, 3);
            }
    };
    const uint8_t grey[3] = {100, 100, 100}, green[3] = {0, 255, 0}, red[3] = {255, 0, 0};
    fill_rect(0, 0.031, 0, 1, grey);
    fill_rect(0, 1, 0, 0.031, grey);
    if (obj == 1) fill_rect(0, 1, 0, 1, grey);
    if (obj == 2) fill_rect(0, 1, 0, 1, green);
    if (agent_dir >= 0) {
        const Tri tri;
        const double theta = 0.5 * M_PI * agent_dir;  // rotate_fn(tri, cx=0.5, cy=0.5, theta=0.5*pi*agent_dir)
        const double c = cos(-theta), s = sin(-theta);
        for (int y = 0; y < N; y++)
            for (int x = 0; x < N; x++) {
                const double yf = (y + 0.5) / N, xf = (x + 0.5) / N;
                const double px = xf - 0.5, py = yf - 0.5;
                const double x2 = (0.5 + px * c) - py * s;
                const double y2 = (0.5 + py * c) + px * s;
                if (tri.in(x2, y2)) memcpy(img(y, x), red, 3);
            }
    }
    if (highlight)
        for (uint8_t &px : canvas) {
            const uint8_t p = px;
            double v = (double)p + 0.30 * (double)(uint8_t)(255 - p);
            v = v < 0 ? 0 : (v > 255 ? 255 : v);
            px = (uint8_t)v;
        }
    for (int Y = 0; Y < ts; Y++)
        for (int X = 0; X < ts; X++)
            for (int k = 0; k < 3; k++) {
                double m[3];
                for (int sy = 0; sy < 3; sy++) {
                    const uint8_t *r0 = img(3 * Y + sy, 3 * X);
                    m[sy] = (((double)r0[k] + (double)r0[3 + k]) + (double)r0[6 + k]) / 3.0;
                }
                out[(Y * ts + X) * 3 + k] = (uint8_t)(((m[0] + m[1]) + m[2]) / 3.0);
            }
}

uint8_t g_atlas[MERLIN_OBS_TILES][8][8][3];
std::once_flag g_atlas_once;

void build_atlas() {
    std::call_once(g_atlas_once, [] {
        render_tile(0, -1, false, 8, &g_atlas[0][0][0][0]);  // not visible: empty, no highlight
        render_tile(0, -1, true, 8, &g_atlas[1][0][0][0]);   // visible empty
        render_tile(1, -1, true, 8, &g_atlas[2][0][0][0]);   // visible wall
        render_tile(2, -1, true, 8, &g_atlas[3][0][0][0]);   // visible goal
        render_tile(0, 3, true, 8, &g_atlas[4][0][0][0]);    // agent (view cell (3,6), agent_dir 3 in get_pov_render)
    });
}

// the frame atlas of one tile size (include/merlin_hip.h MERLIN_FRAME_TILES, the order fixed there), built on first
// use and kept
constexpr int FRAME_TS_MIN = 4, FRAME_TS_MAX = 32;
std::vector<uint8_t> g_frame_atlas[FRAME_TS_MAX + 1];
std::mutex g_frame_atlas_mu;

const std::vector<uint8_t> &frame_atlas(int ts) {
    std::lock_guard<std::mutex> lk(g_frame_atlas_mu);
    std::vector<uint8_t> &a = g_frame_atlas[ts];
    if (a.empty()) {
        const size_t tile = (size_t)ts * ts * 3;
        a.resize(MERLIN_FRAME_TILES * tile);
        for (int hl = 0; hl < 2; hl++)
            for (int obj = 0; obj < 3; obj++) render_tile(obj, -1, hl != 0, ts, a.data() + (obj + 3 * hl) * tile);
        for (int on_goal = 0; on_goal < 2; on_goal++)
            for (int dir = 0; dir < 4; dir++)
                for (int hl = 0; hl < 2; hl++)
                    render_tile(on_goal ? 2 : 0, dir, hl != 0, ts,
                                a.data() + (6 + ((on_goal * 4 + dir) * 2 + hl)) * tile);
    }
    return a;
}

// per-device one-time init: atlas upload + GAE partials workspace
struct DeviceWs {
    bool ready = false;
    double *partials = nullptr;
    int max_partials = 0;
    float *conv1_slabs = nullptr;
    int max_slabs = 0;
    void *lut2_slabs = nullptr;  // conv2 table histogram: per-block 4-channel u64 slices
    float *epi_work = nullptr;   // GEMM epilogues: per-block column-sum partials
    double *stage_part = nullptr;  // conv tables' adjoint: the 625-combination type's partial dW2 sums
    uint32_t *tower_err = nullptr;  // device error flags of the tower kernels (merlin_tower_errors)
    double *eps_part = nullptr;     // merlin_episode_class_stats: the per-block class sums
    uint8_t *frame_atlas[33] = {};  // the frame atlas by tile size (merlin_render.hip), uploaded on first use
};
constexpr int MAX_DEV = 64;
DeviceWs g_dev[MAX_DEV];
std::mutex g_dev_mu;
constexpr int WS_PARTIALS = 1 << 16;
constexpr int WS_SLABS = 1024;  // conv1 backward: per-block partial slabs (1024 x 2 towers x 2592 floats)

int device_ws(DeviceWs **out) {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev < 0 || dev >= MAX_DEV) return fail(MERLIN_E_UNSUPPORTED, "device index out of range");
    std::lock_guard<std::mutex> lk(g_dev_mu);
    DeviceWs &w = g_dev[dev];
    if (!w.ready) {
        build_atlas();
        HIP_TRY(merlin::upload_atlas(&g_atlas[0][0][0][0]));
        HIP_TRY(hipMalloc(&w.partials, sizeof(double) * 2 * WS_PARTIALS));
        w.max_partials = WS_PARTIALS;
        HIP_TRY(hipMalloc(&w.conv1_slabs, sizeof(float) * (size_t)WS_SLABS * merlin::conv1_slab_floats(2)));
        w.max_slabs = WS_SLABS;
        HIP_TRY(hipMalloc(&w.lut2_slabs, merlin::conv2_lut_slab_bytes(2, merlin::conv2_lut_fblocks(INT64_MAX / 64))));
        HIP_TRY(hipMalloc(&w.epi_work, sizeof(float) * merlin::epilogue_work_floats()));
        HIP_TRY(hipMalloc(&w.stage_part, sizeof(double) * merlin::STAGE_WS_DOUBLES));
        HIP_TRY(hipMalloc(&w.tower_err, sizeof(uint32_t)));
        HIP_TRY(hipMalloc(&w.eps_part, sizeof(double) * merlin::EPS_MAX_BLOCKS * merlin::EPS_MAX_CLASSES * 4));
        HIP_TRY(hipMemset(w.tower_err, 0, sizeof(uint32_t)));  // once, outside any capture
        HIP_TRY(hipDeviceSynchronize());
        w.ready = true;
    }
    *out = &w;
    return MERLIN_OK;
}

// the device copy of the frame atlas of tile size ts (4..32), uploaded at the first render of that size
int device_frame_atlas(int ts, const uint8_t **out, uint32_t **err) {
    DeviceWs *ws = nullptr;
    int rc = device_ws(&ws);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(g_dev_mu);
    if (!ws->frame_atlas[ts]) {
        const std::vector<uint8_t> &a = frame_atlas(ts);
        uint8_t *d = nullptr;
        HIP_TRY(hipMalloc(&d, a.size()));
        hipError_t e = hipMemcpy(d, a.data(), a.size(), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(d);
            return hip_fail(e, "hipMemcpy(frame atlas)");
        }
        ws->frame_atlas[ts] = d;
    }
    *out = ws->frame_atlas[ts];
    if (err) *err = ws->tower_err;
    return MERLIN_OK;
}

// zero_async's kernel: a 16-B aligned body by grid-stride uint4 stores; the unaligned head and the tail (< 16 B each)
// by block 0's first lanes, byte stores
__global__ void k_zero_fill(uint8_t *__restrict__ p, uint32_t head, size_t n16, uint32_t tail) {
    uint4 *v = reinterpret_cast<uint4 *>(p + head);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (size_t)gridDim.x * 256)
        v[i] = make_uint4(0u, 0u, 0u, 0u);
    if (blockIdx.x == 0) {
        if (threadIdx.x < head) p[threadIdx.x] = 0;
        if (threadIdx.x < tail) p[head + n16 * 16 + threadIdx.x] = 0;
    }
}
}  // namespace

hipError_t merlin::zero_async(void *p, size_t bytes, hipStream_t s) {
    if (bytes == 0) return hipSuccess;
    auto *b = static_cast<uint8_t *>(p);
    size_t head = (16 - (reinterpret_cast<uintptr_t>(b) & 15)) & 15;
    if (head > bytes) head = bytes;
    const size_t n16 = (bytes - head) / 16;
    const size_t tail = bytes - head - n16 * 16;
    const int grid = (int)std::max<size_t>(1, std::min<size_t>((n16 + 255) / 256, 2048));
    hipLaunchKernelGGL(k_zero_fill, dim3(grid), dim3(256), 0, s, b, (uint32_t)head, n16, (uint32_t)tail);
    return hipGetLastError();
}

extern "C" {

int merlin_version(void) { return MERLIN_ABI_VERSION; }

const char *merlin_last_error(void) { return g_err.c_str(); }

int merlin_tile_atlas(uint8_t *out_host) {
    if (!out_host) return fail(MERLIN_E_INVALID, "null output");
    build_atlas();
    memcpy(out_host, g_atlas, sizeof(g_atlas));
    return MERLIN_OK;
}

int merlin_frame_atlas(int32_t tile_size, uint8_t *out_host) {
    if (!out_host) return fail(MERLIN_E_INVALID, "null output");
    if (tile_size < FRAME_TS_MIN || tile_size > FRAME_TS_MAX) return fail(MERLIN_E_INVALID, "tile_size must be in [4, 32]");
    const std::vector<uint8_t> &a = frame_atlas(tile_size);
    memcpy(out_host, a.data(), a.size());
    return MERLIN_OK;
}

int merlin_render_frames(const uint32_t *walls, const int32_t *goal, const int32_t *agent, const int32_t *map_index,
                         int64_t n_frames, int32_t size, int32_t tile_size, int32_t highlight, uint8_t *out,
                         void *stream) {
    const bool ts_ok = tile_size >= FRAME_TS_MIN && tile_size <= FRAME_TS_MAX;
    const char *ts_err = ts_ok ? nullptr : "tile_size must be in [4, 32]";
    ARGS_TRY(map_args(size, ts_err, n_frames, "negative frame count", walls && agent && out));
    const uint8_t *atlas = nullptr;
    uint32_t *err = nullptr;
    int rc = device_frame_atlas(tile_size, &atlas, &err);
    if (rc) return rc;
    HIP_TRY(merlin::launch_render_frames(walls, goal, agent, map_index, n_frames, size, tile_size, highlight, atlas,
                                         out, err, (hipStream_t)stream));
    return MERLIN_OK;
}

int merlin_env_render(merlin_env *e, const int64_t *index, int64_t n, int32_t tile_size, int32_t highlight,
                      uint8_t *out, void *stream) {
    if (!e) return fail(MERLIN_E_INVALID, "null env");
    if (!e->has_state) return fail(MERLIN_E_INVALID, "merlin_env_render before merlin_env_reset");
    if (tile_size < FRAME_TS_MIN || tile_size > FRAME_TS_MAX) return fail(MERLIN_E_INVALID, "tile_size must be in [4, 32]");
    if (n < 0 || (!index && n != e->dev.n)) return fail(MERLIN_E_INVALID, "without env ids, n must be num_envs");
    if (n == 0) return MERLIN_OK;
    if (!out) return fail(MERLIN_E_INVALID, "null output");
    const uint8_t *atlas = nullptr;
    int rc = device_frame_atlas(tile_size, &atlas, nullptr);
    if (rc) return rc;
    HIP_TRY(merlin::launch_env_render(e->dev, index, n, tile_size, highlight, atlas, out, (hipStream_t)stream));
    return MERLIN_OK;
}

int merlin_env_snapshot(merlin_env *e, uint32_t *walls, int32_t *goal, int32_t *agent, void *stream) {
    if (!e) return fail(MERLIN_E_INVALID, "null env");
    if (!e->has_state) return fail(MERLIN_E_INVALID, "merlin_env_snapshot before merlin_env_reset");
    if (!walls && !goal && !agent) return MERLIN_OK;
    HIP_TRY(merlin::launch_env_snapshot(e->dev, walls, goal, agent, (hipStream_t)stream));
    return MERLIN_OK;
}

int merlin_shortest_paths(const uint32_t *walls, const int32_t *goal, const int32_t *agent, const int32_t *map_index,
                          int64_t n, int32_t size, int32_t *dist, int16_t *field, void *stream) {
    ARGS_TRY(map_args(size, nullptr, n, "negative query count", walls && goal && agent && dist));
    HIP_TRY(merlin::launch_shortest_paths(walls, goal, agent, map_index, n, size, dist, field, (hipStream_t)stream));
    return MERLIN_OK;
}

int merlin_env_optimal_steps(merlin_env *e, int32_t *dist, int16_t *field, void *stream) {
    if (!e) return fail(MERLIN_E_INVALID, "null env");
    if (!e->has_state) return fail(MERLIN_E_INVALID, "merlin_env_optimal_steps before merlin_env_reset");
    if (!dist) return fail(MERLIN_E_INVALID, "null output");
    HIP_TRY(merlin::launch_env_optimal_steps(e->dev, dist, field, (hipStream_t)stream));
    return MERLIN_OK;
}

int merlin_shortest_paths_host(const uint32_t *walls, const int32_t *goal, const int32_t *agent, int64_t n,
                               int32_t size, int32_t *dist, int16_t *field) {
    ARGS_TRY(map_args(size, nullptr, n, "negative query count", walls && goal && agent && dist));
    merlin::shortest_paths_host(walls, goal, agent, n, size, dist, field);
    return MERLIN_OK;
}

int merlin_view_codes(const uint32_t *walls, const int32_t *goal, const int32_t *agent, const int32_t *map_index,
                      int64_t n, int32_t size, uint32_t *codes, void *stream) {
    ARGS_TRY(map_args(size, nullptr, n, "negative query count", walls && agent && codes));
    DeviceWs *ws = nullptr;
    int rc = device_ws(&ws);
    if (rc) return rc;
    HIP_TRY(merlin::launch_view_codes(walls, goal, agent, map_index, n, size, codes, ws->tower_err,
                                      (hipStream_t)stream));
    return MERLIN_OK;
}

int merlin_policy_paths(const uint32_t *walls, const int32_t *goal, const int8_t *action, int64_t n_maps,
                        int32_t size, int16_t *steps, void *stream) {
    ARGS_TRY(map_args(size, nullptr, n_maps, "negative map count", walls && goal && action && steps));
    HIP_TRY(merlin::launch_policy_paths(walls, goal, action, n_maps, size, steps, (hipStream_t)stream));
    return MERLIN_OK;
}

int merlin_policy_paths_host(const uint32_t *walls, const int32_t *goal, const int8_t *action, int64_t n_maps,
                             int32_t size, int16_t *steps) {
    ARGS_TRY(map_args(size, nullptr, n_maps, "negative map count", walls && goal && action && steps));
    merlin::policy_paths_host(walls, goal, action, n_maps, size, steps);
    return MERLIN_OK;
}

// map_args for the four sampled-policy entries: the horizon's range, and at least one output
static int chain_args(int64_t n_maps, int32_t size, int32_t horizon, bool required, bool any_output) {
    const char *t_err = horizon >= 1 && horizon <= 16384 ? nullptr : "horizon must be in [1, 16384]";
    const int rc = map_args(size, t_err, n_maps, "negative map count", required);
    return rc || any_output ? rc : fail(MERLIN_E_INVALID, "no output requested");
}

int merlin_policy_chain(const uint32_t *walls, const int32_t *goal, const float *probs, int64_t n_maps, int32_t size,
                        int32_t horizon, double gamma, double *success, double *ret, double *steps, double *disc,
                        void *stream) {
    ARGS_TRY(chain_args(n_maps, size, horizon, walls && goal && probs, success || ret || steps || disc));
    HIP_TRY(merlin::launch_policy_chain(walls, goal, probs, n_maps, size, horizon, gamma, success, ret, steps, disc,
                                        (hipStream_t)stream));
    return MERLIN_OK;
}

int merlin_policy_chain_host(const uint32_t *walls, const int32_t *goal, const float *probs, int64_t n_maps,
                             int32_t size, int32_t horizon, double gamma, double *success, double *ret,
                             double *steps, double *disc) {
    ARGS_TRY(chain_args(n_maps, size, horizon, walls && goal && probs, success || ret || steps || disc));
    merlin::policy_chain_host(walls, goal, probs, n_maps, size, horizon, gamma, success, ret, steps, disc);
    return MERLIN_OK;
}

int merlin_policy_occupancy(const uint32_t *walls, const int32_t *goal, const float *probs, const int32_t *agent,
                            int64_t n_maps, int32_t size, int32_t horizon, double *visits, double *hit,
                            void *stream) {
    ARGS_TRY(chain_args(n_maps, size, horizon, walls && goal && probs && agent, visits || hit));
    DeviceWs *ws = nullptr;
    const int rc = device_ws(&ws);
    if (rc) return rc;
    HIP_TRY(merlin::launch_policy_occupancy(walls, goal, probs, agent, n_maps, size, horizon, visits, hit,
                                            ws->tower_err, (hipStream_t)stream));
    return MERLIN_OK;
}

int merlin_policy_occupancy_host(const uint32_t *walls, const int32_t *goal, const float *probs,
                                 const int32_t *agent, int64_t n_maps, int32_t size, int32_t horizon,
                                 double *visits, double *hit) {
    ARGS_TRY(chain_args(n_maps, size, horizon, walls && goal && probs && agent, visits || hit));
    merlin::policy_occupancy_host(walls, goal, probs, agent, n_maps, size, horizon, visits, hit);
    return MERLIN_OK;
}

int64_t merlin_env_config_layout(int64_t *offsets_host, int32_t n_fields) {
    const int64_t off[MERLIN_ENV_CONFIG_FIELDS] = {
        (int64_t)offsetof(merlin_env_config, num_envs),     (int64_t)offsetof(merlin_env_config, size),
        (int64_t)offsetof(merlin_env_config, difficulty),   (int64_t)offsetof(merlin_env_config, max_steps),
        (int64_t)offsetof(merlin_env_config, stuck_penalty), (int64_t)offsetof(merlin_env_config, max_stay),
        (int64_t)offsetof(merlin_env_config, penalty),      (int64_t)offsetof(merlin_env_config, exploration_bonus),
        (int64_t)offsetof(merlin_env_config, bonus),        (int64_t)offsetof(merlin_env_config, reseed_each_reset)};
    if (offsets_host)
        for (int i = 0; i < n_fields && i < MERLIN_ENV_CONFIG_FIELDS; i++) offsets_host[i] = off[i];
    return (int64_t)sizeof(merlin_env_config);
}

int merlin_env_create(const merlin_env_config *cfg, merlin_env **out) {
    if (!cfg || !out) return fail(MERLIN_E_INVALID, "null argument");
    *out = nullptr;
    if (cfg->num_envs <= 0) return fail(MERLIN_E_INVALID, "num_envs must be > 0");
    if (cfg->size < 5 || cfg->size > 32)
        return fail(MERLIN_E_UNSUPPORTED, "grid size must be in [5, 32]");
    if (cfg->difficulty < MERLIN_EASY || cfg->difficulty > MERLIN_HARDEST)
        return fail(MERLIN_E_INVALID, "unknown difficulty");
    // the sizes at which the reference's generators run: every other difficulty (hard included: one gap, the goal
    // and the agent each have a free column at 5) generates from 5 up; hardest draws integers(2, size/2 - 1) for its
    // first opening, an empty range below 8 (numpy raises ValueError)
    if (cfg->difficulty == MERLIN_HARDEST && cfg->size < 8)
        return fail(MERLIN_E_UNSUPPORTED, "hardest needs size >= 8 (integers(2, size/2 - 1) is empty below)");
    DeviceWs *ws = nullptr;
    int rc = device_ws(&ws);
    if (rc) return rc;
    merlin_env *e = new merlin_env();
    e->refill_every = merlin::REFILL_EVERY;
    merlin::EnvDev &d = e->dev;
    d.n = cfg->num_envs;
    d.size = cfg->size;
    d.sp = cfg->size <= 16 ? 16 : 32;
    d.difficulty = cfg->difficulty;
    d.max_steps = cfg->max_steps > 0 ? cfg->max_steps : 4 * cfg->size * cfg->size;
    d.stuck_on = cfg->stuck_penalty ? 1 : 0;
    d.max_stay = cfg->max_stay > 0 ? cfg->max_stay : 3;
    d.penalty = cfg->penalty;
    d.explore_on = cfg->exploration_bonus ? 1 : 0;
    d.bonus = cfg->bonus;
    d.reseed = cfg->reseed_each_reset ? 1 : 0;
    (void)hipGetDevice(&e->device);
    const size_t n = (size_t)d.n;
    hipError_t err = hipSuccess;
    auto alloc = [&](void **p, size_t bytes) {
        if (err == hipSuccess) err = hipMalloc(p, bytes);
        if (err == hipSuccess) err = hipMemset(*p, 0, bytes);
    };
    alloc((void **)&d.walls, n * d.sp * sizeof(uint32_t));
    alloc((void **)&d.agent, n * sizeof(uint4));
    alloc((void **)&d.rng_s, n * sizeof(ulonglong2));
    alloc((void **)&d.rng_i, n * sizeof(ulonglong2));
    alloc((void **)&d.rng_b, n * sizeof(uint2));
    alloc((void **)&d.ep_ret, n * sizeof(double));
    alloc((void **)&d.ep_len, n * sizeof(int32_t));
    alloc((void **)&d.err, 2 * sizeof(uint32_t));
    alloc((void **)&d.pg_walls, n * d.sp * sizeof(uint32_t));
    alloc((void **)&d.pg_agent, n * sizeof(uint4));
    alloc((void **)&d.pg_rng_s, n * sizeof(ulonglong2));
    alloc((void **)&d.pg_rng_b, n * sizeof(uint2));
    alloc((void **)&d.pg_valid, n * sizeof(uint8_t));
    alloc((void **)&d.pg_ring, n * sizeof(uint32_t));
    d.pg_depth = 1;
    alloc((void **)&d.rflag, n * sizeof(uint8_t));
    alloc((void **)&d.bflag, (n + 63) / 64);  // one flag per step block (merlin_env.hip SBLK >= 64 envs)
    if (d.explore_on) alloc((void **)&d.visited, n * d.sp * sizeof(uint32_t));
    alloc((void **)&e->diff_buf, n * sizeof(uint8_t));
    if (err != hipSuccess) {
        merlin_env_destroy(e);
        return hip_fail(err, "hipMalloc(env state)");
    }
    *out = e;
    return MERLIN_OK;
}

int merlin_env_destroy(merlin_env *e) {
    if (!e) return MERLIN_OK;
    merlin::EnvDev &d = e->dev;
    void *ptrs[] = {d.walls, d.agent, d.rng_s, d.rng_i, d.rng_b, d.ep_ret, d.ep_len, d.err, d.visited,
                    d.pg_walls, d.pg_agent, d.pg_rng_s, d.pg_rng_b, d.pg_valid, d.pg_ring, d.rflag, d.bflag,
                    e->diff_buf, e->lv_flags, (void *)d.lv_walls, (void *)d.lv_agent, (void *)d.lv_cdf, d.lv_count, d.lv_cur};
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
    delete e;
    return MERLIN_OK;
}

int merlin_env_num_envs(const merlin_env *e) { return e ? e->dev.n : -1; }
int merlin_env_size(const merlin_env *e) { return e ? e->dev.size : -1; }

// head = count = 0 for every env: the rings' maps are stale (new seeds, new classes, a new depth)
static hipError_t drop_lookahead(merlin_env *e, hipStream_t s) {
    const size_t N = (size_t)e->dev.n;
    hipError_t err = merlin::zero_async(e->dev.pg_valid, N, s);
    if (err == hipSuccess) err = merlin::zero_async(e->dev.pg_ring, N * sizeof(uint32_t), s);
    e->seed_slots_full = false;
    return err;
}

int merlin_env_seed(merlin_env *e, const uint64_t *seeds, int32_t n, void *stream) {
    if (!e || !seeds) return fail(MERLIN_E_INVALID, "null argument");
    if (n != e->dev.n) return fail(MERLIN_E_INVALID, "seed count must equal num_envs");
    hipStream_t s = (hipStream_t)stream;
    const size_t N = (size_t)n;
    ulonglong2 *st = new ulonglong2[N];
    ulonglong2 *inc = new ulonglong2[N];
    for (size_t i = 0; i < N; i++) {
        U128 a, b;
        seed_pcg64(seeds[i], a, b);
        st[i] = make_ulonglong2(a.lo, a.hi);
        inc[i] = make_ulonglong2(b.lo, b.hi);
    }
    hipError_t err = hipMemcpyAsync(e->dev.rng_s, st, N * sizeof(ulonglong2), hipMemcpyHostToDevice, s);
    if (err == hipSuccess)
        err = hipMemcpyAsync(e->dev.rng_i, inc, N * sizeof(ulonglong2), hipMemcpyHostToDevice, s);
    if (err == hipSuccess) err = merlin::zero_async(e->dev.rng_b, N * sizeof(uint2), s);
    if (err == hipSuccess) err = drop_lookahead(e, s);  // look-ahead maps are stale
    e->seed_slots_full = false;
    if (err == hipSuccess) err = hipStreamSynchronize(s);  // host staging buffers are freed below
    delete[] st;
    delete[] inc;
    if (err != hipSuccess) return hip_fail(err, "merlin_env_seed");
    return MERLIN_OK;
}

int merlin_env_set_difficulties(merlin_env *e, const int32_t *diff, int32_t n, void *stream) {
    if (!e) return fail(MERLIN_E_INVALID, "null env");
    hipStream_t s = (hipStream_t)stream;
    const size_t N = (size_t)e->dev.n;
    hipError_t err = hipSuccess;
    uint8_t *host = nullptr;
    if (diff) {
        if (n != e->dev.n) return fail(MERLIN_E_INVALID, "difficulty count must equal num_envs");
        for (size_t i = 0; i < N; i++) {
            if (diff[i] < MERLIN_EASY || diff[i] > MERLIN_HARDEST) return fail(MERLIN_E_INVALID, "unknown difficulty");
            if (diff[i] == MERLIN_HARDEST && e->dev.size < 8)  // merlin_env_create's rule
                return fail(MERLIN_E_UNSUPPORTED, "hardest needs size >= 8 (integers(2, size/2 - 1) is empty below)");
        }
        host = new uint8_t[N];
        for (size_t i = 0; i < N; i++) host[i] = (uint8_t)diff[i];
        err = hipMemcpyAsync(e->diff_buf, host, N, hipMemcpyHostToDevice, s);
        e->dev.diff = e->diff_buf;
    } else {
        e->dev.diff = nullptr;
    }
    if (err == hipSuccess) err = drop_lookahead(e, s);  // look-ahead maps are stale
    e->seed_slots_full = false;
    if (err == hipSuccess) err = hipStreamSynchronize(s);  // the host staging buffer is freed below
    delete[] host;
    if (err != hipSuccess) return hip_fail(err, "merlin_env_set_difficulties");
    return MERLIN_OK;
}

static void free_levels(merlin_env *e) {
    merlin::EnvDev &d = e->dev;
    void *ptrs[] = {(void *)d.lv_walls, (void *)d.lv_agent, (void *)d.lv_cdf, d.lv_count, d.lv_cur, e->lv_flags};
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
    e->lv_flags = nullptr;
    d.lv_n = 0;
    d.lv_walls = nullptr;
    d.lv_agent = nullptr;
    d.lv_cdf = nullptr;
    d.lv_count = nullptr;
    d.lv_cur = nullptr;
    d.lv_seed = 0;
    d.lv_off = 0;
    e->level_log = nullptr;
}

int merlin_env_set_levels(merlin_env *e, const uint32_t *walls, const int32_t *goal, const int32_t *agent, int64_t L,
                          uint64_t level_seed, int64_t env_offset, void *stream) {
    if (!e) return fail(MERLIN_E_INVALID, "null env");
    hipStream_t s = (hipStream_t)stream;
    const bool unbind = L == 0 || !walls || !goal || !agent;
    if (!unbind && (L < 1 || L > (1 << 20))) return fail(MERLIN_E_INVALID, "the level count must be in [1, 2^20]");
    if (!unbind && e->dev.reseed)
        return fail(MERLIN_E_UNSUPPORTED, "level mode on a reseed_each_reset context (every reset replays one seed)");
    HIP_TRY(hipStreamSynchronize(s));  // nothing queued on the stream reads the old bank
    free_levels(e);
    if (unbind) return MERLIN_OK;
    merlin::EnvDev &d = e->dev;
    const size_t n = (size_t)d.n, l = (size_t)L;
    hipError_t err = hipMalloc((void **)&d.lv_walls, l * d.sp * sizeof(uint32_t));
    if (err == hipSuccess) err = hipMalloc((void **)&d.lv_agent, l * sizeof(uint4));
    if (err == hipSuccess) err = hipMalloc((void **)&d.lv_cdf, l * sizeof(double));
    if (err == hipSuccess) err = hipMalloc((void **)&d.lv_count, n * sizeof(uint32_t));
    if (err == hipSuccess) err = hipMalloc((void **)&d.lv_cur, n * sizeof(int32_t));
    if (err == hipSuccess) err = hipMalloc((void **)&e->lv_flags, l);
    if (err == hipSuccess) {
        d.lv_n = (int)L;
        d.lv_seed = level_seed;
        d.lv_off = env_offset;
        err = merlin::launch_level_bind(d, walls, goal, agent, s);
    }
    if (err == hipSuccess) err = hipStreamSynchronize(s);
    if (err != hipSuccess) {
        free_levels(e);
        return hip_fail(err, "merlin_env_set_levels");
    }
    return MERLIN_OK;
}

int merlin_env_set_level_cdf(merlin_env *e, const double *cdf, void *stream) {
    if (!e || !cdf) return fail(MERLIN_E_INVALID, "null argument");
    if (!e->dev.lv_n) return fail(MERLIN_E_INVALID, "merlin_env_set_level_cdf before merlin_env_set_levels");
    HIP_TRY(hipMemcpyAsync(const_cast<double *>(e->dev.lv_cdf), cdf, (size_t)e->dev.lv_n * sizeof(double),
                           hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return MERLIN_OK;
}

int merlin_env_levels(merlin_env *e, int32_t *cur, uint32_t *count, void *stream) {
    if (!e) return fail(MERLIN_E_INVALID, "null env");
    if (!e->dev.lv_n) return fail(MERLIN_E_INVALID, "merlin_env_levels before merlin_env_set_levels");
    if (!cur && !count) return MERLIN_OK;
    HIP_TRY(merlin::launch_env_levels(e->dev, cur, count, (hipStream_t)stream));
    return MERLIN_OK;
}

int merlin_env_set_level_log(merlin_env *e, int32_t *log) {
    if (!e) return fail(MERLIN_E_INVALID, "null env");
    if (log && !e->dev.lv_n) return fail(MERLIN_E_INVALID, "merlin_env_set_level_log before merlin_env_set_levels");
    e->level_log = log;
    return MERLIN_OK;
}

int merlin_env_replace_levels(merlin_env *e, const int32_t *slot, const uint32_t *walls, const int32_t *goal,
                              const int32_t *agent, int64_t C, void *stream) {
    if (!e) return fail(MERLIN_E_INVALID, "null env");
    if (!e->dev.lv_n) return fail(MERLIN_E_INVALID, "merlin_env_replace_levels before merlin_env_set_levels");
    if (C < 0) return fail(MERLIN_E_INVALID, "negative child count");
    if (C == 0) return MERLIN_OK;
    if (!slot || !walls || !goal || !agent) return fail(MERLIN_E_INVALID, "null argument");
    HIP_TRY(merlin::launch_level_replace(e->dev, slot, walls, goal, agent, C, e->lv_flags, (hipStream_t)stream));
    return MERLIN_OK;
}

int merlin_env_level_bank(merlin_env *e, uint32_t *walls, int32_t *goal, int32_t *agent, void *stream) {
    if (!e) return fail(MERLIN_E_INVALID, "null env");
    if (!e->dev.lv_n) return fail(MERLIN_E_INVALID, "merlin_env_level_bank before merlin_env_set_levels");
    if (!walls && !goal && !agent) return MERLIN_OK;
    merlin::EnvDev bank = e->dev;  // the bank holds its maps as the envs hold theirs: merlin_env_snapshot's kernel reads it
    bank.n = bank.lv_n;
    bank.walls = const_cast<uint32_t *>(bank.lv_walls);
    bank.agent = const_cast<uint4 *>(bank.lv_agent);
    HIP_TRY(merlin::launch_env_snapshot(bank, walls, goal, agent, (hipStream_t)stream));
    return MERLIN_OK;
}

static int mutate_args(int64_t P, const int32_t *parent, int64_t C, int32_t size, int32_t edits, bool required) {
    const char *range = (edits < 0 || edits > 64) ? "edits must be in [0, 64]" : P < 0 ? "negative parent count" : nullptr;
    const int rc = map_args(size, range, C, "negative child count", required);
    if (rc) return rc;
    if (!parent && C > P) return fail(MERLIN_E_INVALID, "without a parent index, C <= P");
    return 0;
}

int merlin_levels_mutate(const uint32_t *walls, const int32_t *goal, const int32_t *agent, int64_t P,
                         const int32_t *parent, int64_t C, int32_t size, int32_t edits, uint64_t edit_seed,
                         uint64_t generation, uint32_t *out_walls, int32_t *out_goal, int32_t *out_agent, int32_t *dist,
                         uint8_t *changed, void *stream) {
    ARGS_TRY(mutate_args(P, parent, C, size, edits,
                         walls && goal && agent && out_walls && out_goal && out_agent && dist && changed));
    HIP_TRY(merlin::launch_levels_mutate(walls, goal, agent, P, parent, C, size, edits, edit_seed, generation, out_walls,
                                         out_goal, out_agent, dist, changed, (hipStream_t)stream));
    return MERLIN_OK;
}

int merlin_levels_mutate_host(const uint32_t *walls, const int32_t *goal, const int32_t *agent, int64_t P,
                              const int32_t *parent, int64_t C, int32_t size, int32_t edits, uint64_t edit_seed,
                              uint64_t generation, uint32_t *out_walls, int32_t *out_goal, int32_t *out_agent,
                              int32_t *dist, uint8_t *changed) {
    ARGS_TRY(mutate_args(P, parent, C, size, edits,
                         walls && goal && agent && out_walls && out_goal && out_agent && dist && changed));
    merlin::levels_mutate_host(walls, goal, agent, P, parent, C, size, edits, edit_seed, generation, out_walls, out_goal,
                               out_agent, dist, changed);
    return MERLIN_OK;
}

int merlin_level_draw_host(uint64_t level_seed, int64_t env_first, int64_t n, int64_t k_first, int64_t k_count,
                           const double *cdf, int64_t L, int32_t *out) {
    if (n < 0 || k_count < 0) return fail(MERLIN_E_INVALID, "negative count");
    if (L < 1 || L > (1 << 20)) return fail(MERLIN_E_INVALID, "the level count must be in [1, 2^20]");
    if (n == 0 || k_count == 0) return MERLIN_OK;
    if (!cdf || !out) return fail(MERLIN_E_INVALID, "null argument");
    for (int64_t i = 0; i < n; i++)
        for (int64_t k = 0; k < k_count; k++)
            out[i * k_count + k] =
                merlin::level_draw(cdf, (int)L, level_seed, (uint64_t)(k_first + k), (uint64_t)(env_first + i));
    return MERLIN_OK;
}

static int level_scores_args(const float *adv, const int32_t *level, int32_t T, int32_t N, int64_t L, int32_t kind,
                             const int64_t *sum, const int64_t *count) {
    if (T < 0 || N < 0) return fail(MERLIN_E_INVALID, "negative step or env count");
    if ((int64_t)T * N > (1 << 24)) return fail(MERLIN_E_INVALID, "T * N must be <= 2^24 (the int64 sums' headroom)");
    if (L < 1 || L > (1 << 20)) return fail(MERLIN_E_INVALID, "the level count must be in [1, 2^20]");
    if (kind != 0 && kind != 1) return fail(MERLIN_E_INVALID, "kind: 0 (L1 value loss) or 1 (positive value loss)");
    if (!sum || !count || ((int64_t)T * N > 0 && (!adv || !level))) return fail(MERLIN_E_INVALID, "null argument");
    return MERLIN_OK;
}

int merlin_level_scores(const float *adv, const int32_t *level, int32_t T, int32_t N, int64_t L, int32_t kind,
                        int64_t *sum, int64_t *count, int32_t accumulate, void *stream) {
    const int rc = level_scores_args(adv, level, T, N, L, kind, sum, count);
    if (rc) return rc;
    HIP_TRY(merlin::launch_level_scores(adv, level, T, N, (int)L, kind, sum, count, accumulate, (hipStream_t)stream));
    return MERLIN_OK;
}

int merlin_level_scores_host(const float *adv, const int32_t *level, int32_t T, int32_t N, int64_t L, int32_t kind,
                             int64_t *sum, int64_t *count, int32_t accumulate) {
    const int rc = level_scores_args(adv, level, T, N, L, kind, sum, count);
    if (rc) return rc;
    merlin::level_scores_host(adv, level, T, N, (int)L, kind, sum, count, accumulate);
    return MERLIN_OK;
}

int merlin_env_reset(merlin_env *e, const uint8_t *mask, uint32_t *obs, void *stream) {
    if (!e) return fail(MERLIN_E_INVALID, "null env");
    // + look-ahead refill; a deeper ring whose refills are the caller's (interval 0) is topped up by the caller too
    const bool refill = e->dev.pg_depth == 1 || e->refill_every > 0;
    HIP_TRY(merlin::launch_env_reset(e->dev, mask, obs, refill, (hipStream_t)stream));
    e->steps_since_refill = 0;
    if (!mask) {
        e->has_state = true;
        // the reset's full refill filled every slot with its seed map
        e->seed_slots_full = e->dev.reseed != 0 && refill;
    }
    return MERLIN_OK;
}

int merlin_env_step(merlin_env *e, const int64_t *actions, int32_t n_steps, int64_t action_stride,
                    uint32_t *obs, float *reward, uint8_t *term, uint8_t *trunc, float *done,
                    double *ep_ret, int32_t *ep_len, int32_t autoreset, void *stream) {
    if (!e || !actions) return fail(MERLIN_E_INVALID, "null argument");
    if (!e->has_state) return fail(MERLIN_E_INVALID, "merlin_env_step before merlin_env_reset");
    if (n_steps <= 0) return MERLIN_OK;
    if (action_stride < e->dev.n && n_steps > 1)
        return fail(MERLIN_E_INVALID, "action_stride must be >= num_envs");
    merlin::StepOut o{};
    o.actions = actions;
    o.action_stride = action_stride;
    o.n_steps = n_steps;
    o.autoreset = autoreset;
    o.obs = obs;
    o.reward = reward;
    o.term = term;
    o.trunc = trunc;
    o.done = done;
    o.ep_ret_out = ep_ret;
    o.ep_len_out = ep_len;
    const bool refill = !e->seed_slots_full && e->refill_every > 0 && ++e->steps_since_refill >= e->refill_every;
    if (refill) e->steps_since_refill = 0;
    o.no_fallback = e->seed_slots_full || (e->no_fallback && e->refill_every == 0);
    o.level_log = e->level_log;
    HIP_TRY(merlin::launch_env_step(e->dev, o, refill, (hipStream_t)stream));
    return MERLIN_OK;
}

int merlin_env_act_step(merlin_env *e, const float *head_part, int32_t n_parts, const float *b_actor,
                        const float *b_critic, int32_t act_dim, int32_t deterministic, uint64_t seed,
                        const int64_t *epoch, int64_t step, int64_t env_offset, int64_t *action, float *logp,
                        float *value, uint32_t *obs, float *reward, uint8_t *term, uint8_t *trunc, float *done,
                        double *ep_ret, int32_t *ep_len, void *stream) {
    if (!e || !head_part || !b_actor || !b_critic || !action || !logp || !value)
        return fail(MERLIN_E_INVALID, "null argument");
    if (!e->has_state) return fail(MERLIN_E_INVALID, "merlin_env_act_step before merlin_env_reset");
    if (n_parts < 1 || act_dim < 1 || act_dim > 4) return fail(MERLIN_E_INVALID, "n_parts >= 1, act_dim in [1, 4]");
    if (!deterministic && !epoch) return fail(MERLIN_E_INVALID, "a sampled action needs the epoch counter");
    merlin::StepOut o{};
    o.actions = action;
    o.action_stride = e->dev.n;
    o.n_steps = 1;
    o.autoreset = 1;
    o.obs = obs;
    o.reward = reward;
    o.term = term;
    o.trunc = trunc;
    o.done = done;
    o.ep_ret_out = ep_ret;
    o.ep_len_out = ep_len;
    o.act = merlin::ActIn{reinterpret_cast<const float4 *>(head_part), n_parts, b_actor, b_critic, act_dim,
                          deterministic ? 1 : 0, seed, epoch, step, env_offset, action, logp, value};
    const bool refill = !e->seed_slots_full && e->refill_every > 0 && ++e->steps_since_refill >= e->refill_every;
    if (refill) e->steps_since_refill = 0;
    o.no_fallback = e->seed_slots_full || (e->no_fallback && e->refill_every == 0);
    o.level_log = e->level_log;
    HIP_TRY(merlin::launch_env_step(e->dev, o, refill, (hipStream_t)stream));
    return MERLIN_OK;
}

int merlin_group_act(const uint32_t *codes, int32_t groups, const float *T2, const float *b2, const float *W3t,
                     const float *b3, const float *W4p, const float *b4, const float *Wa, const float *ba,
                     const float *Wc, const float *bc, int32_t act_dim, float *a3_ws, float *head_part,
                     int32_t shared_weights, void *stream) {
    if (groups < 0) return fail(MERLIN_E_INVALID, "negative group count");
    if (act_dim < 1 || act_dim > 4) return fail(MERLIN_E_INVALID, "act_dim must be in [1, 4]");
    if (groups > 0 && (!codes || !T2 || !b2 || !W3t || !b3 || !W4p || !b4 || !Wa || !ba || !Wc || !bc || !a3_ws ||
                       !head_part))
        return fail(MERLIN_E_INVALID, "null argument");
    HIP_TRY(merlin::launch_group_act(codes, groups, T2, b2, W3t, b3, W4p, b4, Wa, ba, Wc, bc, act_dim, a3_ws,
                                     head_part, shared_weights != 0, (hipStream_t)stream));
    return MERLIN_OK;
}

int merlin_env_set_step_fallback(merlin_env *e, int32_t on) {
    if (!e) return fail(MERLIN_E_INVALID, "null env");
    e->no_fallback = on == 0;
    return MERLIN_OK;
}

int merlin_env_set_refill_interval(merlin_env *e, int32_t every) {
    if (!e) return fail(MERLIN_E_INVALID, "null env");
    if (every < 0) return fail(MERLIN_E_INVALID, "refill interval must be >= 0");
    e->refill_every = every;
    e->steps_since_refill = 0;
    return MERLIN_OK;
}

int merlin_env_refill(merlin_env *e, void *stream) {
    if (!e) return fail(MERLIN_E_INVALID, "null env");
    // a deeper ring is the caller's to top up between runs of steps, when most envs have used a map or several:
    // one wave per 64 envs, all generating at once, as after a full reset
    HIP_TRY(merlin::launch_env_refill(e->dev, e->dev.pg_depth > 1, (hipStream_t)stream));
    return MERLIN_OK;
}

int merlin_env_set_lookahead_depth(merlin_env *e, int32_t depth) {
    if (!e) return fail(MERLIN_E_INVALID, "null env");
    if (depth < 1 || depth > 65535) return fail(MERLIN_E_INVALID, "look-ahead depth must be in [1, 65535]");
    merlin::EnvDev &d = e->dev;
    HIP_TRY(hipDeviceSynchronize());  // nothing in flight reads the old ring (fails inside a capture)
    const size_t slots = (size_t)d.n * (size_t)depth;
    void *p[4] = {nullptr, nullptr, nullptr, nullptr};
    const size_t bytes[4] = {slots * d.sp * sizeof(uint32_t), slots * sizeof(uint4), slots * sizeof(ulonglong2),
                             slots * sizeof(uint2)};
    hipError_t err = hipSuccess;
    for (int k = 0; k < 4 && err == hipSuccess; k++) {
        err = hipMalloc(&p[k], bytes[k]);
        if (err == hipSuccess) err = hipMemset(p[k], 0, bytes[k]);
    }
    if (err != hipSuccess) {  // the env keeps the ring it had
        for (void *q : p)
            if (q) (void)hipFree(q);
        return hip_fail(err, "hipMalloc(look-ahead ring)");
    }
    void *old[4] = {d.pg_walls, d.pg_agent, d.pg_rng_s, d.pg_rng_b};
    for (void *q : old) (void)hipFree(q);
    d.pg_walls = (uint32_t *)p[0];
    d.pg_agent = (uint4 *)p[1];
    d.pg_rng_s = (ulonglong2 *)p[2];
    d.pg_rng_b = (uint2 *)p[3];
    d.pg_depth = depth;
    e->steps_since_refill = 0;
    HIP_TRY(drop_lookahead(e, nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));
    return MERLIN_OK;
}

int merlin_env_full_obs(merlin_env *e, uint8_t *out, void *stream) {
    if (!e || !out) return fail(MERLIN_E_INVALID, "null argument");
    HIP_TRY(merlin::launch_env_full_obs(e->dev, out, (hipStream_t)stream));
    return MERLIN_OK;
}

int merlin_env_get_state(merlin_env *e, uint32_t *walls, int32_t *agent, uint64_t *rng, void *stream) {
    if (!e) return fail(MERLIN_E_INVALID, "null env");
    hipStream_t s = (hipStream_t)stream;
    const merlin::EnvDev &d = e->dev;
    const size_t n = (size_t)d.n;
    if (walls) {
        uint32_t *tmp = new uint32_t[n * d.sp];
        hipError_t err = hipMemcpyAsync(tmp, d.walls, n * d.sp * 4, hipMemcpyDeviceToHost, s);
        if (err == hipSuccess) err = hipStreamSynchronize(s);
        if (err == hipSuccess)
            for (size_t i = 0; i < n; i++)
                for (int y = 0; y < d.size; y++) walls[i * d.size + y] = tmp[i * d.sp + y];
        delete[] tmp;
        if (err != hipSuccess) return hip_fail(err, "get_state(walls)");
    }
    if (agent) {
        uint4 *tmp = new uint4[n];
        hipError_t err = hipMemcpyAsync(tmp, d.agent, n * sizeof(uint4), hipMemcpyDeviceToHost, s);
        if (err == hipSuccess) err = hipStreamSynchronize(s);
        if (err == hipSuccess)
            for (size_t i = 0; i < n; i++) {
                int32_t *a = agent + i * 8;
                a[0] = tmp[i].x & 0xff;
                a[1] = (tmp[i].x >> 8) & 0xff;
                a[2] = (tmp[i].x >> 16) & 3;
                a[3] = (int32_t)tmp[i].y;
                a[4] = tmp[i].z & 0xff;
                a[5] = (tmp[i].z >> 8) & 0xff;
                a[6] = (int32_t)(tmp[i].w >> 16);
                a[7] = 0;
            }
        delete[] tmp;
        if (err != hipSuccess) return hip_fail(err, "get_state(agent)");
    }
    if (rng) {
        ulonglong2 *a = new ulonglong2[n], *b = new ulonglong2[n];
        uint2 *c = new uint2[n];
        hipError_t err = hipMemcpyAsync(a, d.rng_s, n * sizeof(ulonglong2), hipMemcpyDeviceToHost, s);
        if (err == hipSuccess) err = hipMemcpyAsync(b, d.rng_i, n * sizeof(ulonglong2), hipMemcpyDeviceToHost, s);
        if (err == hipSuccess) err = hipMemcpyAsync(c, d.rng_b, n * sizeof(uint2), hipMemcpyDeviceToHost, s);
        if (err == hipSuccess) err = hipStreamSynchronize(s);
        if (err == hipSuccess)
            for (size_t i = 0; i < n; i++) {
                uint64_t *r = rng + i * 5;
                r[0] = a[i].y;
                r[1] = a[i].x;
                r[2] = b[i].y;
                r[3] = b[i].x;
                r[4] = ((uint64_t)c[i].x << 32) | c[i].y;
            }
        delete[] a;
        delete[] b;
        delete[] c;
        if (err != hipSuccess) return hip_fail(err, "get_state(rng)");
    }
    return MERLIN_OK;
}

int merlin_env_errors(merlin_env *e, uint32_t *flags, uint32_t *fallbacks, void *stream) {
    if (!e) return fail(MERLIN_E_INVALID, "null env");
    hipStream_t s = (hipStream_t)stream;
    uint32_t h[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(h, e->dev.err, sizeof(h), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(merlin::zero_async(e->dev.err, sizeof(h), s));
    if (flags) *flags = h[0];
    if (fallbacks) *fallbacks = h[1];
    return MERLIN_OK;
}

int merlin_obs_expand_f32(const uint32_t *codes, const int64_t *index, int64_t n, float *out, float scale,
                          int32_t layout, void *stream) {
    if ((!codes || !out) && n > 0) return fail(MERLIN_E_INVALID, "null argument");
    if (layout != MERLIN_LAYOUT_NCHW && layout != MERLIN_LAYOUT_NHWC)
        return fail(MERLIN_E_INVALID, "unknown layout");
    DeviceWs *ws = nullptr;
    int rc = device_ws(&ws);
    if (rc) return rc;
    HIP_TRY(merlin::launch_obs_expand_f32(codes, index, n, out, scale, layout, (hipStream_t)stream));
    return MERLIN_OK;
}

int merlin_obs_expand_u8(const uint32_t *codes, const int64_t *index, int64_t n, uint8_t *out, void *stream) {
    if ((!codes || !out) && n > 0) return fail(MERLIN_E_INVALID, "null argument");
    DeviceWs *ws = nullptr;
    int rc = device_ws(&ws);
    if (rc) return rc;
    HIP_TRY(merlin::launch_obs_expand_u8(codes, index, n, out, (hipStream_t)stream));
    return MERLIN_OK;
}

int merlin_gae(const float *rew, const float *val, const float *done, const float *last, float *adv,
               float *ret, int32_t T, int32_t N, double gamma, double lam, double *stats, void *stream) {
    if (!rew || !val || !done || !last || !adv || !ret) return fail(MERLIN_E_INVALID, "null argument");
    if (T <= 0 || N <= 0) return fail(MERLIN_E_INVALID, "T and N must be > 0");
    DeviceWs *ws = nullptr;
    int rc = device_ws(&ws);
    if (rc) return rc;
    if (stats && merlin::gae_partials_needed(T, N) > ws->max_partials)
        return fail(MERLIN_E_UNSUPPORTED, "too many envs for the GAE stats workspace");
    HIP_TRY(merlin::launch_gae(rew, val, done, last, adv, ret, T, N, gamma, lam, stats, ws->partials,
                               ws->max_partials, (hipStream_t)stream));
    return MERLIN_OK;
}

int merlin_adv_normalize(const float *adv, int64_t n, const double *stats, float *out, void *stream) {
    if (!adv || !stats || !out) return fail(MERLIN_E_INVALID, "null argument");
    HIP_TRY(merlin::launch_adv_normalize(adv, n, stats, out, (hipStream_t)stream));
    return MERLIN_OK;
}

int merlin_conv1_lut_fwd(const uint32_t *codes, const int64_t *index, int64_t n, const float *tables,
                         const float *bias, int32_t towers, float *out, void *stream) {
    if ((!codes || !tables || !bias || !out) && n > 0) return fail(MERLIN_E_INVALID, "null argument");
    if (towers < 1 || towers > 2) return fail(MERLIN_E_INVALID, "towers must be 1 or 2");
    HIP_TRY(merlin::launch_conv1_lut_fwd(codes, index, n, tables, bias, towers, out, (hipStream_t)stream));
    return MERLIN_OK;
}

int merlin_conv1_lut_bwd(const uint32_t *codes, const int64_t *index, int64_t n, const float *act,
                         const float *grad, int32_t towers, float *dtables, float *dbias, void *stream) {
    if (!dtables || !dbias || ((!codes || !act || !grad) && n > 0)) return fail(MERLIN_E_INVALID, "null argument");
    if (towers < 1 || towers > 2) return fail(MERLIN_E_INVALID, "towers must be 1 or 2");
    DeviceWs *ws = nullptr;
    int rc = device_ws(&ws);
    if (rc) return rc;
    HIP_TRY(merlin::launch_conv1_lut_bwd(codes, index, n, act, grad, towers, dtables, dbias, ws->conv1_slabs,
                                         ws->max_slabs, (hipStream_t)stream));
    return MERLIN_OK;
}

int merlin_tower_conv2_im2col_fwd(const uint32_t *codes, const int64_t *index, int64_t n, const float *tables,
                                  const float *bias, int32_t towers, float *A2, void *stream) {
    if ((!codes || !tables || !bias || !A2) && n > 0) return fail(MERLIN_E_INVALID, "null argument");
    if (towers < 1 || towers > 2) return fail(MERLIN_E_INVALID, "towers must be 1 or 2");
    HIP_TRY(merlin::launch_conv1_im2col_fwd(codes, index, n, tables, bias, towers, A2, (hipStream_t)stream));
    return MERLIN_OK;
}

int merlin_tower_conv2_im2col_bwd(const uint32_t *codes, const int64_t *index, int64_t n, const float *tables,
                                  const float *bias, const float *dA2, int32_t towers, float *dtables,
                                  float *dbias, void *stream) {
    if (!dtables || !dbias || ((!codes || !tables || !bias || !dA2) && n > 0))
        return fail(MERLIN_E_INVALID, "null argument");
    if (towers < 1 || towers > 2) return fail(MERLIN_E_INVALID, "towers must be 1 or 2");
    DeviceWs *ws = nullptr;
    int rc = device_ws(&ws);
    if (rc) return rc;
    HIP_TRY(merlin::launch_conv1_im2col_bwd(codes, index, n, tables, bias, dA2, towers, dtables, dbias,
                                            ws->conv1_slabs, ws->max_slabs, (hipStream_t)stream));
    return MERLIN_OK;
}

int merlin_tower_conv3_im2col_fwd(const float *Z2, const float *b2, int64_t n, int32_t towers, float *A3,
                                  void *stream) {
    if ((!Z2 || !b2 || !A3) && n > 0) return fail(MERLIN_E_INVALID, "null argument");
    HIP_TRY(merlin::launch_im2col3_fwd(Z2, b2, n, towers, A3, (hipStream_t)stream));
    return MERLIN_OK;
}

int merlin_tower_conv3_col2im_bwd(const float *dA3, const float *Z2, const float *b2, int64_t n, int32_t towers,
                                  float *dZ2, void *stream) {
    if ((!dA3 || !Z2 || !b2 || !dZ2) && n > 0) return fail(MERLIN_E_INVALID, "null argument");
    HIP_TRY(merlin::launch_col2im3_bwd(dA3, Z2, b2, n, towers, 0, dZ2, nullptr, (hipStream_t)stream));
    return MERLIN_OK;
}

int merlin_tower_conv3_col2im_bwd_chunked(const float *dA3, const float *Z2, const float *b2, int64_t n,
                                          int32_t towers, float *dZ2c, uint32_t *absmax, void *stream) {
    if (!absmax || ((!dA3 || !Z2 || !b2 || !dZ2c) && n > 0)) return fail(MERLIN_E_INVALID, "null argument");
    if (towers < 1) return fail(MERLIN_E_INVALID, "towers must be >= 1");
    HIP_TRY(merlin::launch_col2im3_bwd(dA3, Z2, b2, n, towers, 1, dZ2c, absmax, (hipStream_t)stream));
    return MERLIN_OK;
}

int merlin_tower_conv2_lut_rows(void) { return merlin::conv2_lut_rows(); }

int merlin_tower_conv2_lut_fwd(const uint32_t *codes, const int64_t *index, int64_t n, const float *tables,
                               int32_t towers, float *Z2, void *stream) {
    if ((!codes || !tables || !Z2) && n > 0) return fail(MERLIN_E_INVALID, "null argument");
    if (towers < 1 || towers > 2) return fail(MERLIN_E_INVALID, "towers must be 1 or 2");
    HIP_TRY(merlin::launch_conv2_lut_fwd(codes, index, n, tables, towers, Z2, (hipStream_t)stream));
    return MERLIN_OK;
}

int merlin_tower_conv2_lut_bwd(const uint32_t *codes, int64_t n, const float *dZ2c, const uint32_t *absmax,
                               int32_t towers, float *dtables, void *stream) {
    if (!dtables || ((!codes || !dZ2c || !absmax) && n > 0)) return fail(MERLIN_E_INVALID, "null argument");
    if (towers < 1 || towers > 2) return fail(MERLIN_E_INVALID, "towers must be 1 or 2");
    DeviceWs *ws = nullptr;
    int rc = device_ws(&ws);
    if (rc) return rc;
    HIP_TRY(merlin::launch_conv2_lut_bwd(codes, n, dZ2c, absmax, towers, dtables, ws->lut2_slabs,
                                         (hipStream_t)stream));
    return MERLIN_OK;
}

int merlin_tower_conv2_lut_fwd_grouped(const uint32_t *codes, int64_t n, int64_t group_frames, const float *tables,
                                       int32_t towers, float *Z2, void *stream) {
    if ((!codes || !tables || !Z2) && n > 0) return fail(MERLIN_E_INVALID, "null argument");
    if (towers < 2 || towers % 2 || group_frames <= 0) return fail(MERLIN_E_INVALID, "bad grouping");
    if (n != (int64_t)(towers / 2) * group_frames) return fail(MERLIN_E_INVALID, "n != groups * group_frames");
    HIP_TRY(merlin::launch_conv2_lut_fwd(codes, nullptr, n, tables, towers, Z2, (hipStream_t)stream, group_frames));
    return MERLIN_OK;
}

int64_t merlin_tower_conv2_lut_slab_bytes(int32_t towers, int64_t group_frames) {
    return (int64_t)merlin::conv2_lut_slab_bytes(towers, merlin::conv2_lut_fblocks(group_frames));
}

int merlin_tower_conv2_lut_bwd_grouped(const uint32_t *codes, int64_t group_frames, const float *dZ2c,
                                       const uint32_t *absmax, int32_t towers, float *dtables, void *slabs,
                                       void *stream) {
    if (!dtables || ((!codes || !dZ2c || !absmax || !slabs) && group_frames > 0))
        return fail(MERLIN_E_INVALID, "null argument");
    if (towers < 2 || towers % 2) return fail(MERLIN_E_INVALID, "bad grouping");
    HIP_TRY(merlin::launch_conv2_lut_bwd(codes, group_frames, dZ2c, absmax, towers, dtables, slabs,
                                         (hipStream_t)stream, group_frames));
    return MERLIN_OK;
}

int merlin_tower_window_lut(const int32_t *rows, int64_t nw, const float *tables, int32_t towers, float *Z2w,
                            void *stream) {
    if ((!rows || !tables || !Z2w) && nw > 0) return fail(MERLIN_E_INVALID, "null argument");
    if (towers < 1 || towers > 2) return fail(MERLIN_E_INVALID, "towers must be 1 or 2");
    HIP_TRY(merlin::launch_window_lut(rows, nw, tables, towers, Z2w, (hipStream_t)stream));
    return MERLIN_OK;
}

int merlin_minibatch_patch_maps(const int32_t *kid, const int64_t *group_keys, int64_t n_groups, int64_t n_frames,
                                const int64_t *group_offsets, int32_t n_patches, int32_t *kmap, int32_t *rmap,
                                int32_t *rep_row, void *stream) {
    if (n_groups < 0 || n_frames < 1 || n_patches < 1) return fail(MERLIN_E_INVALID, "bad shape");
    if (n_groups > 0 && (!kid || !group_keys || !group_offsets || !kmap || !rmap || !rep_row))
        return fail(MERLIN_E_INVALID, "null argument");
    if (n_groups * 9 > INT32_MAX) return fail(MERLIN_E_UNSUPPORTED, "more than 2^31 rows");
    HIP_TRY(merlin::launch_patch_maps(kid, group_keys, n_groups, n_frames, group_offsets, n_patches, kmap, rmap,
                                      rep_row, (hipStream_t)stream));
    return MERLIN_OK;
}

namespace {
// shared argument rules of the two merlin_plan_minibatches entries; the key span (minibatches * frames) or a code
int64_t plan_key_span(int64_t n, int64_t period, int64_t mbs, int64_t n_frames, int *rc) {
    *rc = MERLIN_OK;
    if (n < 1 || period < 1 || mbs < 1 || n_frames < 1 || n % period) {
        *rc = fail(MERLIN_E_INVALID, "bad shape: n must be a positive multiple of period");
        return 0;
    }
    const int64_t nmb = (n / period) * ((period + mbs - 1) / mbs);
    if (n > INT32_MAX || nmb > INT32_MAX / n_frames) {
        *rc = fail(MERLIN_E_UNSUPPORTED, "more than 2^31 samples or (minibatch, frame) keys");
        return 0;
    }
    return nmb * n_frames;
}
}  // namespace

int64_t merlin_plan_sort_workspace(int64_t n, int32_t key_bytes) {
    if (n < 1 || n > INT32_MAX || (key_bytes != 4 && key_bytes != 8)) {
        fail(MERLIN_E_INVALID, "bad sort shape");
        return -1;
    }
    const int64_t bytes = merlin::plan_sort_workspace(n, key_bytes);
    if (bytes < 0) fail(MERLIN_E_HIP, "rocprim scratch size query failed");
    return bytes;
}

namespace {
// a stage's scratch rule: its sort of n pairs with key_bytes-wide keys must fit the workspace
int plan_stage_args(int64_t n, int32_t key_bytes, const void *ws, int64_t ws_bytes, int64_t item_len, bool ptrs) {
    if (n < 1 || item_len < 1) return fail(MERLIN_E_INVALID, "bad shape");
    if (n > INT32_MAX) return fail(MERLIN_E_UNSUPPORTED, "more than 2^31 list entries");
    if (!ws || !ptrs) return fail(MERLIN_E_INVALID, "null argument");
    const int64_t need = merlin_plan_sort_workspace(n, key_bytes);
    if (need < 0) return MERLIN_E_HIP;
    if (ws_bytes < need) return fail(MERLIN_E_INVALID, "workspace smaller than merlin_plan_sort_workspace");
    return MERLIN_OK;
}
}  // namespace

int merlin_plan_frames(const uint32_t *codes, int64_t n, const uint64_t *mult_host, void *ws, int64_t ws_bytes,
                       int64_t *uid, int64_t *rep, int32_t *wkey, uint64_t *pkey, int32_t *mark, int32_t *wrank,
                       int64_t *counts, void *stream) {
    if (n > INT32_MAX / 25) return fail(MERLIN_E_UNSUPPORTED, "more than 2^31 / 25 frames");
    const int rc = plan_stage_args(n, 8, ws, ws_bytes, 1,
                                   codes && mult_host && uid && rep && wkey && pkey && mark && wrank && counts);
    if (rc != MERLIN_OK) return rc;
    HIP_TRY(merlin::launch_plan_frames(codes, n, mult_host, ws, ws_bytes, uid, rep, wkey, pkey, mark, wrank, counts,
                                       (hipStream_t)stream));
    return MERLIN_OK;
}

int merlin_plan_windows(int64_t n_frames, int64_t n_windows, const int32_t *wkey, const int32_t *mark,
                        const int32_t *wrank, int32_t lut_rows, int64_t item_len, void *ws, int64_t ws_bytes,
                        int32_t *wid, int32_t *rows, int32_t *key, int32_t *idx, int32_t *fix, int32_t *head_fix,
                        int64_t *counts, void *stream) {
    if (n_frames < 1 || n_frames > INT32_MAX / 25 || n_windows > 1953125 || lut_rows < 1)
        return fail(MERLIN_E_INVALID, "bad shape");
    const int rc = plan_stage_args(n_windows * 16, 4, ws, ws_bytes, item_len,
                                   wkey && mark && wrank && wid && rows && key && idx && fix && head_fix && counts);
    if (rc != MERLIN_OK) return rc;
    HIP_TRY(merlin::launch_plan_windows(n_frames, n_windows, wkey, mark, wrank, lut_rows, item_len, ws, ws_bytes, wid,
                                        rows, key, idx, fix, head_fix, counts, (hipStream_t)stream));
    return MERLIN_OK;
}

int merlin_plan_patches(int64_t n_frames, const uint64_t *pkey, int64_t item_len, void *ws, int64_t ws_bytes,
                        int32_t *kid, uint64_t *pk, int32_t *key, int32_t *idx, int32_t *fix, int32_t *head_fix,
                        int64_t *counts, void *stream) {
    if (n_frames < 1 || n_frames > INT32_MAX / 25) return fail(MERLIN_E_INVALID, "bad shape");
    const int rc = plan_stage_args(n_frames * 9, 8, ws, ws_bytes, item_len,
                                   pkey && kid && pk && key && idx && fix && head_fix && counts);
    if (rc != MERLIN_OK) return rc;
    HIP_TRY(merlin::launch_plan_patches(n_frames, pkey, item_len, ws, ws_bytes, kid, pk, key, idx, fix, head_fix,
                                        counts, (hipStream_t)stream));
    return MERLIN_OK;
}

int merlin_plan_bands(int64_t n_patches, const uint64_t *pk, int64_t item_len, void *ws, int64_t ws_bytes,
                      uint64_t *ub, int32_t *key, int32_t *idx, int32_t *fix, int32_t *head_fix, int64_t *counts,
                      void *stream) {
    if (n_patches < 1 || n_patches > INT32_MAX / 3) return fail(MERLIN_E_INVALID, "bad shape");
    const int rc = plan_stage_args(n_patches * 3, 8, ws, ws_bytes, item_len,
                                   pk && ub && key && idx && fix && head_fix && counts);
    if (rc != MERLIN_OK) return rc;
    HIP_TRY(merlin::launch_plan_bands(n_patches, pk, item_len, ws, ws_bytes, ub, key, idx, fix, head_fix, counts,
                                      (hipStream_t)stream));
    return MERLIN_OK;
}

int merlin_plan_dq(int64_t n_bands, int64_t n_windows, const uint64_t *ub, const int32_t *mark, const int32_t *wrank,
                   int64_t item_len, void *ws, int64_t ws_bytes, int32_t *key, int32_t *idx, int32_t *fix,
                   int32_t *head_fix, int64_t *counts, void *stream) {
    if (n_bands < 1 || n_bands > INT32_MAX / 3 || n_windows < 1 || n_windows > 1953125)
        return fail(MERLIN_E_INVALID, "bad shape");
    const int rc = plan_stage_args(n_bands * 3, 4, ws, ws_bytes, item_len,
                                   ub && mark && wrank && key && idx && fix && head_fix && counts);
    if (rc != MERLIN_OK) return rc;
    HIP_TRY(merlin::launch_plan_dq(n_bands, n_windows, ub, mark, wrank, item_len, ws, ws_bytes, key, idx, fix,
                                   head_fix, counts, (hipStream_t)stream));
    return MERLIN_OK;
}

int64_t merlin_plan_minibatches_workspace(int64_t n, int64_t period, int64_t minibatch, int64_t n_frames) {
    int rc;
    const int64_t span = plan_key_span(n, period, minibatch, n_frames, &rc);
    if (rc != MERLIN_OK) return -1;
    const int64_t bytes = merlin::plan_minibatches_workspace(n, span);
    if (bytes < 0) fail(MERLIN_E_HIP, "rocprim scratch size query failed");
    return bytes;
}

int merlin_plan_minibatches(const int64_t *idxs, int64_t n, int64_t period, int64_t minibatch, const int64_t *uid,
                            int64_t n_samples, int64_t n_frames, void *workspace, int64_t workspace_bytes,
                            int64_t *group_keys, int64_t *groups, int64_t *inv, int32_t *slot, int32_t *order,
                            int32_t *offs, int64_t *group_offsets, void *stream) {
    int rc;
    plan_key_span(n, period, minibatch, n_frames, &rc);
    if (rc != MERLIN_OK) return rc;
    if (n_samples < 1) return fail(MERLIN_E_INVALID, "bad shape");
    if (!idxs || !uid || !workspace || !group_keys || !groups || !inv || !slot || !order || !offs || !group_offsets)
        return fail(MERLIN_E_INVALID, "null argument");
    if (workspace_bytes < merlin_plan_minibatches_workspace(n, period, minibatch, n_frames))
        return fail(MERLIN_E_INVALID, "workspace smaller than merlin_plan_minibatches_workspace");
    HIP_TRY(merlin::launch_plan_minibatches(idxs, n, period, minibatch, uid, n_samples, n_frames, workspace,
                                            workspace_bytes, group_keys, groups, inv, slot, order, offs,
                                            group_offsets, (hipStream_t)stream));
    return MERLIN_OK;
}

int merlin_tower_window_lut_bias_relu(const int32_t *rows, int64_t nw, const float *tables, int32_t towers,
                                      const float *b2, float *a2w, void *stream) {
    if ((!rows || !tables || !a2w || !b2) && nw > 0) return fail(MERLIN_E_INVALID, "null argument");
    if (towers < 1 || towers > 2) return fail(MERLIN_E_INVALID, "towers must be 1 or 2");
    HIP_TRY(merlin::launch_window_lut(rows, nw, tables, towers, a2w, (hipStream_t)stream, b2));
    return MERLIN_OK;
}

int merlin_tower_window_conv3(const float *Q, int64_t nw, const int32_t *wid, const int64_t *groups, int64_t n,
                              const float *b3, int32_t towers, float *Y3, void *stream) {
    if ((!Q || !wid || !b3 || !Y3) && n > 0) return fail(MERLIN_E_INVALID, "null argument");
    if (towers < 1 || towers > 2) return fail(MERLIN_E_INVALID, "towers must be 1 or 2");
    HIP_TRY(merlin::launch_window_conv3(Q, nw, wid, groups, n, b3, towers, Y3, nullptr, nullptr, nullptr, 0,
                                        (hipStream_t)stream));
    return MERLIN_OK;
}

int merlin_tower_window_conv3_bits(const float *Q, int64_t nw, const int32_t *wid, const int64_t *groups, int64_t n,
                                   const float *b3, int32_t towers, float *Y3, uint64_t *relu_bits, uint32_t *amax,
                                   void *stream) {
    if ((!Q || !wid || !b3 || !Y3 || !relu_bits) && n > 0) return fail(MERLIN_E_INVALID, "null argument");
    if (towers < 1 || towers > 2) return fail(MERLIN_E_INVALID, "towers must be 1 or 2");
    HIP_TRY(merlin::launch_window_conv3(Q, nw, wid, groups, n, b3, towers, Y3, relu_bits, amax, nullptr, 0,
                                        (hipStream_t)stream));
    return MERLIN_OK;
}

int merlin_tower_window_conv3_reuse(const float *Q, int64_t nw, const int32_t *wid, const int64_t *groups, int64_t n,
                                    const float *b3, int32_t towers, float *Y3, uint64_t *relu_bits, uint32_t *amax,
                                    const int32_t *rep_row, int32_t copy, void *stream) {
    if ((!rep_row || !Y3 || (!(copy & 4) && (!Q || !wid || !b3))) && n > 0)
        return fail(MERLIN_E_INVALID, "null argument");
    if (towers < 1 || towers > 2) return fail(MERLIN_E_INVALID, "towers must be 1 or 2");
    if (copy < 0 || copy > 7) return fail(MERLIN_E_INVALID, "copy must be 0..7");
    HIP_TRY(merlin::launch_window_conv3(Q, nw, wid, groups, n, b3, towers, Y3, relu_bits, amax, rep_row, copy,
                                        (hipStream_t)stream));
    return MERLIN_OK;
}

int merlin_tower_window_conv3_planes(const float *Q, int64_t nw, const int32_t *wid, const int64_t *groups, int64_t n,
                                     const float *b3, int32_t towers, void *Y3_planes, uint64_t *relu_bits,
                                     const int32_t *rep_row, uint32_t *colmax_ws, uint32_t *bound, void *stream) {
    if ((!rep_row || !Y3_planes || !Q || !wid || !b3 || !relu_bits || !colmax_ws || !bound) && n > 0)
        return fail(MERLIN_E_INVALID, "null argument");
    if (towers < 1 || towers > 2) return fail(MERLIN_E_INVALID, "towers must be 1 or 2");
    if (n > 0 && nw <= 0) return fail(MERLIN_E_INVALID, "no windows");
    HIP_TRY(merlin::launch_window_conv3(Q, nw, wid, groups, n, b3, towers, static_cast<float *>(Y3_planes), relu_bits,
                                        nullptr, rep_row, 0, (hipStream_t)stream, colmax_ws, bound));
    return MERLIN_OK;
}

int64_t merlin_tower_all_windows(void) { return 458752; }  // 4^9 + 3 * 4^8 (merlin_window.hip k_codes_conv3)

int merlin_tower_codes_conv3_amax(const uint32_t *codes, int64_t n, const float *Qall, const float *b3,
                                  int32_t towers, float *Y3, uint32_t *amax, void *stream) {
    if ((!codes || !Qall || !b3 || !Y3) && n > 0) return fail(MERLIN_E_INVALID, "null argument");
    if (towers < 1 || towers > 2) return fail(MERLIN_E_INVALID, "towers must be 1 or 2");
    DeviceWs *ws = nullptr;
    if (int r = device_ws(&ws)) return r;
    HIP_TRY(merlin::launch_codes_conv3(codes, n, Qall, b3, towers, Y3, amax, ws->tower_err, (hipStream_t)stream));
    return MERLIN_OK;
}

int merlin_tower_errors(uint32_t *flags, void *stream) {
    DeviceWs *ws = nullptr;
    if (int r = device_ws(&ws)) return r;
    hipStream_t s = (hipStream_t)stream;
    uint32_t h = 0;
    HIP_TRY(hipMemcpyAsync(&h, ws->tower_err, sizeof(h), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(merlin::zero_async(ws->tower_err, sizeof(h), s));
    if (flags) *flags = h;
    return MERLIN_OK;
}

int merlin_tower_codes_conv3(const uint32_t *codes, int64_t n, const float *Qall, const float *b3, int32_t towers,
                             float *Y3, void *stream) {
    return merlin_tower_codes_conv3_amax(codes, n, Qall, b3, towers, Y3, nullptr, stream);
}

static int segment_sum_fused(const float *src, const void *mask, int64_t src_rows, const int32_t *idx,
                             const int32_t *key, int64_t nnz, const int32_t *slot, int32_t sub, int64_t item_len,
                             const int32_t *fix, int64_t n_fix, int32_t towers, float *out, int64_t out_rows,
                             float *carry, int32_t flags, int32_t *mark, const int32_t *head_fix, int32_t *counters,
                             const int32_t *mask_rows, void *stream) {
    if (!out && out_rows > 0) return fail(MERLIN_E_INVALID, "null output");
    if (nnz > 0 && (!src || !idx || !key || !carry)) return fail(MERLIN_E_INVALID, "null argument");
    if (n_fix > 0 && !fix) return fail(MERLIN_E_INVALID, "null fix-up list");
    if ((head_fix == nullptr) != (counters == nullptr)) return fail(MERLIN_E_INVALID, "head_fix and counters go together");
    if (counters && nnz > 0 && n_fix != (nnz + item_len - 1) / item_len)
        return fail(MERLIN_E_INVALID, "in-launch fix-ups need one fix row per item");
    if (towers < 1 || towers > 2) return fail(MERLIN_E_INVALID, "towers must be 1 or 2");
    if (item_len <= 0 || sub <= 0) return fail(MERLIN_E_INVALID, "item_len and sub must be > 0");
    if (flags & ~(MERLIN_SEG_ACCUMULATE | MERLIN_SEG_NO_FILL | MERLIN_SEG_MASK_BITS | MERLIN_SEG_ROLE_MASK))
        return fail(MERLIN_E_INVALID, "unknown flags");
    HIP_TRY(merlin::launch_seg_sum(src, mask, (flags & MERLIN_SEG_MASK_BITS) ? 1 : 0, src_rows, idx, key, nnz, slot,
                                   sub, item_len, fix, n_fix, towers, out, out_rows, carry,
                                   (flags & MERLIN_SEG_ACCUMULATE) ? 1 : 0, (flags & MERLIN_SEG_NO_FILL) ? 0 : 1,
                                   (flags & MERLIN_SEG_ROLE_MASK) >> MERLIN_SEG_ROLE_SHIFT, mark, head_fix, counters,
                                   (hipStream_t)stream, mask_rows));
    return MERLIN_OK;
}

int merlin_segment_sum_fused(const float *src, const void *mask, int64_t src_rows, const int32_t *idx,
                             const int32_t *key, int64_t nnz, const int32_t *slot, int32_t sub, int64_t item_len,
                             const int32_t *fix, int64_t n_fix, int32_t towers, float *out, int64_t out_rows,
                             float *carry, int32_t flags, int32_t *mark, const int32_t *head_fix, int32_t *counters,
                             void *stream) {
    return segment_sum_fused(src, mask, src_rows, idx, key, nnz, slot, sub, item_len, fix, n_fix, towers, out,
                             out_rows, carry, flags, mark, head_fix, counters, nullptr, stream);
}

int merlin_segment_sum_mask_rows(const float *src, const void *mask, int64_t src_rows, const int32_t *idx,
                                 const int32_t *key, int64_t nnz, const int32_t *slot, int32_t sub, int64_t item_len,
                                 const int32_t *fix, int64_t n_fix, int32_t towers, float *out, int64_t out_rows,
                                 float *carry, int32_t flags, int32_t *mark, const int32_t *head_fix,
                                 int32_t *counters, const int32_t *mask_rows, void *stream) {
    if (nnz > 0 && (!mask || !mask_rows || !(flags & MERLIN_SEG_MASK_BITS)))
        return fail(MERLIN_E_INVALID, "mask_rows needs MERLIN_SEG_MASK_BITS words");
    return segment_sum_fused(src, mask, src_rows, idx, key, nnz, slot, sub, item_len, fix, n_fix, towers, out,
                             out_rows, carry, flags, mark, head_fix, counters, mask_rows, stream);
}

int merlin_segment_sum_marked(const float *src, const void *mask, int64_t src_rows, const int32_t *idx,
                              const int32_t *key, int64_t nnz, const int32_t *slot, int32_t sub, int64_t item_len,
                              const int32_t *fix, int64_t n_fix, int32_t towers, float *out, int64_t out_rows,
                              float *carry, int32_t flags, int32_t *mark, void *stream) {
    return merlin_segment_sum_fused(src, mask, src_rows, idx, key, nnz, slot, sub, item_len, fix, n_fix, towers, out,
                                    out_rows, carry, flags, mark, nullptr, nullptr, stream);
}

int merlin_segment_sum_masked(const float *src, const void *mask, int64_t src_rows, const int32_t *idx,
                              const int32_t *key, int64_t nnz, const int32_t *slot, int32_t sub, int64_t item_len,
                              const int32_t *fix, int64_t n_fix, int32_t towers, float *out, int64_t out_rows,
                              float *carry, int32_t flags, void *stream) {
    return merlin_segment_sum_marked(src, mask, src_rows, idx, key, nnz, slot, sub, item_len, fix, n_fix, towers, out,
                                     out_rows, carry, flags, nullptr, stream);
}

int merlin_segment_sum(const float *src, int64_t src_rows, const int32_t *idx, const int32_t *key, int64_t nnz,
                       const int32_t *slot, int32_t sub, int64_t item_len, const int32_t *fix, int64_t n_fix,
                       int32_t towers, float *out, int64_t out_rows, float *carry, int32_t accumulate,
                       void *stream) {
    return merlin_segment_sum_masked(src, nullptr, src_rows, idx, key, nnz, slot, sub, item_len, fix, n_fix, towers,
                                     out, out_rows, carry, accumulate ? MERLIN_SEG_ACCUMULATE : 0, stream);
}

int merlin_act_heads(const float *z, const float *b4, int64_t n, int32_t hidden, const float *w_actor,
                     const float *b_actor, const float *w_critic, const float *b_critic, int32_t act_dim,
                     int32_t deterministic, uint64_t seed, const int64_t *epoch, int64_t step, int64_t env_offset,
                     int64_t *action, float *logp, float *value, void *stream) {
    if (n < 0) return fail(MERLIN_E_INVALID, "negative size");
    if (act_dim < 1 || act_dim > 8) return fail(MERLIN_E_INVALID, "act_dim must be in [1, 8]");
    if (hidden <= 0 || hidden % 4) return fail(MERLIN_E_INVALID, "hidden must be a positive multiple of 4");
    if (n > 0 && (!z || !b4 || !w_actor || !b_actor || !w_critic || !b_critic || !action || !logp || !value))
        return fail(MERLIN_E_INVALID, "null argument");
    HIP_TRY(merlin::launch_act_heads(z, b4, n, hidden, w_actor, b_actor, w_critic, b_critic, act_dim,
                                     deterministic ? 1 : 0, seed, epoch, step, env_offset, action, logp, value,
                                     (hipStream_t)stream));
    return MERLIN_OK;
}

int64_t merlin_ppo_loss_workspace(int64_t n_samples) { return merlin::ppo_loss_workspace_doubles(n_samples); }

int merlin_ppo_loss(const float *logits, const float *value, const float *bias_actor, const float *bias_critic,
                    int64_t n_frames, int32_t act_dim, const int32_t *offs, const int32_t *order,
                    const int64_t *frame_of, int64_t n_samples, const int64_t *sample_index, const int64_t *actions,
                    const float *logp_old, const float *adv, const float *ret, double clip_eps, double vf_coef,
                    double ent_coef, float *dlogits, float *dvalue, float *dbias_actor, float *dbias_critic,
                    float *loss, double *stats, double *workspace, void *stream) {
    return merlin_ppo_loss_absmax(logits, value, bias_actor, bias_critic, n_frames, act_dim, offs, order, frame_of,
                                  n_samples, sample_index, actions, logp_old, adv, ret, clip_eps, vf_coef, ent_coef,
                                  dlogits, dvalue, dbias_actor, dbias_critic, loss, stats, workspace, nullptr, stream);
}

int merlin_ppo_loss_absmax(const float *logits, const float *value, const float *bias_actor, const float *bias_critic,
                           int64_t n_frames, int32_t act_dim, const int32_t *offs, const int32_t *order,
                           const int64_t *frame_of, int64_t n_samples, const int64_t *sample_index,
                           const int64_t *actions, const float *logp_old, const float *adv, const float *ret,
                           double clip_eps, double vf_coef, double ent_coef, float *dlogits, float *dvalue,
                           float *dbias_actor, float *dbias_critic, float *loss, double *stats, double *workspace,
                           uint32_t *grad_absmax, void *stream) {
    if (n_frames < 0 || n_samples < 0) return fail(MERLIN_E_INVALID, "negative size");
    if (n_frames > n_samples) return fail(MERLIN_E_INVALID, "every frame needs at least one sample");
    if (act_dim < 1 || act_dim > 8) return fail(MERLIN_E_INVALID, "act_dim must be in [1, 8]");
    if (!workspace) return fail(MERLIN_E_INVALID, "null workspace");
    if (n_frames > 0 && (!logits || !value || !offs || !dlogits || !dvalue))
        return fail(MERLIN_E_INVALID, "null argument");
    if (n_samples > 0 && (!order || !frame_of || !actions || !logp_old || !adv || !ret))
        return fail(MERLIN_E_INVALID, "null argument");
    if (n_samples > INT32_MAX) return fail(MERLIN_E_INVALID, "n_samples exceeds int32");
    HIP_TRY(merlin::launch_ppo_loss(logits, value, bias_actor, bias_critic, n_frames, act_dim, offs, order, frame_of,
                                    n_samples, sample_index, actions, logp_old, adv, ret, clip_eps, vf_coef, ent_coef,
                                    dlogits, dvalue, dbias_actor, dbias_critic, loss, stats, workspace,
                                    (hipStream_t)stream, grad_absmax));
    return MERLIN_OK;
}

int merlin_tower_bias_relu(float *z, const float *bias, int64_t rows, int32_t cols, int32_t towers, void *stream) {
    if ((!z || !bias) && rows > 0) return fail(MERLIN_E_INVALID, "null argument");
    if (towers < 1 || towers > 2) return fail(MERLIN_E_INVALID, "towers must be 1 or 2");
    if (cols <= 0 || cols % 4) return fail(MERLIN_E_INVALID, "cols must be a positive multiple of 4");
    HIP_TRY(merlin::launch_bias_relu(z, bias, rows, cols, towers, (hipStream_t)stream));
    return MERLIN_OK;
}

int merlin_tower_relu_bwd(const float *y, const float *dy, float *dz, int64_t rows, int32_t cols, int32_t towers,
                          float *dbias, void *stream) {
    if (!dbias || ((!y || !dy || !dz) && rows > 0)) return fail(MERLIN_E_INVALID, "null argument");
    if (towers < 1 || towers > 2) return fail(MERLIN_E_INVALID, "towers must be 1 or 2");
    if (!merlin::epilogue_cols_ok(cols)) return fail(MERLIN_E_UNSUPPORTED, "cols must be 4 x a divisor of 256");
    DeviceWs *ws = nullptr;
    int rc = device_ws(&ws);
    if (rc) return rc;
    HIP_TRY(merlin::launch_relu_bwd_colsum(y, dy, dz, rows, cols, towers, dbias, ws->epi_work, (hipStream_t)stream));
    return MERLIN_OK;
}

int merlin_tower_colsum(const float *x, int64_t rows, int32_t cols, int64_t row_stride, int64_t tower_stride,
                        int32_t towers, float *out, void *stream) {
    if (!out || (!x && rows > 0)) return fail(MERLIN_E_INVALID, "null argument");
    if (towers < 1 || towers > 2) return fail(MERLIN_E_INVALID, "towers must be 1 or 2");
    if (!merlin::epilogue_cols_ok(cols)) return fail(MERLIN_E_UNSUPPORTED, "cols must be 4 x a divisor of 256");
    if (row_stride < cols || row_stride % 4 || tower_stride % 4) return fail(MERLIN_E_INVALID, "bad strides");
    DeviceWs *ws = nullptr;
    int rc = device_ws(&ws);
    if (rc) return rc;
    HIP_TRY(merlin::launch_colsum(x, rows, cols, row_stride, tower_stride, towers, out, ws->epi_work,
                                  (hipStream_t)stream));
    return MERLIN_OK;
}

int merlin_tower_head_bwd(const float *h, const float *dlogits, const float *dvalue, const float *w_actor,
                          const float *w_critic, int64_t n, int32_t hidden, int32_t act_dim, float *dz, float *dbias,
                          float *dw_actor, float *dw_critic, uint32_t *amax, void *stream) {
    if (!dbias || !dw_actor || !dw_critic || ((!h || !dlogits || !dvalue || !w_actor || !w_critic || !dz) && n > 0))
        return fail(MERLIN_E_INVALID, "null argument");
    if (act_dim < 1 || act_dim > merlin::epilogue_max_act()) return fail(MERLIN_E_UNSUPPORTED, "act_dim must be 1..8");
    if (!merlin::epilogue_cols_ok(hidden)) return fail(MERLIN_E_UNSUPPORTED, "hidden must be 4 x a divisor of 256");
    DeviceWs *ws = nullptr;
    int rc = device_ws(&ws);
    if (rc) return rc;
    HIP_TRY(merlin::launch_head_bwd(h, dlogits, dvalue, w_actor, w_critic, n, hidden, act_dim, dz, dbias, dw_actor,
                                    dw_critic, ws->epi_work, amax, (hipStream_t)stream));
    return MERLIN_OK;
}

int merlin_tower_head_bwd_planes(const float *h, const float *dlogits, const float *dvalue, const float *w_actor,
                                 const float *w_critic, int64_t n, int32_t hidden, int32_t act_dim, void *dz_planes,
                                 float *dbias, float *dw_actor, float *dw_critic, const uint32_t *grad_absmax,
                                 uint32_t *dz_bound, void *stream) {
    if (!dbias || !dw_actor || !dw_critic || !grad_absmax || !dz_bound ||
        ((!h || !dlogits || !dvalue || !w_actor || !w_critic || !dz_planes) && n > 0))
        return fail(MERLIN_E_INVALID, "null argument");
    if (act_dim < 1 || act_dim > 8) return fail(MERLIN_E_UNSUPPORTED, "act_dim must be 1..8");
    if (!merlin::epilogue_cols_ok(hidden) || hidden % 8) return fail(MERLIN_E_UNSUPPORTED, "hidden must be 8 x a divisor of 128");
    DeviceWs *ws = nullptr;
    int rc = device_ws(&ws);
    if (rc) return rc;
    HIP_TRY(merlin::launch_head_bwd(h, dlogits, dvalue, w_actor, w_critic, n, hidden, act_dim, nullptr, dbias,
                                    dw_actor, dw_critic, ws->epi_work, dz_bound, (hipStream_t)stream, grad_absmax,
                                    dz_planes));
    return MERLIN_OK;
}

int merlin_tower_heads_fwd(const float *h, int64_t n, int32_t hidden, const float *w_actor, int32_t act_dim,
                           const float *w_critic, const float *b_actor, const float *b_critic, float *logits,
                           float *value, void *stream) {
    if ((!h || !w_actor || !w_critic || !logits || !value) && n > 0) return fail(MERLIN_E_INVALID, "null argument");
    if (n < 0) return fail(MERLIN_E_INVALID, "n must be >= 0");
    if (act_dim < 1 || act_dim > merlin::epilogue_max_act()) return fail(MERLIN_E_UNSUPPORTED, "act_dim must be 1..8");
    if (hidden != 512) return fail(MERLIN_E_UNSUPPORTED, "hidden must be 512");
    HIP_TRY(merlin::launch_heads_fwd(h, n, hidden, w_actor, act_dim, w_critic, b_actor, b_critic, logits, value,
                                     (hipStream_t)stream));
    return MERLIN_OK;
}

int merlin_x6_split(const float *x, int64_t n, void *planes, void *stream) {
    if ((!x || !planes) && n > 0) return fail(MERLIN_E_INVALID, "null argument");
    if (n < 0 || n % 8) return fail(MERLIN_E_INVALID, "n must be a non-negative multiple of 8");
    HIP_TRY(merlin::launch_x6_split(x, n, planes, (hipStream_t)stream));
    return MERLIN_OK;
}

int merlin_stage_tables_fwd(const float *W1, const float *b1, const float *W2, const float *atlas, const int16_t *idx,
                            int32_t towers, float *HT, float *T2, void *stream) {
    if (!W1 || !b1 || !W2 || !atlas || !idx || !HT || !T2) return fail(MERLIN_E_INVALID, "null argument");
    if (towers < 1 || towers > 2) return fail(MERLIN_E_INVALID, "towers must be 1 or 2");
    HIP_TRY(merlin::launch_stage_fwd(W1, b1, W2, atlas, idx, towers, HT, T2, (hipStream_t)stream));
    return MERLIN_OK;
}

int merlin_stage_tables_bwd(const float *W2, const float *HT, const float *dT2, const float *atlas,
                            const int16_t *koff, const int16_t *kv, int32_t towers, float *dH, float *dW1, float *db1,
                            float *dW2, void *stream) {
    if (!W2 || !HT || !dT2 || !atlas || !koff || !kv || !dH || !dW1 || !db1 || !dW2)
        return fail(MERLIN_E_INVALID, "null argument");
    if (towers < 1 || towers > 2) return fail(MERLIN_E_INVALID, "towers must be 1 or 2");
    DeviceWs *ws = nullptr;
    int rc = device_ws(&ws);
    if (rc != MERLIN_OK) return rc;
    HIP_TRY(merlin::launch_stage_bwd(W2, HT, dT2, atlas, koff, kv, towers, dH, dW1, db1, dW2, ws->stage_part,
                                     (hipStream_t)stream));
    return MERLIN_OK;
}

int merlin_stage_fwd_planes(const float *W1, const float *b1, const float *W2, const float *atlas, const int16_t *idx,
                            int32_t towers, float *HT, float *T2, const float *x0, const float *x1, int64_t n,
                            const uint32_t *amax, void *planes0, void *planes1, void *stream) {
    if (!W1 || !b1 || !W2 || !atlas || !idx || !HT || !T2) return fail(MERLIN_E_INVALID, "null argument");
    if (towers < 1 || towers > 2) return fail(MERLIN_E_INVALID, "towers must be 1 or 2");
    if (x0 && (!x1 || !amax || !planes0 || !planes1)) return fail(MERLIN_E_INVALID, "null plane argument");
    if (x0 && (n <= 0 || n % 8)) return fail(MERLIN_E_INVALID, "n must be a positive multiple of 8");
    HIP_TRY(merlin::launch_stage_fwd_planes(W1, b1, W2, atlas, idx, towers, HT, T2, x0, x1, n, amax, planes0, planes1,
                                            (hipStream_t)stream));
    return MERLIN_OK;
}

int merlin_stage_bwd_scatter(const float *W2, const float *HT, const float *dT2, const float *atlas,
                             const int16_t *koff, const int16_t *kv, int32_t towers, float *dH, float *DG,
                             int64_t off_w1, int64_t off_b1, int64_t off_w2, const int32_t *map, int64_t n, float *flat,
                             void *stream) {
    if (!W2 || !HT || !dT2 || !atlas || !koff || !kv || !dH || !DG || !map || !flat)
        return fail(MERLIN_E_INVALID, "null argument");
    if (towers < 1 || towers > 2) return fail(MERLIN_E_INVALID, "towers must be 1 or 2");
    const int64_t ends[3] = {off_w1 + (int64_t)towers * 32 * 192, off_b1 + (int64_t)towers * 32,
                             off_w2 + (int64_t)towers * 64 * 32 * 16};
    if (off_w1 < 0 || off_b1 < 0 || off_w2 < 0 || ends[0] > n || ends[1] > n || ends[2] > n)
        return fail(MERLIN_E_INVALID, "a gradient segment lies outside DG[:n]");
    DeviceWs *ws = nullptr;
    int rc = device_ws(&ws);
    if (rc != MERLIN_OK) return rc;
    HIP_TRY(merlin::launch_stage_bwd_scatter(W2, HT, dT2, atlas, koff, kv, towers, dH, DG, off_w1, off_b1, off_w2, map,
                                             n, flat, ws->stage_part, (hipStream_t)stream));
    return MERLIN_OK;
}

int merlin_gather_f32(const float *src, const int32_t *map, int64_t n, float *dst, void *stream) {
    if (n < 0 || (n > 0 && (!src || !map || !dst))) return fail(MERLIN_E_INVALID, "bad argument");
    HIP_TRY(merlin::launch_stage_gather(src, map, n, dst, (hipStream_t)stream));
    return MERLIN_OK;
}

int merlin_window_gemm_fwd(const float *a2w, const float *W3r, int32_t towers, int64_t nw, float *Q, void *stream) {
    if (!a2w || !W3r || !Q) return fail(MERLIN_E_INVALID, "null argument");
    if (towers < 1 || towers > 2) return fail(MERLIN_E_INVALID, "towers must be 1 or 2");
    if (nw < 0) return fail(MERLIN_E_INVALID, "nw must be >= 0");
    HIP_TRY(merlin::launch_winfwd(a2w, W3r, towers, nw, Q, (hipStream_t)stream));
    return MERLIN_OK;
}

int64_t merlin_window_gemm_bwd_work(int32_t towers, int64_t nw) {
    if (towers < 1 || towers > 2 || nw <= 0) return -1;
    return merlin::winbwd_work_floats(towers, nw);
}

int merlin_window_gemm_bwd(const float *a2w, const float *dQ, const float *W3r, int32_t towers, int64_t nw,
                           float *da2w, float *db2, float *dW3r, float *db3, float *work, int64_t work_floats,
                           void *stream) {
    if (!a2w || !dQ || !W3r || !da2w || !db2 || !dW3r || !work) return fail(MERLIN_E_INVALID, "null argument");
    if (towers < 1 || towers > 2) return fail(MERLIN_E_INVALID, "towers must be 1 or 2");
    if (nw <= 0) return fail(MERLIN_E_INVALID, "nw must be > 0");
    if (work_floats < merlin::winbwd_work_floats(towers, nw)) return fail(MERLIN_E_INVALID, "work too small");
    HIP_TRY(merlin::launch_winbwd(a2w, dQ, W3r, towers, nw, da2w, db2, dW3r, work, (hipStream_t)stream, db3));
    return MERLIN_OK;
}

int merlin_x6_join(const void *planes, int64_t n, float *x, void *stream) {
    if ((!x || !planes) && n > 0) return fail(MERLIN_E_INVALID, "null argument");
    if (n < 0 || n % 8) return fail(MERLIN_E_INVALID, "n must be a non-negative multiple of 8");
    HIP_TRY(merlin::launch_x6_join(planes, n, x, (hipStream_t)stream));
    return MERLIN_OK;
}

int merlin_x6_gemm_nt(const float *A, const void *B, int64_t M, int32_t N, int32_t K, int32_t towers, int64_t a_stride,
                      int64_t b_stride, const float *bias, float *C, int64_t c_stride, int32_t cfg, void *stream) {
    if (M < 0 || N <= 0 || K <= 0) return fail(MERLIN_E_INVALID, "bad shape");
    if (M > 0 && (!A || !B || !C)) return fail(MERLIN_E_INVALID, "null argument");
    if (K % 32) return fail(MERLIN_E_UNSUPPORTED, "K must be a multiple of 32");
    if (towers < 1 || towers > 2) return fail(MERLIN_E_INVALID, "towers must be 1 or 2");
    if (a_stride % 4 || b_stride % 8) return fail(MERLIN_E_INVALID, "tower strides: A multiple of 4, B of 8");
    const hipError_t e = merlin::launch_x6_gemm_nt(A, B, M, N, K, towers, a_stride, b_stride, bias, C, c_stride, cfg,
                                                   (hipStream_t)stream);
    if (e == hipErrorInvalidValue) return fail(MERLIN_E_UNSUPPORTED, "N not a multiple of the tile width / bad cfg");
    HIP_TRY(e);
    return MERLIN_OK;
}

int64_t merlin_x6_tn_slab_floats(int32_t M, int32_t N, int32_t towers, int32_t splits) {
    return (int64_t)std::max(1, splits) * towers * M * N;
}

int merlin_x6_gemm_tn(const float *A, const float *B, int64_t Kd, int32_t M, int32_t N, int32_t towers, int64_t a_stride,
                      int64_t b_stride, int32_t splits, float *slab, float *out, int32_t cfg, void *stream) {
    if (Kd < 0 || M <= 0 || N <= 0) return fail(MERLIN_E_INVALID, "bad shape");
    if (!out || (Kd > 0 && (!A || !B || !slab))) return fail(MERLIN_E_INVALID, "null argument");
    if (towers < 1 || towers > 2) return fail(MERLIN_E_INVALID, "towers must be 1 or 2");
    if (splits < 1 || splits > merlin::x6_tn_max_splits()) return fail(MERLIN_E_INVALID, "splits out of range");
    if (M % 8 || N % 8 || a_stride % 4 || b_stride % 4) return fail(MERLIN_E_INVALID, "M, N: multiples of 8");
    const hipError_t e = merlin::launch_x6_gemm_tn(A, B, Kd, M, N, towers, a_stride, b_stride, splits, slab, out, cfg,
                                                   (hipStream_t)stream);
    if (e == hipErrorInvalidValue) return fail(MERLIN_E_UNSUPPORTED, "M / N not multiples of the tile / bad cfg");
    HIP_TRY(e);
    return MERLIN_OK;
}

int merlin_h3_amax(const float *x, int64_t n, int32_t towers, int64_t stride, uint32_t *amax, void *stream) {
    if (!amax || (n > 0 && !x)) return fail(MERLIN_E_INVALID, "null argument");
    // n == 0: zero amax[0 .. towers) only (any count up to 2^20: a rollout's per-step scales at once)
    if (towers < 1 || (n > 0 && towers > 2) || towers > (1 << 20))
        return fail(MERLIN_E_INVALID, "towers must be 1 or 2");
    if (n < 0 || n % 4 || stride % 4 || (towers > 1 && stride < n)) return fail(MERLIN_E_INVALID, "n, stride: multiples of 4");
    HIP_TRY(merlin::launch_h3_amax(x, n, towers, stride, amax, (hipStream_t)stream));
    return MERLIN_OK;
}

int merlin_h3_split(const float *x, int64_t n, int32_t towers, const uint32_t *amax, void *planes, void *stream) {
    if ((!x || !planes || !amax) && n > 0) return fail(MERLIN_E_INVALID, "null argument");
    if (towers < 1 || towers > 2) return fail(MERLIN_E_INVALID, "towers must be 1 or 2");
    if (n < 0 || n % 8) return fail(MERLIN_E_INVALID, "n must be a non-negative multiple of 8");
    HIP_TRY(merlin::launch_h3_split(x, n, towers, amax, planes, (hipStream_t)stream));
    return MERLIN_OK;
}

static int h3_gemm_nt(const float *A, const uint32_t *amax_a, const void *B, const uint32_t *amax_b, int64_t M,
                      int32_t N, int32_t K, int32_t towers, int64_t a_stride, int64_t b_stride, const float *bias,
                      float *C, int64_t c_stride, void *a_planes, const int32_t *a_rows, int32_t cfg, void *stream,
                      const float *head_w0 = nullptr, int32_t n_actions = 0, const float *head_w1 = nullptr,
                      float *head_part = nullptr, bool a_is_planes = false) {
    if (M < 0 || N <= 0 || K <= 0) return fail(MERLIN_E_INVALID, "bad shape");
    if (M > 0 && (!A || !B || (!C && !head_part) || !amax_a || !amax_b)) return fail(MERLIN_E_INVALID, "null argument");
    if (K % 32) return fail(MERLIN_E_UNSUPPORTED, "K must be a multiple of 32");
    if (towers < 1 || towers > 2) return fail(MERLIN_E_INVALID, "towers must be 1 or 2");
    if (a_stride % 4 || b_stride % 8) return fail(MERLIN_E_INVALID, "tower strides: A multiple of 4, B of 8");
    const hipError_t e = merlin::launch_h3_gemm_nt(A, amax_a, B, amax_b, M, N, K, towers, a_stride, b_stride, bias, C,
                                                   c_stride, a_planes, cfg, (hipStream_t)stream, a_rows, head_w0,
                                                   n_actions, head_w1, head_part, a_is_planes);
    if (e == hipErrorInvalidValue)
        return fail(MERLIN_E_UNSUPPORTED, "N not a multiple of the tile width / bad cfg / unsupported gather");
    HIP_TRY(e);
    return MERLIN_OK;
}

int merlin_h3_gemm_nt(const float *A, const uint32_t *amax_a, const void *B, const uint32_t *amax_b, int64_t M,
                      int32_t N, int32_t K, int32_t towers, int64_t a_stride, int64_t b_stride, const float *bias,
                      float *C, int64_t c_stride, void *a_planes, int32_t cfg, void *stream) {
    return h3_gemm_nt(A, amax_a, B, amax_b, M, N, K, towers, a_stride, b_stride, bias, C, c_stride, a_planes, nullptr,
                      cfg, stream);
}

int merlin_h3_gemm_nt_planes(const void *A_planes, const uint32_t *amax_a, const void *B, const uint32_t *amax_b,
                             int64_t M, int32_t N, int32_t K, int32_t towers, int64_t a_stride, int64_t b_stride,
                             const float *bias, float *C, int64_t c_stride, int32_t cfg, void *stream) {
    if (cfg < 60 || (cfg >= 70 && cfg != 77 && cfg != 78))
        return fail(MERLIN_E_UNSUPPORTED, "plane-operand cfgs are 60..69, 77 and 78");
    return h3_gemm_nt(static_cast<const float *>(A_planes), amax_a, B, amax_b, M, N, K, towers, a_stride, b_stride,
                      bias, C, c_stride, nullptr, nullptr, cfg, stream);
}

int merlin_h3_gemm_nt_gather(const float *A, const uint32_t *amax_a, const void *B, const uint32_t *amax_b, int64_t M,
                             int32_t N, int32_t K, int32_t towers, int64_t a_stride, int64_t b_stride,
                             const float *bias, float *C, int64_t c_stride, const int32_t *a_rows, int32_t cfg,
                             void *stream) {
    if (M > 0 && !a_rows) return fail(MERLIN_E_INVALID, "null argument");
    if (K % 64) return fail(MERLIN_E_UNSUPPORTED, "gathered rows: K must be a multiple of 64");
    return h3_gemm_nt(A, amax_a, B, amax_b, M, N, K, towers, a_stride, b_stride, bias, C, c_stride, nullptr, a_rows,
                      cfg, stream);
}

static int h3_gemm_tn(const void *A, const uint32_t *amax_a, const void *B, const uint32_t *amax_b, int64_t Kd,
                      int32_t M, int32_t N, int32_t towers, int64_t a_stride, int64_t b_stride, int32_t splits,
                      float *slab, float *out, bool planes, int32_t cfg, void *stream, const int32_t *b_rows = nullptr,
                      bool a_planes = false, bool b_planes = false) {
    if (Kd < 0 || M <= 0 || N <= 0) return fail(MERLIN_E_INVALID, "bad shape");
    if (!out || (Kd > 0 && (!A || !B || !slab || !amax_a || !amax_b))) return fail(MERLIN_E_INVALID, "null argument");
    if (towers < 1 || towers > 2) return fail(MERLIN_E_INVALID, "towers must be 1 or 2");
    if (splits < 1 || splits > merlin::x6_tn_max_splits()) return fail(MERLIN_E_INVALID, "splits out of range");
    if (M % 8 || N % 8 || a_stride % 4 || b_stride % 4) return fail(MERLIN_E_INVALID, "M, N: multiples of 8");
    const hipError_t e = merlin::launch_h3_gemm_tn(A, amax_a, B, amax_b, Kd, M, N, towers, a_stride, b_stride, splits,
                                                   slab, out, planes, cfg, (hipStream_t)stream, b_rows, a_planes,
                                                   b_planes);
    if (e == hipErrorInvalidValue) return fail(MERLIN_E_UNSUPPORTED, "M / N not multiples of the tile / bad cfg");
    HIP_TRY(e);
    return MERLIN_OK;
}

int merlin_h3_gemm_tn(const float *A, const uint32_t *amax_a, const float *B, const uint32_t *amax_b, int64_t Kd,
                      int32_t M, int32_t N, int32_t towers, int64_t a_stride, int64_t b_stride, int32_t splits,
                      float *slab, float *out, int32_t cfg, void *stream) {
    return h3_gemm_tn(A, amax_a, B, amax_b, Kd, M, N, towers, a_stride, b_stride, splits, slab, out, false, cfg,
                      stream);
}

int merlin_h3_gemm_nt_heads(const float *A, const uint32_t *amax_a, const void *B, const uint32_t *amax_b, int64_t M,
                            int32_t N, int32_t K, int64_t a_stride, int64_t b_stride, const float *bias, float *C,
                            int64_t c_stride, const int32_t *a_rows, const float *head_w0, int32_t n_actions,
                            const float *head_w1, float *head_partials, int32_t cfg, void *stream) {
    if (M > 0 && (!bias || !head_w0 || !head_w1 || !head_partials)) return fail(MERLIN_E_INVALID, "null argument");
    if (n_actions < 1 || n_actions > 4) return fail(MERLIN_E_UNSUPPORTED, "heads epilogue: 1..4 actions");
    if (merlin::h3_heads_parts(N, cfg) == 0) return fail(MERLIN_E_UNSUPPORTED, "heads epilogue: cfg 10, 12 or 13");
    if (a_rows && K % 64) return fail(MERLIN_E_UNSUPPORTED, "gathered rows: K must be a multiple of 64");
    return h3_gemm_nt(A, amax_a, B, amax_b, M, N, K, 2, a_stride, b_stride, bias, C, c_stride, nullptr, a_rows, cfg,
                      stream, head_w0, n_actions, head_w1, head_partials);
}

int32_t merlin_h3_heads_parts(int32_t N, int32_t cfg) { return merlin::h3_heads_parts(N, cfg); }

int merlin_h3_walk_blocks(int32_t blocks) {
    if (blocks < 0) return fail(MERLIN_E_INVALID, "blocks must be 0 (one per CU) or positive");
    merlin::set_h3p_walk_blocks(blocks);
    return MERLIN_OK;
}

int merlin_act_draw(const float *partials, int32_t parts, int64_t n, const float *b_actor, const float *b_critic,
                    int32_t n_actions, int32_t deterministic, uint64_t seed, const int64_t *epoch, int64_t step,
                    int64_t env_offset, int64_t *action, float *logp, float *value, void *stream) {
    if (n < 0 || parts < 1 || n_actions < 1 || n_actions > 4) return fail(MERLIN_E_INVALID, "bad shape");
    if (n > 0 && (!partials || !b_actor || !b_critic || !action || !logp || !value))
        return fail(MERLIN_E_INVALID, "null argument");
    HIP_TRY(merlin::launch_act_draw(partials, parts, n, b_actor, b_critic, n_actions, deterministic, seed, epoch, step,
                                    env_offset, action, logp, value, (hipStream_t)stream));
    return MERLIN_OK;
}

int merlin_heads_combine(const float *partials, int32_t parts, int64_t M, int32_t n_actions, float *logits,
                         float *value, void *stream) {
    if (M < 0 || parts < 1 || n_actions < 1 || n_actions > 4) return fail(MERLIN_E_INVALID, "bad shape");
    if (M > 0 && (!partials || !logits || !value)) return fail(MERLIN_E_INVALID, "null argument");
    HIP_TRY(merlin::launch_heads_combine(partials, parts, M, n_actions, logits, value, (hipStream_t)stream));
    return MERLIN_OK;
}

int merlin_h3_gemm_tn_gather(const float *A, const uint32_t *amax_a, const float *B, const uint32_t *amax_b, int64_t Kd,
                             int32_t M, int32_t N, int32_t towers, int64_t a_stride, int64_t b_stride, int32_t splits,
                             float *slab, float *out, const int32_t *b_rows, int32_t cfg, void *stream) {
    if (Kd > 0 && !b_rows) return fail(MERLIN_E_INVALID, "null argument");
    if (N % 64) return fail(MERLIN_E_UNSUPPORTED, "gathered rows: N must be a multiple of 64");
    return h3_gemm_tn(A, amax_a, B, amax_b, Kd, M, N, towers, a_stride, b_stride, splits, slab, out, false, cfg, stream,
                      b_rows);
}

int merlin_h3_gemm_nt_heads_planes(const void *A_planes, const uint32_t *amax_a, const void *B,
                                   const uint32_t *amax_b, int64_t M, int32_t N, int32_t K, int64_t a_stride,
                                   int64_t b_stride, const float *bias, float *C, int64_t c_stride,
                                   const int32_t *a_rows, const float *head_w0, int32_t n_actions,
                                   const float *head_w1, float *head_partials, int32_t cfg, void *stream) {
    if (M > 0 && (!bias || !C || !a_rows || (head_partials && (!head_w0 || !head_w1))))
        return fail(MERLIN_E_INVALID, "null argument");
    if (head_partials && (n_actions < 1 || n_actions > 4))
        return fail(MERLIN_E_UNSUPPORTED, "heads epilogue: 1..4 actions");
    if (merlin::h3_heads_parts(N, cfg) == 0) return fail(MERLIN_E_UNSUPPORTED, "planes forward: cfg 10, 12 or 13");
    if (K % 64) return fail(MERLIN_E_UNSUPPORTED, "gathered rows: K must be a multiple of 64");
    return h3_gemm_nt(static_cast<const float *>(A_planes), amax_a, B, amax_b, M, N, K, 2, a_stride, b_stride, bias,
                      C, c_stride, nullptr, a_rows, cfg, stream, head_w0, n_actions, head_w1, head_partials, true);
}

int merlin_h3_gemm_tn_gather_planes(const void *A_planes, const uint32_t *amax_a, const void *B_planes,
                                    const uint32_t *amax_b, int64_t Kd, int32_t M, int32_t N, int32_t towers,
                                    int64_t a_stride, int64_t b_stride, int32_t splits, float *slab, float *out,
                                    const int32_t *b_rows, int32_t cfg, void *stream) {
    if (Kd > 0 && !b_rows) return fail(MERLIN_E_INVALID, "null argument");
    if (N % 64) return fail(MERLIN_E_UNSUPPORTED, "gathered rows: N must be a multiple of 64");
    return h3_gemm_tn(A_planes, amax_a, B_planes, amax_b, Kd, M, N, towers, a_stride, b_stride, splits, slab, out,
                      false, cfg, stream, b_rows, true, true);
}

int merlin_h3_gemm_tn_gather_planes_a(const void *A_planes, const uint32_t *amax_a, const float *B,
                                      const uint32_t *amax_b, int64_t Kd, int32_t M, int32_t N, int32_t towers,
                                      int64_t a_stride, int64_t b_stride, int32_t splits, float *slab, float *out,
                                      const int32_t *b_rows, int32_t cfg, void *stream) {
    if (Kd > 0 && !b_rows) return fail(MERLIN_E_INVALID, "null argument");
    if (N % 64) return fail(MERLIN_E_UNSUPPORTED, "gathered rows: N must be a multiple of 64");
    return h3_gemm_tn(A_planes, amax_a, B, amax_b, Kd, M, N, towers, a_stride, b_stride, splits, slab, out, false, cfg,
                      stream, b_rows, true);
}

int merlin_h3_gemm_tn_planes(const void *A, const uint32_t *amax_a, const void *B, const uint32_t *amax_b, int64_t Kd,
                             int32_t M, int32_t N, int32_t towers, int64_t a_stride, int64_t b_stride, int32_t splits,
                             float *slab, float *out, int32_t cfg, void *stream) {
    return h3_gemm_tn(A, amax_a, B, amax_b, Kd, M, N, towers, a_stride, b_stride, splits, slab, out, true, cfg,
                      stream);
}

int64_t merlin_clip_adam_workspace(int32_t n_tensors, const int64_t *numel) {
    if (n_tensors < 0 || n_tensors > merlin::OPT_MAX_TENSORS || (n_tensors > 0 && !numel)) return -1;
    return std::max<int64_t>(1, merlin::opt_blocks(n_tensors, numel));
}

int merlin_clip_adam(int32_t n_tensors, float *const *params, float *const *grads, float *const *exp_avg,
                     float *const *exp_avg_sq, float *const *steps, const int64_t *numel, double lr, double beta1,
                     double beta2, double eps, float max_norm, float *norm_out, double *workspace, void *stream) {
    if (n_tensors < 1 || n_tensors > merlin::OPT_MAX_TENSORS)
        return fail(MERLIN_E_INVALID, "n_tensors must be in [1, 32]");
    if (!params || !grads || !exp_avg || !exp_avg_sq || !steps || !numel || !workspace)
        return fail(MERLIN_E_INVALID, "null argument");
    int64_t blocks = 0;
    for (int i = 0; i < n_tensors; i++) {
        if (numel[i] <= 0) return fail(MERLIN_E_INVALID, "every tensor needs numel > 0");
        if (!params[i] || !grads[i] || !exp_avg[i] || !exp_avg_sq[i] || !steps[i])
            return fail(MERLIN_E_INVALID, "null tensor pointer");
    }
    blocks = merlin::opt_blocks(n_tensors, numel);
    if (blocks > INT32_MAX / 2) return fail(MERLIN_E_INVALID, "too many elements");
    HIP_TRY(merlin::launch_clip_adam(n_tensors, params, grads, exp_avg, exp_avg_sq, steps, numel, lr, beta1, beta2, eps,
                                     max_norm, norm_out, workspace, (hipStream_t)stream));
    return MERLIN_OK;
}

int merlin_clip_adam_chain(int32_t n_tensors, float *const *params, float *const *grads, float *const *exp_avg,
                           float *const *exp_avg_sq, float *const *steps, const int64_t *numel, double lr, double beta1,
                           double beta2, double eps, float max_norm, float *norm_out, double *workspace,
                           uint32_t *zero0, int32_t n_zero0, uint32_t *zero1, int32_t n_zero1, const float *flat,
                           int64_t n_flat, const int32_t *slots, float *D, uint32_t *amax, const int32_t *amax_slot,
                           double *total, void *stream) {
    if (n_tensors < 1 || n_tensors > merlin::OPT_MAX_TENSORS)
        return fail(MERLIN_E_INVALID, "n_tensors must be in [1, 32]");
    if (!params || !grads || !exp_avg || !exp_avg_sq || !steps || !numel || !workspace || !flat || !slots || !D)
        return fail(MERLIN_E_INVALID, "null argument");
    if (n_zero0 < 0 || n_zero1 < 0 || (n_zero0 > 0 && !zero0) || (n_zero1 > 0 && !zero1))
        return fail(MERLIN_E_INVALID, "bad zero list");
    if (amax_slot && !amax) return fail(MERLIN_E_INVALID, "amax_slot without amax_dev");
    merlin::OptChain ch{};
    for (int i = 0; i < n_tensors; i++) {
        if (numel[i] <= 0) return fail(MERLIN_E_INVALID, "every tensor needs numel > 0");
        if (!params[i] || !grads[i] || !exp_avg[i] || !exp_avg_sq[i] || !steps[i])
            return fail(MERLIN_E_INVALID, "null tensor pointer");
        if (params[i] < flat || params[i] + numel[i] > flat + n_flat)
            return fail(MERLIN_E_INVALID, "a parameter lies outside the flat buffer");
        ch.amax_slot[i] = amax_slot ? amax_slot[i] : -1;
        if (ch.amax_slot[i] < -1 || ch.amax_slot[i] > 1) return fail(MERLIN_E_INVALID, "amax_slot must be -1, 0 or 1");
    }
    const int64_t blocks = merlin::opt_blocks(n_tensors, numel);
    if (blocks > INT32_MAX / 2) return fail(MERLIN_E_INVALID, "too many elements");
    ch.zero[0] = zero0, ch.zero[1] = zero1, ch.n_zero[0] = n_zero0, ch.n_zero[1] = n_zero1;
    ch.flat = flat, ch.slots = reinterpret_cast<const int2 *>(slots), ch.D = D, ch.amax = amax, ch.total = total;
    HIP_TRY(merlin::launch_clip_adam(n_tensors, params, grads, exp_avg, exp_avg_sq, steps, numel, lr, beta1, beta2, eps,
                                     max_norm, norm_out, workspace, (hipStream_t)stream, &ch));
    return MERLIN_OK;
}

int64_t merlin_group_clip_sgd_workspace(int32_t n_tensors, const int64_t *numel, int32_t G) {
    if (n_tensors < 0 || n_tensors > merlin::OPT_MAX_TENSORS || G < 0 || (n_tensors > 0 && !numel)) return -1;
    for (int i = 0; i < n_tensors; i++)
        if (numel[i] <= 0) return -1;
    return std::max<int64_t>(1, merlin::group_blocks(n_tensors, numel) * (int64_t)G);
}

int merlin_group_clip_sgd(int32_t n_tensors, float *const *params, float *const *grads, const int64_t *numel,
                          int32_t G, float lr, float max_norm, float *norm_out, double *workspace, void *stream) {
    if (n_tensors < 0 || n_tensors > merlin::OPT_MAX_TENSORS)
        return fail(MERLIN_E_INVALID, "n_tensors must be in [0, 32]");
    if (G < 0 || G > 65535) return fail(MERLIN_E_INVALID, "G must be in [0, 65535]");
    if (n_tensors == 0 || G == 0) return MERLIN_OK;
    if (!params || !grads || !numel || !workspace) return fail(MERLIN_E_INVALID, "null argument");
    for (int i = 0; i < n_tensors; i++) {
        if (numel[i] <= 0) return fail(MERLIN_E_INVALID, "every tensor needs numel > 0");
        if (!params[i] || !grads[i]) return fail(MERLIN_E_INVALID, "null tensor pointer");
    }
    if (merlin::group_blocks(n_tensors, numel) > INT32_MAX / 2) return fail(MERLIN_E_INVALID, "too many elements");
    HIP_TRY(merlin::launch_group_clip_sgd(n_tensors, params, grads, numel, G, lr, max_norm, norm_out, workspace,
                                          (hipStream_t)stream));
    return MERLIN_OK;
}

int merlin_episode_loss(const float *reward, const float *value, const float *new_logp, const float *new_value,
                        const int32_t *length, int32_t T, int32_t n, double gamma, double lam, float *workspace,
                        float *loss, void *stream) {
    if (T < 1 || n < 0) return fail(MERLIN_E_INVALID, "episode_loss needs T >= 1 and n >= 0");
    if (n == 0) return MERLIN_OK;
    if (!reward || !value || !new_logp || !new_value || !length || !workspace || !loss)
        return fail(MERLIN_E_INVALID, "null argument");
    HIP_TRY(merlin::launch_episode_loss(reward, value, new_logp, new_value, length, T, n, gamma, lam, workspace, loss,
                                        (hipStream_t)stream));
    return MERLIN_OK;
}

int merlin_episode_class_stats(const float *done, const double *ep_return, const int32_t *ep_length,
                               const uint8_t *cls, int32_t T, int32_t N, int32_t n_classes, double *out,
                               int32_t accumulate, void *stream) {
    if (T < 0 || N < 0) return fail(MERLIN_E_INVALID, "episode_class_stats needs T >= 0 and N >= 0");
    if (n_classes < 1 || n_classes > merlin::EPS_MAX_CLASSES)
        return fail(MERLIN_E_INVALID, "episode_class_stats needs n_classes in [1, 8]");
    if (!out) return fail(MERLIN_E_INVALID, "null argument");
    if (T > 0 && N > 0 && (!done || !ep_return || !ep_length || !cls)) return fail(MERLIN_E_INVALID, "null argument");
    DeviceWs *ws = nullptr;
    int rc = device_ws(&ws);
    if (rc) return rc;
    HIP_TRY(merlin::launch_episode_class_stats(done, ep_return, ep_length, cls, T, N, n_classes, out, accumulate,
                                               ws->eps_part, (hipStream_t)stream));
    return MERLIN_OK;
}

}  // extern "C"
