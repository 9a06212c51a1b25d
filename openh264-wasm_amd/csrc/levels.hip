// levels.hip -- histograms, level tables (LUTs) and automatic levels of tight I420 frames on the device (gfx950), as
// include/h264mi.h defines them (h264mi_i420_hist_dev, h264mi_i420_lut_dev, h264mi_i420_levels_dev). DESIGN.md §5.19.
//   hist_kernel          : n frames and their three planes per launch -- the standalone call, the first step of AUTO
//   levels_decide_kernel : one wave per frame: the measured ends, the state, the gain limit, the 768 table bytes, the record
//   lut_kernel           : n frames and their three planes per launch, O = T[plane][C] -- the standalone call, the last
//                          step of the levels call, an encoder's stage in place on the input area
// The rules (the header has them in full): H[plane][v] counts the samples; AUTO measures lo_m and hi_m from the luma
// histogram under the clip shares, smooths them in 1/256 levels with a floor shift, widens the span to the gain limit
// and maps lo_e..hi_e linearly to out_lo..out_hi, rounded once; chroma is a gain about 128. picture_host.h holds the
// follow, limit and table-entry functions for host and device.
//
// Work split of the two streaming kernels. A plane of a tight frame is one run of bytes, so neither kernel knows rows.
// The run is laid on the grid of 16-byte units of the address space: LV_CHUNK = 16384 bytes of that grid (256 threads x
// LV_ITER = 4 units of LV_UNIT = 16 bytes) are one item, and the items (frame, plane, chunk) are dealt to at most
// PIC_MAX_BLOCKS blocks in runs of consecutive items; the loop count and every branch around a barrier depend on the
// block only. A unit that lies inside the plane moves as one 16-byte word, whatever the plane's address and length; the
// at most two units a plane only partly covers -- its first bytes up to a multiple of 16 and its last ones, or all of a
// plane of 1 or 9 bytes -- move as bytes under a range test. An aligned unit inside the run never leaves it, the byte
// path tests every byte: no access leaves a plane. A frame's chunk count is taken for the worst address (15 bytes past
// a multiple of 16), so it is the same for every frame of a launch; a chunk past the run's end does nothing.
//
// Histogram. A wave owns a sub-histogram of 256 32-bit counters in LDS (a block four: 4 KB) and adds to it with LDS
// atomics. A sub-histogram receives at most one plane's samples, 2^26: the counters cannot wrap. When the block moves on
// to another plane or frame, and at the end, thread t sums bin t of the four and adds a non-zero sum to d_hist with one
// global integer add: whatever the order, the same words. The hazard is content: on a flat plane all 64 lanes add to one
// address and the LDS serialises them. So a dword that is the same in every lane of the wave -- one readfirstlane, one
// compare, a wave-uniform branch -- is counted by lanes 0..3 adding 64 to the bins of its four bytes. DESIGN.md §5.19
// has what that bought.
// LUT. A block holds the frame's 768 table bytes in LDS, loaded when its run of items enters a frame (once a launch
// with a shared table set). A lane looks its 16 samples up by byte reads of LDS and stores one 16-byte word. In place
// is safe lane by lane: a lane reads a unit (or a byte) before it writes exactly that unit (or byte), and no other lane
// touches it. Out of place the grid is the destination's; a source that sits differently on it is read as bytes.
// Decide. Lane l holds bins 4l..4l+3 of the luma histogram. The sums below and above a bin come from one inclusive scan
// over the lanes' totals (the sum from above is npix minus the sum below); the ends are a wave minimum and maximum of
// the lanes' first and last bins past the thresholds, which the host computed (the rule's only 64-bit arithmetic). Every
// lane then holds the same ends and writes the twelve table bytes of its bins as three dwords; lane 0 writes the state
// and the record. Everything is an ordinary vector store.
//
// A translation unit and a code object of its own, as denoise.hip is: the library's other kernels stay byte for byte
// what they were. The host runtime (enc_input.inc, capi_enc.inc) reaches it through the functions picture_host.h declares.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/h264mi.h"
#include "picture_host.h"
#include "picture_dev.h"

namespace h264mi {
#define LV_UNIT 16                       // bytes a lane moves at once
#define LV_ITER 4                        // units a thread takes of an item
#define LV_CHUNK (256 * LV_UNIT * LV_ITER)  // bytes of the unit grid an item covers

// the items of a launch over n frames
struct LevelsGrid {
    size_t fb;             // frame f: base + f * fb
    size_t off[3];         // a frame's planes
    uint32_t len[3];       // their bytes, at most 2^26
    int nch[3];            // chunks of a plane, the same for every address
    int per_frame;         // nch[0] + nch[1] + nch[2]
    long long items, per;  // n * per_frame; items a block
};
struct HistLaunch { const uint8_t *frames; uint32_t *hist; LevelsGrid g; };
struct LutLaunch {
    const uint8_t *src;
    uint8_t *dst;
    const uint8_t *luts;
    size_t lut_stride;  // 768, or 0: one set for every frame
    LevelsGrid g;
};

// item `it`: its frame, plane and chunk
PICDEV void levels_item(const LevelsGrid &g, long long it, long long &f, int &pl, int &k) {
    f = it / g.per_frame;
    k = (int)(it - f * g.per_frame);
    pl = 0;
    if (k >= g.nch[0]) {
        k -= g.nch[0]; pl = 1;
        if (k >= g.nch[1]) { k -= g.nch[1]; pl = 2; }
    }
}

// a dword of a unit into the wave's sub-histogram. Every lane of the wave runs it; in: the lane's dword is inside the plane
PICDEV void hist_dword(uint32_t *h, uint32_t d, bool in, int lane) {
    const uint32_t u = (uint32_t)__builtin_amdgcn_readfirstlane((int)d);
    if (__all(in && d == u)) {  // the same in every lane: 64 of each byte
        if (lane < 4) atomicAdd(&h[(u >> (8 * lane)) & 255u], 64u);
    } else if (in) {
        atomicAdd(&h[d & 255u], 1u); atomicAdd(&h[(d >> 8) & 255u], 1u);
        atomicAdd(&h[(d >> 16) & 255u], 1u); atomicAdd(&h[d >> 24], 1u);
    }
}

// the block's four sub-histograms summed into the 256 words at out, and zeroed for the next plane
PICDEV void hist_flush(uint32_t (*sh)[256], uint32_t *out, int t) {
    __syncthreads();
    const uint32_t c = sh[0][t] + sh[1][t] + sh[2][t] + sh[3][t];
    sh[0][t] = sh[1][t] = sh[2][t] = sh[3][t] = 0;
    if (c) atomicAdd(out + t, c);
    __syncthreads();
}

__global__ __launch_bounds__(256) void hist_kernel(HistLaunch a) {
    __shared__ uint32_t sh[4][256];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    sh[0][t] = sh[1][t] = sh[2][t] = sh[3][t] = 0;
    __syncthreads();
    const long long it0 = (long long)blockIdx.x * a.g.per, it1 = min(it0 + a.g.per, a.g.items);
    long long key = -1;  // 3 f + plane of what the sub-histograms hold
    for (long long it = it0; it < it1; it++) {  // the same count, frame and plane in every thread of a block
        long long f; int pl, k;
        levels_item(a.g, it, f, pl, k);
        if (3 * f + pl != key) {
            if (key >= 0) hist_flush(sh, a.hist + 256 * key, t);
            key = 3 * f + pl;
        }
        const uint8_t *P = a.frames + (size_t)f * a.g.fb + a.g.off[pl];
        const uint32_t lo = (uint32_t)((uintptr_t)P & (LV_UNIT - 1)), hi = lo + a.g.len[pl];  // the plane on the unit grid
        const uint8_t *A = P - lo;
        uint4 v[LV_ITER];
        bool full[LV_ITER];
#pragma unroll
        for (int i = 0; i < LV_ITER; i++) {
            const uint32_t o = (uint32_t)k * LV_CHUNK + (uint32_t)(i * 256 + t) * LV_UNIT;
            full[i] = o >= lo && o + LV_UNIT <= hi;
            v[i] = full[i] ? *(const uint4 *)(A + o) : make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < LV_ITER; i++) {
            hist_dword(sh[wv], v[i].x, full[i], lane); hist_dword(sh[wv], v[i].y, full[i], lane);
            hist_dword(sh[wv], v[i].z, full[i], lane); hist_dword(sh[wv], v[i].w, full[i], lane);
            const uint32_t o = (uint32_t)k * LV_CHUNK + (uint32_t)(i * 256 + t) * LV_UNIT;
            if (!full[i] && o < hi && o + LV_UNIT > lo)  // a unit the plane partly covers
                for (uint32_t j = max(o, lo); j < min(o + LV_UNIT, hi); j++) atomicAdd(&sh[wv][A[j]], 1u);
        }
    }
    if (key >= 0) hist_flush(sh, a.hist + 256 * key, t);
}

PICDEV uint32_t lut_dword(const uint8_t *T, uint32_t d) {
    return (uint32_t)T[d & 255u] | (uint32_t)T[(d >> 8) & 255u] << 8 | (uint32_t)T[(d >> 16) & 255u] << 16 | (uint32_t)T[d >> 24] << 24;
}

__global__ __launch_bounds__(256) void lut_kernel(LutLaunch a) {
    __shared__ __attribute__((aligned(16))) uint8_t tab[768];
    const int t = threadIdx.x;
    const long long it0 = (long long)blockIdx.x * a.g.per, it1 = min(it0 + a.g.per, a.g.items);
    long long tf = -1;  // the frame whose tables are in tab
    for (long long it = it0; it < it1; it++) {  // the same count and frame in every thread of a block
        long long f; int pl, k;
        levels_item(a.g, it, f, pl, k);
        if (tf < 0 || (a.lut_stride && f != tf)) {
            if (tf >= 0) __syncthreads();  // the reads of the last frame's tables
            const uint8_t *L = a.luts + (size_t)f * a.lut_stride;
            tab[t] = L[t]; tab[256 + t] = L[256 + t]; tab[512 + t] = L[512 + t];
            __syncthreads();
            tf = f;
        }
        const uint8_t *T = tab + 256 * pl;
        const size_t po = (size_t)f * a.g.fb + a.g.off[pl];
        uint8_t *D = a.dst + po;
        const uint32_t lo = (uint32_t)((uintptr_t)D & (LV_UNIT - 1)), hi = lo + a.g.len[pl];  // the plane on the destination's unit grid
        uint8_t *A = D - lo;
        const uint8_t *SA = a.src + po - lo;
        const bool same = ((uintptr_t)SA & (LV_UNIT - 1)) == 0;  // the source sits on the same grid
        uint4 v[LV_ITER];
        bool full[LV_ITER];
#pragma unroll
        for (int i = 0; i < LV_ITER; i++) {
            const uint32_t o = (uint32_t)k * LV_CHUNK + (uint32_t)(i * 256 + t) * LV_UNIT;
            full[i] = o >= lo && o + LV_UNIT <= hi;
            v[i] = make_uint4(0, 0, 0, 0);
            if (full[i]) {
                if (same) {
                    v[i] = *(const uint4 *)(SA + o);
                } else {
                    uint32_t d[4] = {0, 0, 0, 0};
#pragma unroll
                    for (int j = 0; j < LV_UNIT; j++) d[j >> 2] |= (uint32_t)SA[o + j] << (8 * (j & 3));
                    v[i] = make_uint4(d[0], d[1], d[2], d[3]);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < LV_ITER; i++) {
            const uint32_t o = (uint32_t)k * LV_CHUNK + (uint32_t)(i * 256 + t) * LV_UNIT;
            if (full[i]) {
                *(uint4 *)(A + o) = make_uint4(lut_dword(T, v[i].x), lut_dword(T, v[i].y), lut_dword(T, v[i].z), lut_dword(T, v[i].w));
            } else if (o < hi && o + LV_UNIT > lo) {  // a unit the plane partly covers
                for (uint32_t j = max(o, lo); j < min(o + LV_UNIT, hi); j++) A[j] = T[SA[j]];
            }
        }
    }
}

// ---- the decision
struct DecideLaunch {
    uint8_t *luts;         // n table sets, at a multiple of 4
    const uint32_t *hist;  // n * 768 words; null in FIXED mode
    int32_t *state;        // n * 4 words, or null
    int32_t *record;       // n * 8 words, or null
    uint32_t npix, k_lo, k_hi;
    h264mi_levels p;
};

PICDEV int wave_min_i(int v) {
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
    return v;
}
PICDEV int wave_max_i(int v) {
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}

__global__ __launch_bounds__(64) void levels_decide_kernel(DecideLaunch a) {
    const size_t f = blockIdx.x;
    const int lane = threadIdx.x;
    const h264mi_levels &p = a.p;
    int lo_m = 0, hi_m = 0, lo_s = 0, hi_s = 0, lo_e, hi_e;
    uint32_t below = 0, above = 0;
    if (p.mode == H264MI_LEVELS_AUTO) {
        const uint32_t *H = a.hist + 768 * f + 4 * lane;
        const uint32_t hb[4] = {H[0], H[1], H[2], H[3]};
        const uint32_t tot = hb[0] + hb[1] + hb[2] + hb[3];
        uint32_t inc = tot;  // the inclusive scan over the lanes' totals
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t u = __shfl_up(inc, o);
            if (lane >= o) inc += u;
        }
        uint32_t c = inc - tot;  // the samples below the lane's first bin
        int first = 256, last = -1;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (a.npix - c > a.k_hi) last = 4 * lane + j;  // the sum from this bin up
            c += hb[j];
            if (c > a.k_lo && first == 256) first = 4 * lane + j;  // the sum up to this bin
        }
        lo_m = wave_min_i(first);
        hi_m = wave_max_i(last);
        int has = 0;
        int32_t *st = a.state ? a.state + 4 * f : nullptr;
        if (st) { has = st[0]; lo_s = st[1]; hi_s = st[2]; }  // every lane the same words, in front of lane 0's stores
        if (!has) { lo_s = lo_m << 8; hi_s = hi_m << 8; }
        else { lo_s = levels_follow(lo_s, lo_m, p.speed); hi_s = levels_follow(hi_s, hi_m, p.speed); }
        if (st && lane == 0) { st[0] = 1; st[1] = lo_s; st[2] = hi_s; st[3] = 0; }
        levels_limit(lo_s, hi_s, p.out_hi - p.out_lo, p.max_gain, lo_e, hi_e);
        if (a.record) {  // the same in every lane
            uint32_t b = 0, ab = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int v8 = (4 * lane + j) << 8;
                if (v8 < lo_e) b += hb[j];
                if (v8 > hi_e) ab += hb[j];
            }
            below = wave_sum(b);
            above = wave_sum(ab);
        }
    } else {
        lo_e = p.in_lo << 8;
        hi_e = p.in_hi << 8;
    }
    uint32_t y4 = 0, c4 = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        y4 |= (uint32_t)levels_luma(4 * lane + j, lo_e, hi_e, p.out_lo, p.out_hi) << (8 * j);
        c4 |= (uint32_t)levels_chroma(4 * lane + j, p.sat) << (8 * j);
    }
    uint32_t *T = (uint32_t *)(a.luts + 768 * f);
    T[lane] = y4; T[64 + lane] = c4; T[128 + lane] = c4;
    if (a.record && lane == 0) {
        int32_t *r = a.record + 8 * f;
        r[0] = lo_m; r[1] = hi_m; r[2] = lo_s; r[3] = hi_s; r[4] = lo_e; r[5] = hi_e; r[6] = (int32_t)below; r[7] = (int32_t)above;
    }
}

// ---- host
// the definitions on the host as plain loops
void hist_frame_host(uint32_t *hist, const uint8_t *frame, int w, int h) {
    const size_t len[3] = {(size_t)w * h, (size_t)(w / 2) * (h / 2), (size_t)(w / 2) * (h / 2)};
    memset(hist, 0, 768 * sizeof(uint32_t));
    const uint8_t *P = frame;
    for (int pl = 0; pl < 3; P += len[pl], pl++)
        for (size_t i = 0; i < len[pl]; i++) hist[256 * pl + P[i]]++;
}
void lut_frame_host(uint8_t *dst, const uint8_t *src, int w, int h, const uint8_t *lut768) {
    const size_t len[3] = {(size_t)w * h, (size_t)(w / 2) * (h / 2), (size_t)(w / 2) * (h / 2)};
    size_t at = 0;
    for (int pl = 0; pl < 3; at += len[pl], pl++)
        for (size_t i = 0; i < len[pl]; i++) dst[at + i] = lut768[256 * pl + src[at + i]];
}
// hist_y: the 256 luma words (AUTO); state4 and record8 may be null
void levels_lut_host(uint8_t *lut768, const uint32_t *hist_y, int w, int h, const h264mi_levels &p, int32_t *state4, int32_t *record8) {
    int lo_m = 0, hi_m = 0, lo_s = 0, hi_s = 0, lo_e, hi_e;
    uint32_t below = 0, above = 0;
    if (p.mode == H264MI_LEVELS_AUTO) {
        const uint32_t k_lo = levels_clip_count(p.clip_lo, w, h), k_hi = levels_clip_count(p.clip_hi, w, h);
        uint32_t c = 0;
        for (lo_m = 0; lo_m < 255; lo_m++)
            if ((c += hist_y[lo_m]) > k_lo) break;
        c = 0;
        for (hi_m = 255; hi_m > 0; hi_m--)
            if ((c += hist_y[hi_m]) > k_hi) break;
        if (!state4 || !state4[0]) { lo_s = lo_m << 8; hi_s = hi_m << 8; }
        else { lo_s = levels_follow(state4[1], lo_m, p.speed); hi_s = levels_follow(state4[2], hi_m, p.speed); }
        if (state4) { state4[0] = 1; state4[1] = lo_s; state4[2] = hi_s; state4[3] = 0; }
        levels_limit(lo_s, hi_s, p.out_hi - p.out_lo, p.max_gain, lo_e, hi_e);
        for (int v = 0; v < 256; v++) {
            if ((v << 8) < lo_e) below += hist_y[v];
            if ((v << 8) > hi_e) above += hist_y[v];
        }
    } else {
        lo_e = p.in_lo << 8;
        hi_e = p.in_hi << 8;
    }
    for (int v = 0; v < 256; v++) {
        lut768[v] = (uint8_t)levels_luma(v, lo_e, hi_e, p.out_lo, p.out_hi);
        lut768[256 + v] = lut768[512 + v] = (uint8_t)levels_chroma(v, p.sat);
    }
    if (record8) {
        const int32_t r[8] = {lo_m, hi_m, lo_s, hi_s, lo_e, hi_e, (int32_t)below, (int32_t)above};
        memcpy(record8, r, sizeof r);
    }
}

static LevelsGrid levels_grid(int w, int h, int n) {
    LevelsGrid g{};
    const size_t ly = (size_t)w * h, lc = (size_t)(w / 2) * (h / 2);
    g.fb = ly + 2 * lc;
    g.off[0] = 0; g.off[1] = ly; g.off[2] = ly + lc;
    g.len[0] = (uint32_t)ly; g.len[1] = g.len[2] = (uint32_t)lc;
    g.per_frame = 0;
    for (int pl = 0; pl < 3; pl++) {
        g.nch[pl] = (int)((g.len[pl] + (LV_UNIT - 1) + LV_CHUNK - 1) / LV_CHUNK);  // the plane 15 bytes past a multiple of 16
        g.per_frame += g.nch[pl];
    }
    g.items = (long long)n * g.per_frame;
    const long long blocks = std::min(g.items, (long long)PIC_MAX_BLOCKS);
    g.per = (g.items + blocks - 1) / blocks;
    return g;
}
static inline unsigned levels_blocks(const LevelsGrid &g) { return (unsigned)((g.items + g.per - 1) / g.per); }

// n tight w x h I420 frames: arguments as hist_args_ok accepts them. One memset and one launch
int launch_hist_i420(uint32_t *hist, const uint8_t *frames, int w, int h, int n, hipStream_t s) {
    HistLaunch a{frames, hist, levels_grid(w, h, n)};
    if (hipMemsetAsync(hist, 0, (size_t)n * LEVELS_HIST_BYTES, s) != hipSuccess) return -1;
    (void)hipGetLastError();
    hipLaunchKernelGGL(hist_kernel, dim3(levels_blocks(a.g)), dim3(256), 0, s, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
// arguments as lut_args_ok accepts them. One launch
int launch_lut_i420(uint8_t *dst, const uint8_t *src, int w, int h, int n, const uint8_t *luts, int per_frame, hipStream_t s) {
    LutLaunch a{src, dst, luts, per_frame ? LEVELS_LUT_BYTES : 0, levels_grid(w, h, n)};
    (void)hipGetLastError();
    hipLaunchKernelGGL(lut_kernel, dim3(levels_blocks(a.g)), dim3(256), 0, s, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
// the decision for n frames: a wave each. hist is null in FIXED mode, which reads nothing but p
int launch_levels_decide(uint8_t *luts, const uint32_t *hist, int32_t *state, int32_t *record, int w, int h, int n, const h264mi_levels &p,
                         hipStream_t s) {
    DecideLaunch a{luts, hist, state, record, (uint32_t)w * (uint32_t)h, levels_clip_count(p.clip_lo, w, h), levels_clip_count(p.clip_hi, w, h), p};
    (void)hipGetLastError();
    hipLaunchKernelGGL(levels_decide_kernel, dim3((unsigned)n), dim3(64), 0, s, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
// arguments as levels_args_ok accepts them. work: n histograms, then n table sets
int launch_levels_i420(uint8_t *dst, const uint8_t *src, int w, int h, int n, const h264mi_levels &p, int32_t *state, int32_t *record,
                       uint8_t *work, hipStream_t s) {
    uint32_t *hist = (uint32_t *)work;
    uint8_t *luts = work + (size_t)n * LEVELS_HIST_BYTES;
    const bool autom = p.mode == H264MI_LEVELS_AUTO;
    if (autom && launch_hist_i420(hist, src, w, h, n, s) != 0) return -1;
    if (launch_levels_decide(luts, autom ? hist : nullptr, state, record, w, h, n, p, s) != 0) return -1;
    return launch_lut_i420(dst, src, w, h, n, luts, 1, s);
}
}  // namespace h264mi
